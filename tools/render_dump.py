#!/usr/bin/env python3
"""A contact sheet of a few environments for a human to look at.

    python tools/render_dump.py [--id MyCobotPickAndPlace-Dense-IK-v0] [--envs 8] [--steps 20] [--size 240] [--out sheet]

Writes <out>.npy (uint8 [rows * H, cameras * W, 3]: one row per environment, one column per world camera) and <out>.png where an
image writer (PIL or matplotlib) is importable.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--id", default="MyCobotPickAndPlace-Dense-IK-v0")
    ap.add_argument("--envs", type=int, default=8)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--size", type=int, default=240)
    ap.add_argument("--samples", type=int, default=2)
    ap.add_argument("--out", default="sheet")
    args = ap.parse_args()
    envs = mg.make(args.id, num_envs=args.envs, seed=0)
    envs.reset(seed=0)
    g = torch.Generator(); g.manual_seed(0)
    for _ in range(args.steps):
        envs.step(torch.rand(args.envs, envs.action_dim, generator=g) * 2 - 1)
    cams = sorted(mg.load_scene()["cameras"])
    cols = [envs.render(camera=c, width=args.size, height=args.size, samples=args.samples).cpu().numpy() for c in cams]
    sheet = np.concatenate([np.concatenate(list(c), axis=0) for c in cols], axis=1)
    np.save(args.out + ".npy", sheet)
    print(f"{args.out}.npy: {sheet.shape}, columns {cams}")
    try:
        from PIL import Image
        Image.fromarray(sheet).save(args.out + ".png")
        print(args.out + ".png")
    except ImportError:
        try:
            import matplotlib.image
            matplotlib.image.imsave(args.out + ".png", sheet)
            print(args.out + ".png")
        except ImportError:
            print("no image writer importable: the .npy only")
    envs.close()


if __name__ == "__main__":
    main()
