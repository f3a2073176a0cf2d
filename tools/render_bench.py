#!/usr/bin/env python3
"""Device-event timing of mcg_render next to the step of the same engine.

    python tools/render_bench.py [--envs 8192] [--reps 20] [--out profiles/render/render_bench.json]

Per case (64 x 64 at samples 1, 2, 4 on --envs environments; 480 x 480 on 256): warm-up launches, then `reps` windows of `inner`
back-to-back launches between two events on the launch stream; reported: median and spread of the per-launch time.  The states are
a seeded random-policy rollout with desynchronised episodes (what a training run renders), not the reset pose.  Also: one step() of
the -v1 image engine (step + render + masked reset + render) against the -v0 state engine of the same configuration.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402


def timed(fn, warmup, reps, inner):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record(); b.synchronize()
        ms.append(a.elapsed_time(b) / inner)
    ms = np.asarray(ms)
    return {"median_ms": float(np.median(ms)), "min_ms": float(ms.min()), "max_ms": float(ms.max()), "reps": reps, "inner": inner}


def rollout(envs, steps, seed=0):
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    for _ in range(steps):
        envs.step(torch.rand(envs.num_envs, envs.action_dim, generator=g) * 2 - 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="reach-joint,pnp-joint")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("render_bench needs the GPU: a timing taken anywhere else says nothing")
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "cases": []}
    for cfg in args.configs.split(","):
        task, ctrl = cfg.split("-")
        name = f"MyCobot{'Reach' if task == 'reach' else 'PickAndPlace'}-Dense-{ctrl}"
        for n, w, h, samples in ((args.envs, 64, 64, 1), (args.envs, 64, 64, 2), (args.envs, 64, 64, 4), (256, 480, 480, 1)):
            envs = mg.make(name + "-v0", num_envs=n, seed=1)
            envs.reset(seed=1)
            rollout(envs, 30)
            out = {"gray": torch.zeros(n, h, w, dtype=torch.uint8, device=envs.device)} if samples > 1 or w == 64 else \
                  {"rgb": torch.zeros(n, h, w, 3, dtype=torch.uint8, device=envs.device)}
            r = timed(lambda: envs.render_into(out, samples=samples), warmup=5, reps=args.reps, inner=10)
            rays = n * w * h * samples * samples
            r.update(config=cfg, what="mcg_render", envs=n, width=w, height=h, samples=samples, output=list(out)[0],
                     grays_per_s=rays / (r["median_ms"] * 1e-3) / 1e9)
            res["cases"].append(r); print(json.dumps(r), flush=True)
            envs.close()
        # one step of the engine with and without pictures
        v0 = mg.make(name + "-v0", num_envs=args.envs, seed=1); v1 = mg.make(name + "-v1", num_envs=args.envs, seed=1)
        for e, what in ((v0, "step -v0"), (v1, "step -v1 (step + render + masked reset + render, samples 2)")):
            e.reset(seed=1)
            rollout(e, 30)
            a = torch.rand(args.envs, e.action_dim, device=e.device) * 2 - 1
            r = timed(lambda: e.step(a, copy=False), warmup=5, reps=args.reps, inner=10)
            r.update(config=cfg, what=what, envs=args.envs)
            res["cases"].append(r); print(json.dumps(r), flush=True)
            e.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
