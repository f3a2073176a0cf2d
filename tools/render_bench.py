#!/usr/bin/env python3
"""Device-event timing of mcg_render next to the step of the same engine.

    python tools/render_bench.py [--envs 8192] [--reps 20] [--out profiles/render/render_bench.json]
    python tools/render_bench.py --alternate-against ab/parent/libmycobot_hip.so [--rounds 3] [--out ...]

Per case (64 x 64 at samples 1, 2, 4 on --envs environments; 480 x 480 on 256): warm-up launches, then `reps` windows of `inner`
back-to-back launches between two events on the launch stream; reported: median and spread of the per-launch time.  The states are
a seeded random-policy rollout with desynchronised episodes (what a training run renders), not the reset pose.  Also: one step() of
the -v1 image engine (step + render + masked reset + render) against the -v0 state engine of the same configuration.  The camera is
`sideview`; the 64 x 64 cases at samples 1 and 2 are measured from `gripper_camera_rgb` (the camera on the flange) as well, and both
again with one scene per environment (mcg_render_scenes on a table drawn by mcg_scene_randomize, whose own time is a row too), and the
-v1 step with visual_randomization.

--alternate-against LIB: the world-camera case (sideview, 64 x 64, samples 1 and 2) of this build and of another build of the library
(the parent commit's), alternated `rounds` times in one call, each measurement in a process of its own (the library is chosen through
MCG_LIB when the package is imported).  A world-camera picture must cost what it cost before the mounted camera: the medians are to lie
within the other build's own min-max spread.
"""
import argparse
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402


def rollout(envs, steps, seed=0):
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    for _ in range(steps):
        envs.step(torch.rand(envs.num_envs, envs.action_dim, generator=g) * 2 - 1)


def env_name(cfg):
    task, ctrl = cfg.split("-")
    return f"MyCobot{'Reach' if task == 'reach' else 'PickAndPlace'}-Dense-{ctrl}"


# the ranges of the per-environment rows: those of tests/test_gpu_scene_rand.py (the gripper camera moves less: it is 5 cm from what it sees)
VISUAL = {"cam_pos": 0.05, "cam_rot": 0.0873, "fovy_scale": (0.9, 1.1), "light_tilt": 0.5236, "light_ambient_scale": (0.7, 1.3),
          "light_diffuse_scale": (0.7, 1.3), "head_scale": (0.7, 1.3), "rgb": 0.1}
VISUAL_MOUNTED = dict(VISUAL, cam_pos=0.005, cam_rot=0.0349)


def render_case(cfg, n, w, h, samples, camera, reps, scenes=False):
    envs = mg.make(env_name(cfg) + "-v0", num_envs=n, seed=1)
    envs.reset(seed=1)
    rollout(envs, 30)
    out = {"gray": torch.zeros(n, h, w, dtype=torch.uint8, device=envs.device)} if samples > 1 or w == 64 else \
          {"rgb": torch.zeros(n, h, w, 3, dtype=torch.uint8, device=envs.device)}
    more = {}
    if scenes:       # one scene per environment; validate=False: the timing is the launch's
        more = dict(scenes=envs.randomize_scenes(VISUAL if camera == "sideview" else VISUAL_MOUNTED, camera=camera), validate=False)
    r = timed(lambda: envs.render_into(out, camera=camera, samples=samples, **more), warmup=5, reps=reps, inner=10)
    rays = n * w * h * samples * samples
    what = "mcg_render_scenes" if scenes else ("mcg_render" if camera == "sideview" else "mcg_render_mounted")
    r.update(config=cfg, what=what, camera=camera, envs=n, width=w, height=h,
             samples=samples, output=list(out)[0], grays_per_s=rays / (r["median_ms"] * 1e-3) / 1e9)
    envs.close()
    return r


def randomize_case(cfg, n, reps):
    envs = mg.make(env_name(cfg) + "-v0", num_envs=n, seed=1)
    envs.reset(seed=1)
    rollout(envs, 30)
    tab = envs.randomize_scenes(VISUAL)
    r = timed(lambda: envs.randomize_scenes(VISUAL, out=tab), warmup=5, reps=reps, inner=10)
    r.update(config=cfg, what="mcg_scene_randomize", camera="sideview", envs=n)
    envs.close()
    return r


def alternate(args):
    """This build against another one, world camera: rounds x (other, this), every measurement in its own process."""
    me = os.path.abspath(__file__)
    res = {"alternation": True, "against": args.alternate_against, "envs": args.envs, "cases": []}
    for k in range(args.rounds):
        for which, lib in (("other", os.path.abspath(args.alternate_against)), ("this", None)):
            env = dict(os.environ)
            env.pop("MCG_LIB", None)
            if lib:
                env["MCG_LIB"] = lib
            p = subprocess.run([sys.executable, me, "--world-only", "--envs", str(args.envs), "--reps", str(args.reps), "--configs", args.configs],
                               env=env, capture_output=True, text=True, timeout=300)
            if p.returncode != 0:
                sys.exit(f"round {k}, {which} build: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")      # nothing more is started
            for line in p.stdout.splitlines():
                if line.startswith("{"):
                    r = json.loads(line); r.update(build=which, round=k)
                    res["cases"].append(r); print(json.dumps(r), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--configs", default="reach-joint,pnp-joint")
    ap.add_argument("--out", default=None)
    ap.add_argument("--alternate-against", default=None, metavar="LIB", help="another build of libmycobot_hip.so (the parent commit's)")
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--world-only", action="store_true", help="the world-camera 64 x 64 cases at samples 1 and 2 alone (a child of --alternate-against)")
    args = ap.parse_args()
    if args.alternate_against:
        res = alternate(args)
        write(args.out, res)
        return
    if not torch.cuda.is_available():
        sys.exit("render_bench needs the GPU: a timing taken anywhere else says nothing")
    res = {"device": torch.cuda.get_device_name(0), "envs": args.envs, "cases": []}
    for cfg in args.configs.split(","):
        name = env_name(cfg)
        cases = [(args.envs, 64, 64, 1, "sideview", False), (args.envs, 64, 64, 2, "sideview", False)]
        if not args.world_only:
            cases += [(args.envs, 64, 64, 4, "sideview", False), (256, 480, 480, 1, "sideview", False),
                      (args.envs, 64, 64, 1, "gripper_camera_rgb", False), (args.envs, 64, 64, 2, "gripper_camera_rgb", False),
                      (args.envs, 64, 64, 1, "sideview", True), (args.envs, 64, 64, 2, "sideview", True),
                      (args.envs, 64, 64, 1, "gripper_camera_rgb", True), (args.envs, 64, 64, 2, "gripper_camera_rgb", True)]
        for n, w, h, samples, camera, scenes in cases:
            r = render_case(cfg, n, w, h, samples, camera, args.reps, scenes)
            res["cases"].append(r); print(json.dumps(r), flush=True)
        if args.world_only:
            continue
        r = randomize_case(cfg, args.envs, args.reps)
        res["cases"].append(r); print(json.dumps(r), flush=True)
        # one step of the engine with and without pictures
        v0 = mg.make(name + "-v0", num_envs=args.envs, seed=1); v1 = mg.make(name + "-v1", num_envs=args.envs, seed=1)
        vr = mg.make(name + "-v1", num_envs=args.envs, seed=1, visual_randomization=VISUAL)
        for e, what in ((v0, "step -v0"), (v1, "step -v1 (step + render + masked reset + render, samples 2)"),
                        (vr, "step -v1 with visual_randomization (step + render + masked reset + masked draw of the table + render, samples 2)")):
            e.reset(seed=1)
            rollout(e, 30)
            a = torch.rand(args.envs, e.action_dim, device=e.device) * 2 - 1
            r = timed(lambda: e.step(a, copy=False), warmup=5, reps=args.reps, inner=10)
            r.update(config=cfg, what=what, envs=args.envs)
            res["cases"].append(r); print(json.dumps(r), flush=True)
            e.close()
    write(args.out, res)


def write(path, res):
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
