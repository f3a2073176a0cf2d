#!/usr/bin/env python3
"""Device-event timing of the CNN actor-critic forward (mycobotgym_amd.CnnActorCritic) against the same policy in eager PyTorch, and of
the on-policy collection loop of a -v1 picture id with each.

    python tools/cnn_policy_bench.py [--envs 8192] [--batch 4096] [--reps 10] [--inner 20] [--out profiles/cnn_policy/cnn_policy_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream; reported: median and min / max of the per-call time (the spread from window to window).  Shapes: S = 64, A = 7, F = 512, at
C = 1 (the registered shape) and C = 4 (a stack of four frames).

    forward          a, v, logp = pol(img): the public call, output allocation and Python included
    values           pol.values(img)
    evaluate         pol.evaluate_actions(obs, actions) on `batch` float32 rows (ImageRolloutBuffer.get's default)
    twin_*           the torch twin (tests/indep_cnn.py: SB3's formula in eager float32 on the same GPU, the / 255 included, whatever
                     MIOpen picks after the warm-up) producing the same outputs
    step             the bare envs.step of the -v1 id
    loop             one step of a collection loop on it: policy -> envs.step -> values(final_observation) -> ImageRolloutBuffer.add;
                     loop_twin: the same with the twin
    floor_ms         the arithmetic floor of the forward at the float32 matrix peak (155 TFLOP/s measured): 2 * multiply-adds / peak;
                     x_floor = median / floor
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402
from tests.indep_cnn import Twin, random_pictures, sizes  # noqa: E402

ENV_ID = "MyCobotReach-Sparse-joint-v1"
S, F, A = 64, 512, 7
PEAK = 155e12


def multiply_adds(C, S, F, A):
    o1, o2, o3 = sizes(S)
    return o1 * o1 * 32 * 64 * C + o2 * o2 * 64 * 512 + o3 * o3 * 64 * 576 + 64 * o3 * o3 * F + F * (A + 1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--inner", type=int, default=20)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("cnn_policy_bench needs the GPU: a timing taken anywhere else says nothing")
    n, B, dev = args.envs, args.batch, torch.device("cuda:0")
    t = lambda fn, inner=args.inner: timed(fn, warmup=5, reps=args.reps, inner=inner)
    cases = []

    def report(what, r, rows=None, C=None, **kw):
        if rows is not None:
            r["floor_ms"] = 2.0 * multiply_adds(C, S, F, A) * rows / PEAK * 1e3
            r["x_floor"] = r["median_ms"] / r["floor_ms"]
        r.update(what=what, envs=n, device=torch.cuda.get_device_name(0), **kw)
        cases.append(r)
        print(json.dumps(r), flush=True)

    for C in (1, 4):
        img = torch.from_numpy(random_pictures(n, C, S, seed=0)).to(dev)
        twin = Twin(C, S, F, A).randomize(0).to(dev)
        pol = mg.CnnActorCritic.from_module(twin, num_envs=n, channels=C, image_size=S, act_dim=A, device=dev)
        obs = img[:B].float() / 255.0
        acts = torch.randn(B, A, device=dev)
        kw = dict(channels=C, image_size=S, features_dim=F, act_dim=A)
        with torch.no_grad():
            report("forward", t(lambda: pol(img)), rows=n, C=C, **kw)
            report("values", t(lambda: pol.values(img)), rows=n, C=C, **kw)
            report("evaluate", t(lambda: pol.evaluate_actions(obs, acts)), rows=B, C=C, batch=B, **kw)
            report("twin_forward", t(lambda: twin(img)[:3]), rows=n, C=C, **kw)
            report("twin_values", t(lambda: twin.predict_values(img)), rows=n, C=C, **kw)
            report("twin_evaluate", t(lambda: twin.evaluate_actions(obs, acts)), rows=B, C=C, batch=B, **kw)
        del pol, twin, img, obs

    T = 8
    base = mg.make(ENV_ID, num_envs=n, seed=1)
    for k in (1, 4):
        envs = base if k == 1 else mg.FrameStack(base, k)
        img0, _ = envs.reset(seed=1)
        a0 = torch.rand(n, envs.action_dim, device=dev) * 2 - 1
        report("step", t(lambda: envs.step(a0), inner=T), env_id=ENV_ID, frame_stack=k)
        twin = Twin(envs.channels, envs.image_size, F, envs.action_dim).randomize(0).to(dev)
        pol = mg.CnnActorCritic.from_module(twin, envs)
        for name, policy, value_fn in (("loop", lambda o: pol(o), pol.values), ("loop_twin", lambda o: twin(o)[:3], twin.predict_values)):
            buf = mg.ImageRolloutBuffer(envs, n_steps=T, seed=0, frame_stack=k)
            img0, _ = envs.reset(seed=1)
            buf.start(img0)
            state = {"img": img0}

            def one_step():
                if buf.full:
                    buf.reset()
                a, v, logp = policy(state["img"])
                img, r, term, trunc, info = envs.step(a.clamp(-1, 1) if name == "loop_twin" else a)      # (the engine clips what it reads)
                state["img"] = img
                buf.add(a, v, logp, img, r, term, trunc, info, final_values=value_fn(info["final_observation"]))
            with torch.no_grad():
                report(name, t(one_step, inner=T), env_id=ENV_ID, frame_stack=k, channels=envs.channels, features_dim=F, n_steps=T)
        del pol, twin
    base.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"cases": cases}, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
