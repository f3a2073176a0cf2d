#!/usr/bin/env python3
"""Device-event timing of the on-policy rollout buffer: insertion, the advantage recursion, one epoch of minibatches, and the same three
written with stock PyTorch ops.

    python tools/rollout_bench.py [--envs 8192] [--steps 64] [--batch 4096] [--reps 20] [--parent-lib PATH] [--out profiles/rollout/rollout_bench.json]

Setup: --envs environments of MyCobotReach-Dense-joint-v0 driven by a seeded random policy (random values and log-probabilities) for
--steps steps into a RolloutBuffer; 50 further step outputs are kept and cycled through, so that every environment's episode is at its
own phase.  Paths, each measured in a process of its own (parent: this script; children: --path NAME), warm-up calls and then `reps`
windows of `inner` back-to-back calls between two events on the launch stream; reported: median and min / max of the per-call time:

    add          RolloutBuffer.add(...) on kept step outputs (the step itself is not in the window): the public call, Python included
    add_raw      mcg_rollout_add alone, on the same kept outputs
    gae          RolloutBuffer.finish(last_values): mcg_rollout_gae over the full buffer
    get          one epoch, `for mb in buf.get(batch)`: M / batch launches of mcg_rollout_gather and their output allocations
    torch_add    the same insertion into preallocated [T, N, ...] tensors by indexed stores, one per field
    torch_gae    the backward loop of T steps in torch ops on [N] rows
    torch_get    torch.randperm(M) and one index op per field and minibatch
    step         the Reach step the insertion follows (step_async, no packaging); with --parent-lib, of that build of the library
                 (MCG_LIB), so that the insertion is held against the parent commit's step in the same run

The PyTorch formulations live in this tool only: they are what a user writes without the mcg_rollout_* calls.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402
from mycobotgym_amd import _abi  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # bench.py's
ENV_ID = "MyCobotReach-Dense-joint-v0"
GAMMA, LAMBDA = 0.99, 0.95
PATHS = ("add", "add_raw", "gae", "get", "torch_add", "torch_gae", "torch_get", "step")


def rollout(envs, n_steps, seed, buf=None):
    """n_steps steps of a seeded random policy; -> the kept (a, v, logp, final_values, step outputs), inserted into `buf` if given."""
    g = torch.Generator(device="cpu"); g.manual_seed(seed)
    n, dev = envs.num_envs, envs.device
    kept = []
    for _ in range(n_steps):
        a = (torch.rand(n, envs.action_dim, generator=g) * 2 - 1).to(dev)
        v, lp, fv = (torch.randn(n, generator=g).to(dev) for _ in range(3))
        out = envs.step(a)
        if buf is not None:
            buf.add(a, v, lp, *out, final_values=fv)
        kept.append((a, v, lp, fv, out))
    return kept


class TorchRollout:
    """The buffer from stock PyTorch ops: one preallocated [T, N, ...] tensor per field."""

    def __init__(self, n, D, A, T, dev):
        f = dict(dtype=torch.float32, device=dev)
        self.n, self.T = n, T
        self.obs, self.ach, self.des = torch.zeros(T, n, D, **f), torch.zeros(T, n, 3, **f), torch.zeros(T, n, 3, **f)
        self.act = torch.zeros(T, n, A, **f)
        self.logp, self.val, self.rew, self.adv, self.ret = (torch.zeros(T, n, **f) for _ in range(5))
        self.start = torch.zeros(T, n, **f)
        self.last_obs, self.last_ach, self.last_des = torch.zeros(n, D, **f), torch.zeros(n, 3, **f), torch.zeros(n, 3, **f)
        self.last_start = torch.ones(n, **f)

    def add(self, pos, a, v, lp, fv, out):
        obs, r, term, trunc, _ = out
        self.obs[pos] = self.last_obs; self.ach[pos] = self.last_ach; self.des[pos] = self.last_des
        self.act[pos] = a; self.logp[pos] = lp; self.val[pos] = v; self.start[pos] = self.last_start
        self.rew[pos] = torch.where(trunc & ~term, r.float() + GAMMA * fv, r.float())
        self.last_obs, self.last_ach, self.last_des = obs["observation"].float(), obs["achieved_goal"].float(), obs["desired_goal"].float()
        self.last_start = (term | trunc).float()

    def gae(self, last_values):
        last = torch.zeros_like(last_values)
        for t in reversed(range(self.T)):
            nnt = 1.0 - (self.last_start if t == self.T - 1 else self.start[t + 1])
            vn = last_values if t == self.T - 1 else self.val[t + 1]
            delta = self.rew[t] + GAMMA * vn * nnt - self.val[t]
            last = delta + GAMMA * LAMBDA * nnt * last
            self.adv[t] = last
        torch.add(self.adv, self.val, out=self.ret)

    def get(self, batch):
        M = self.T * self.n
        perm = torch.randperm(M, device=self.obs.device)
        flat = [x.view(M, *x.shape[2:]) for x in (self.obs, self.ach, self.des, self.act, self.val, self.logp, self.adv, self.ret)]
        for first in range(0, M, batch):
            idx = perm[first:first + batch]
            yield tuple(x[idx] for x in flat) + (idx,)


def child(args):
    if not torch.cuda.is_available():
        sys.exit("rollout_bench needs the GPU: a timing taken anywhere else says nothing")
    envs = mg.make(ENV_ID, num_envs=args.envs, seed=1)
    obs, _ = envs.reset(seed=1)
    n, D, A, T, dev = envs.num_envs, envs.obs_dim, envs.action_dim, args.steps, envs.device
    r = {}
    if args.path == "step":
        a = torch.rand(n, A, device=dev) * 2 - 1
        r = timed(lambda: envs.step_async(a), warmup=20, reps=args.reps, inner=50)
        r["library"] = os.path.relpath(_abi.LIB_PATH, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    elif args.path.startswith("torch_"):
        tb = TorchRollout(n, D, A, T, dev)
        tb.last_obs, tb.last_ach, tb.last_des = obs["observation"].float(), obs["achieved_goal"].float(), obs["desired_goal"].float()
        for pos, k in enumerate(rollout(envs, T, 0)):
            tb.add(pos, *k)
        lv = torch.randn(n, device=dev)
        tb.gae(lv)
        if args.path == "torch_add":
            cycle, state = itertools.cycle(rollout(envs, envs.max_episode_steps, 1)), {"pos": 0}

            def add():
                tb.add(state["pos"], *next(cycle))
                state["pos"] = (state["pos"] + 1) % T
            r = timed(add, warmup=5, reps=args.reps, inner=20)
        elif args.path == "torch_gae":
            r = timed(lambda: tb.gae(lv), warmup=3, reps=args.reps, inner=5)
        else:
            def epoch():
                for _ in tb.get(args.batch):
                    pass
            r = timed(epoch, warmup=3, reps=args.reps, inner=2)
    else:
        buf = mg.RolloutBuffer(envs, n_steps=T, gamma=GAMMA, gae_lambda=LAMBDA, seed=0)
        buf.start(obs)
        rollout(envs, T, 0, buf)
        lv = torch.randn(n, device=dev)
        buf.finish(lv)
        r_bytes = buf.record_bytes
        if args.path in ("add", "add_raw"):
            kept = rollout(envs, envs.max_episode_steps, 1)
            if args.path == "add":
                cycle = itertools.cycle(kept)

                def add():
                    if buf.full:
                        buf.reset()
                    a, v, lp, fv, out = next(cycle)
                    buf.add(a, v, lp, *out, final_values=fv)
                r = timed(add, warmup=5, reps=args.reps, inner=20)
            else:
                lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
                raw = []
                for a, v, lp, fv, (o, rew, term, trunc, info) in kept:
                    rew = rew.double()
                    raw.append((a, v, lp, fv, rew, _abi.McgStepOut(obs=o["observation"].data_ptr(), achieved_goal=o["achieved_goal"].data_ptr(),
                                                                   desired_goal=o["desired_goal"].data_ptr(), reward=rew.data_ptr(),
                                                                   terminated=term.data_ptr(), truncated=trunc.data_ptr())))
                cycle, state = itertools.cycle(raw), {"pos": 0}

                def add_raw():
                    a, v, lp, fv, _, out = next(cycle)
                    _abi.check(lib.mcg_rollout_add(C.byref(buf._cbuf), state["pos"], C.c_void_p(a.data_ptr()), C.c_void_p(v.data_ptr()),
                                                   C.c_void_p(lp.data_ptr()), C.c_void_p(fv.data_ptr()), C.byref(out), stream), "mcg_rollout_add")
                    state["pos"] = (state["pos"] + 1) % T
                r = timed(add_raw, warmup=5, reps=args.reps, inner=20)
            # written: the record and three plane words; read and written: last_obs, last_goals, last_start; read: the step's float64 outputs
            r["bytes_per_env"] = r_bytes + 9 + 2 * (4 * (D + 6) + 1) + 8 * (D + 6 + 1) + 2 + 4 * (A + 3)
            r["gbps"] = r["bytes_per_env"] * n / (r["median_ms"] * 1e-3) / 1e9
        elif args.path == "gae":
            r = timed(lambda: buf.finish(lv), warmup=3, reps=args.reps, inner=5)
            r["bytes_per_transition"] = 4 + 4 + 1 + 4 + 4
            r["gbps"] = r["bytes_per_transition"] * n * T / (r["median_ms"] * 1e-3) / 1e9
        elif args.path == "get":
            def epoch():
                for _ in buf.get(args.batch):
                    pass
            r = timed(epoch, warmup=3, reps=args.reps, inner=2)
            r["bytes_per_sample"] = r_bytes + 12 + 4 * (D + 6 + A + 1) + 16
            r["gbps"] = r["bytes_per_sample"] * n * T / (r["median_ms"] * 1e-3) / 1e9
            r["launches_per_epoch"] = -(-n * T // args.batch)
        else:
            sys.exit(f"unknown path {args.path!r}")
        r["record_bytes"] = r_bytes
    if "gbps" in r:
        r["hbm_peak_gbps"] = HBM_PEAK_GBPS
    r.update(path=args.path, env_id=ENV_ID, envs=args.envs, steps=args.steps, batch=args.batch, device=torch.cuda.get_device_name(0))
    print(json.dumps(r), flush=True)
    envs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--parent-lib", default=None, help="another build of the library (the parent commit's) for the `step` path")
    ap.add_argument("--out", default=None)
    ap.add_argument("--path", default=None, help="one path, in this process (what the parent starts)")
    args = ap.parse_args()
    if args.path:
        child(args)
        return
    res = {"cases": []}
    for path in PATHS:
        env = dict(os.environ)
        if path == "step" and args.parent_lib:
            env["MCG_LIB"] = os.path.abspath(args.parent_lib)
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--path", path, "--envs", str(args.envs), "--steps", str(args.steps),
                            "--batch", str(args.batch), "--reps", str(args.reps)], capture_output=True, text=True, timeout=280, env=env)
        if p.returncode != 0:
            sys.exit(f"{path}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")      # nothing more is started
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line); res["cases"].append(r); print(json.dumps(r), flush=True)
    by = {r["path"]: r for r in res["cases"]}
    faster = lambda hip, ref: by[ref]["median_ms"] - by[hip]["median_ms"] > by[ref]["max_ms"] - by[ref]["min_ms"]
    res["acceptance"] = {"add_faster_than_torch_beyond_its_spread": faster("add", "torch_add"),
                         "gae_faster_than_torch_beyond_its_spread": faster("gae", "torch_gae"),
                         "get_faster_than_torch_beyond_its_spread": faster("get", "torch_get"),
                         "add_below_the_reach_step": by["add"]["median_ms"] < by["step"]["median_ms"]}
    print(json.dumps(res["acceptance"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
