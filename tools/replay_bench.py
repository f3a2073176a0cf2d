#!/usr/bin/env python3
"""Device-event timing of the hindsight replay buffer: insertion, sampling, and the same sampling rule in stock PyTorch ops.

    python tools/replay_bench.py [--envs 8192] [--capacity 1000] [--batch 65536] [--reps 20] [--out profiles/replay/replay_bench.json]

Setup: --envs environments of MyCobotPickAndPlace-Sparse-joint-v0 driven by a seeded random policy for capacity + 50 steps into a
HerBuffer of --capacity slots (the ring has wrapped; episodes are the engine's own 50-step ones).  Paths, each measured in a process
of its own (parent: this script; children: --path NAME), warm-up calls and then `reps` windows of `inner` back-to-back calls between
two events on the launch stream; reported: median and min / max of the per-call time:

    add        HerBuffer.add(a, *out) on kept step outputs (the step itself is not in the window): the public call, Python included
    add_raw    mcg_her_add alone, on the same kept outputs
    sample     HerBuffer.sample(batch, check=False)
    torch      the same rule -- rejection among (slot, env) pairs on the episode bookkeeping, `future` relabelling, float32 outputs -- from
               stock PyTorch indexing ops on one tensor per field, without a synchronisation: what a user writes without mcg_her_sample.
               It lives in this tool only.  (Its draws are torch.rand's, not the kernel's Philox: the batches differ, the work does not.)

bytes_per_sample: one record read plus the float32 output rows and the index written; gbps is that over the median, next to the HBM
peak bench.py uses.
"""
import argparse
import json
import os
import subprocess
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402
from mycobotgym_amd import _abi  # noqa: E402

HBM_PEAK_GBPS = 8000.0          # bench.py's
ENV_ID = "MyCobotPickAndPlace-Sparse-joint-v0"
ROUNDS = 6                      # rejection rounds of the PyTorch formulation (fixed: it may not look at the device to stop early)


def filled(args):
    envs = mg.make(ENV_ID, num_envs=args.envs, seed=1)
    buf = mg.HerBuffer(envs, capacity=args.capacity, n_sampled_goal=4, seed=0)
    obs, _ = envs.reset(seed=1)
    buf.start(obs)
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    a = None
    for _ in range(args.capacity + 50):
        a = (torch.rand(envs.num_envs, envs.action_dim, generator=g) * 2 - 1).to(envs.device)
        buf.add(a, *envs.step(a, copy=False))
    torch.cuda.synchronize()
    return envs, buf, a


def field_tensors(buf):
    """The ring as one tensor per field, [capacity, N, ...]: what a PyTorch ring buffer would hold."""
    rec = buf.records()
    dt = _abi.her_record_dtype(buf.obs_dim, buf.act_dim)
    out = {}
    for name in ("achieved", "next_achieved", "desired", "obs", "next_obs", "action", "reward", "t_in_ep", "ep_len", "terminated"):
        fdt, off = dt.fields[name][:2]
        tdt = {"f8": torch.float64, "f4": torch.float32, "i4": torch.int32, "u1": torch.uint8}[fdt.base.str[1:]]
        count = int(np.prod(fdt.shape)) if fdt.shape else 1
        raw = rec[:, :, off:off + count * fdt.base.itemsize].contiguous()
        t = raw.view(tdt)
        out[name] = t if fdt.shape else t[..., 0]
        out[name] = out[name].contiguous()
    return out


def torch_sampler(buf, F, batch):
    cap, N, dev = buf.capacity, buf.num_envs, buf.device
    n = buf.n_written
    W, pos, oldest = min(n, cap), n % cap, max(0, n - cap)
    n_virtual = buf.n_virtual(batch)
    virtual = torch.arange(batch, device=dev) >= batch - n_virtual
    sparse, thr = buf.reward_type == "sparse", buf.distance_threshold

    def sample():
        s = torch.zeros(batch, dtype=torch.int64, device=dev); e = torch.zeros_like(s)
        need = torch.ones(batch, dtype=torch.bool, device=dev)
        for _ in range(ROUNDS):
            cs = (torch.rand(batch, device=dev, dtype=torch.float64) * W).long().clamp_(max=W - 1)
            ce = (torch.rand(batch, device=dev, dtype=torch.float64) * N).long().clamp_(max=N - 1)
            time = n - 1 - torch.remainder(pos - 1 - cs, cap)
            ok = need & (F["ep_len"][cs, ce] > 0) & (time - F["t_in_ep"][cs, ce] >= oldest)
            s = torch.where(ok, cs, s); e = torch.where(ok, ce, e)
            need = need & ~ok
        t, L = F["t_in_ep"][s, e].long(), F["ep_len"][s, e].long()
        f = torch.minimum(L - 1, t + (torch.rand(batch, device=dev, dtype=torch.float64) * (L - t)).long())
        fs = torch.remainder(s + f - t, cap)
        nach = F["next_achieved"][s, e]
        goal = torch.where(virtual[:, None], F["next_achieved"][fs, e], F["desired"][s, e])
        d = (nach - goal).norm(dim=1)
        r = -(d > thr).float() if sparse else (-d).float()
        reward = torch.where(virtual, r, F["reward"][s, e])
        return {"obs": F["obs"][s, e], "achieved": F["achieved"][s, e].float(), "desired": goal.float(), "next_obs": F["next_obs"][s, e],
                "next_achieved": nach.float(), "action": F["action"][s, e], "reward": reward, "done": F["terminated"][s, e].float(),
                "index": torch.stack([s, e, torch.where(virtual, fs, torch.full_like(fs, -1))], dim=1).int(), "gave_up": need}
    return sample


def child(args):
    if not torch.cuda.is_available():
        sys.exit("replay_bench needs the GPU: a timing taken anywhere else says nothing")
    envs, buf, a = filled(args)
    D, A = buf.obs_dim, buf.act_dim
    if args.path in ("add", "add_raw"):
        import ctypes as C
        import itertools
        # 50 further steps, kept: cycling through them keeps every environment's episode at its own phase, so a call back-fills what a
        # training run's does (1 / 50 of the environments end a 50-step episode)
        g = torch.Generator(device="cpu"); g.manual_seed(1)
        kept = []
        for _ in range(envs.max_episode_steps):
            a = (torch.rand(envs.num_envs, envs.action_dim, generator=g) * 2 - 1).to(envs.device)
            kept.append((a, envs.step(a)))
        if args.path == "add":
            cycle = itertools.cycle(kept)

            def add():
                a, out = next(cycle)
                buf.add(a, *out)
            r = timed(add, warmup=5, reps=args.reps, inner=20)
        else:
            lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(envs.device).cuda_stream)
            raw = []
            for a, (o, rew, term, trunc, info) in kept:
                fin, rew = info["final_observation"], rew.double()
                raw.append((a, rew, _abi.McgStepOut(obs=o["observation"].data_ptr(), achieved_goal=o["achieved_goal"].data_ptr(),
                                                    desired_goal=o["desired_goal"].data_ptr(), reward=rew.data_ptr(), terminated=term.data_ptr(),
                                                    truncated=trunc.data_ptr(), final_obs=fin["observation"].data_ptr(),
                                                    final_achieved=fin["achieved_goal"].data_ptr(), final_desired=fin["desired_goal"].data_ptr())))
            cycle, state = itertools.cycle(raw), {"n": buf.n_written}

            def add_raw():
                a, _, out = next(cycle)
                _abi.check(lib.mcg_her_add(C.byref(buf._cbuf), state["n"], C.c_void_p(a.data_ptr()), C.byref(out), stream), "mcg_her_add")
                state["n"] += 1
            r = timed(add_raw, warmup=5, reps=args.reps, inner=20)
        r["bytes_per_env"] = buf.record_bytes + 8 * (2 * D + 9 + 1) + 4 * A + 2 + 4 * D + 24
        r["gbps"] = r["bytes_per_env"] * buf.num_envs / (r["median_ms"] * 1e-3) / 1e9
        r["overlong_episodes"] = buf.counters()["overlong_episodes"]
    elif args.path == "sample":
        r = timed(lambda: buf.sample(args.batch, check=False), warmup=3, reps=args.reps, inner=5)
        r["give_ups"] = buf.counters()["sample_give_ups"]
    elif args.path == "torch":
        fn = torch_sampler(buf, field_tensors(buf), args.batch)
        r = timed(fn, warmup=3, reps=args.reps, inner=5)
        r["give_ups_last_call"] = int(fn()["gave_up"].sum())
        r["rounds"] = ROUNDS
    else:
        sys.exit(f"unknown path {args.path!r}")
    if args.path in ("sample", "torch"):
        r["bytes_per_sample"] = buf.record_bytes + 4 * (2 * D + A + 9 + 2) + 12
        r["gbps"] = r["bytes_per_sample"] * args.batch / (r["median_ms"] * 1e-3) / 1e9
        r["hbm_peak_gbps"] = HBM_PEAK_GBPS
    r.update(path=args.path, env_id=ENV_ID, envs=args.envs, capacity=args.capacity, batch=args.batch, record_bytes=buf.record_bytes,
             n_written=buf.n_written, device=torch.cuda.get_device_name(0))
    print(json.dumps(r), flush=True)
    envs.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--capacity", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=65536)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    ap.add_argument("--path", default=None, help="one path, in this process (what the parent starts)")
    args = ap.parse_args()
    if args.path:
        child(args)
        return
    res = {"cases": []}
    for path in ("add", "add_raw", "sample", "torch"):
        p = subprocess.run([sys.executable, os.path.abspath(__file__), "--path", path, "--envs", str(args.envs), "--capacity", str(args.capacity),
                            "--batch", str(args.batch), "--reps", str(args.reps)], capture_output=True, text=True, timeout=280)
        if p.returncode != 0:
            sys.exit(f"{path}: exit {p.returncode}\n{p.stdout[-2000:]}\n{p.stderr[-2000:]}")      # nothing more is started
        for line in p.stdout.splitlines():
            if line.startswith("{"):
                r = json.loads(line); res["cases"].append(r); print(json.dumps(r), flush=True)
    by = {r["path"]: r for r in res["cases"]}
    res["acceptance"] = {
        "sample_not_slower_than_torch_beyond_its_spread": by["sample"]["median_ms"] <= by["torch"]["median_ms"] + (by["torch"]["max_ms"] - by["torch"]["min_ms"]),
        "add_below_reach_step_0.20_ms": by["add"]["median_ms"] < 0.20}
    print(json.dumps(res["acceptance"]), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
