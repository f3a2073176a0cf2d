#!/usr/bin/env python3
"""Device-event timing of stacked gathers from the picture rollout buffer: ImageRolloutBuffer(fs, frame_stack=k), which stores single
frames, against the same buffer storing the wrapper's whole stacks as k * C channels -- memory, insertion, the carry between two
rollouts and the minibatch gather -- and against the same rule written with stock PyTorch ops, all in one process.

    python tools/rollout_img_stacked_bench.py [--envs 8192] [--size 64] [--stack 4] [--steps 32] [--batch 4096] [--reps 20] [--out profiles/rollout_img_stacked/rollout_img_stacked_bench.json]

Setup: a FrameStack of --stack frames around --envs environments of MyCobotReach-Dense-joint-v1 (one camera, --size x --size, the
registered time limit of 50) driven by a seeded random policy for two rollouts of --steps steps into both buffers, with reset() between
them, so the second rollout's first steps reach into carried rows and the time limit has ended an episode of every environment.  The
two buffers share the seed, so they hand out the same permutation: before any timing every minibatch of an epoch is compared, bit for
bit, uint8 and float32, and one minibatch with the PyTorch formulation on the same indices.  Every path: warm-up calls, then `reps`
windows of `inner` back-to-back calls between two events on the launch stream; each pair of kernels in alternating rounds.  Reported:
median and min / max of the per-call time, and the algorithmic bytes over the median (N environments, B samples, P bytes of a frame):

    gather_stacked_raw_u8/_f32  mcg_rollout_img_gather_stacked alone            at most k B P read; k B P / 4 k B P written
    gather_wide_raw_u8/_f32     mcg_rollout_img_gather on the wide buffer       k B P read; k B P / 4 k B P written
    torch_stacked_u8/_f32       randperm, index arithmetic, masks and gathers on the single-frame rows, one index op per field
    carry_stacked_raw           mcg_rollout_img_carry_stacked                   k N P read, k N P written
    carry_wide_raw              mcg_rollout_img_carry on the wide buffer        k N P read, k N P written
    add_single_raw              mcg_rollout_img_add, the stack's newest frame   2 N P
    add_wide_raw                mcg_rollout_img_add, the whole stack            2 k N P

The PyTorch formulation lives in this tool only: it is what a user writes without mcg_rollout_img_gather_stacked.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402
from mycobotgym_amd import _abi  # noqa: E402

HBM_SPEC_GBPS = 8000.0          # MI355X: HBM3E peak
HBM_COPY_GBPS = 6290.0          # and what a float4 copy kernel reaches of it
ENV_ID = "MyCobotReach-Dense-joint-v1"
FIELDS = ("value", "advantage", "returns")


class TorchStackedRollout:
    """The stacked rule on the device buffer's own rows, from stock PyTorch ops: history and data as one tensor each."""

    def __init__(self, buf):
        k, g = buf.frame_stack, buf._guard
        self.buf, self.k, self.T, self.n = buf, k, buf.n_steps, buf.num_envs
        end = lambda v: v.shape[0] - g
        self.rows = buf._alloc["pixels"][g:end(buf._alloc["pixels"])]                      # [k - 1 + T + 1, N, P]: row t is index t + k - 1
        self.flags = buf._alloc["episode_start"][g:end(buf._alloc["episode_start"])]      # [k - 1 + T, N]
        A = buf.act_dim
        self.actions = buf.records()[:, :, :4 * A].view(torch.float32)
        self.log_prob = buf.records()[:, :, 4 * A:4 * A + 4].view(torch.float32)[:, :, 0]

    def stacks(self, index, normalize):
        """-> stacks [B, k * P] of the transitions `index` (int64 [B], env * T + step)."""
        k = self.k
        e, t = index // self.T, index % self.T
        valid, slots = torch.ones_like(index, dtype=torch.bool), []
        for i in range(k):          # i = 0: the newest
            slots.append(torch.where(valid[:, None], self.rows[t + (k - 1) - i, e], 0))
            if i < k - 1:
                valid = valid & (self.flags[t + (k - 1) - i, e] == 0)
        obs = torch.cat(slots[::-1], dim=1)
        return obs.float() / 255 if normalize else obs

    def minibatch(self, B, normalize):
        index = torch.randperm(self.T * self.n, device=self.rows.device)[:B]
        e, t = index // self.T, index % self.T
        planes = self.buf.planes()
        return (self.stacks(index, normalize), self.actions[t, e], self.log_prob[t, e]) + tuple(planes[name][t, e] for name in FIELDS)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--stack", type=int, default=4)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds of each pair of kernels")
    ap.add_argument("--machine", default=None, help="a name for the machine the numbers come from (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rollout_img_stacked_bench needs the GPU: a timing taken anywhere else says nothing")
    k, T, B = args.stack, args.steps, args.batch
    fs = mg.FrameStack(mg.make(ENV_ID, num_envs=args.envs, image_size=args.size, seed=1), k)
    n, A, dev, Cc, S = fs.num_envs, fs.action_dim, fs.device, fs.frame_channels, fs.image_size
    single = mg.ImageRolloutBuffer(fs, n_steps=T, seed=0, frame_stack=k)
    wide = mg.ImageRolloutBuffer(fs, n_steps=T, seed=0)                      # the wrapper's stacks as k * C channels
    P, M = single.picture_bytes, T * n
    if P != single.row_bytes:
        sys.exit("the PyTorch formulation here reads unpadded rows: choose a picture whose bytes are a multiple of 16")
    B = min(B, M)
    nbytes = lambda b: sum(v.numel() * v.element_size() for v in b._alloc.values())
    pixel_bytes = {"single": single._alloc["pixels"].numel(), "wide": wide._alloc["pixels"].numel()}
    stack, _ = fs.reset(seed=1)
    single.start(stack); wide.start(stack)
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    kept, ends = [], 0
    for rollout in range(2):
        for t in range(T):
            a = (torch.rand(n, A, generator=g) * 2 - 1).to(dev)
            v, lp, fv = (torch.randn(n, generator=g).to(dev) for _ in range(3))
            out = fs.step(a)
            single.add(a, v, lp, *out, final_values=fv); wide.add(a, v, lp, *out, final_values=fv)
            ends += int((out[2] | out[3]).sum())
            kept = (kept + [(a, v, lp, fv, out)])[-8:]
        lv = torch.randn(n, generator=g).to(dev)
        single.finish(lv); wide.finish(lv)
        if rollout == 0:
            single.reset(); wide.reset()
        print(f"rollout {rollout + 1} of 2 filled, {ends} episode ends so far", flush=True)
    res = {"env_id": ENV_ID, "envs": n, "size": S, "frame_channels": Cc, "frame_stack": k, "n_steps": T, "batch": B, "frame_bytes": P,
           "pixel_bytes": pixel_bytes, "buffer_bytes": {"single": nbytes(single), "wide": nbytes(wide)}, "episode_ends_in_fill": ends,
           "device": torch.cuda.get_device_name(0), "machine": args.machine, "hbm_spec_gbps": HBM_SPEC_GBPS, "hbm_copy_gbps": HBM_COPY_GBPS,
           "cases": {}}
    print(json.dumps({"pixel_bytes": pixel_bytes, "buffer_bytes": res["buffer_bytes"]}), flush=True)
    # ---- the same epoch from both buffers and one minibatch from PyTorch ops, before any timing
    tb = TorchStackedRollout(single)
    same, firsts = {}, list(range(0, M, B))
    for normalize in (False, True):
        tag = "f32" if normalize else "u8"
        ok, depth_hist = True, None
        for first in firsts:
            count = min(B, M - first)
            x, y = single.gather(0, first, count, normalize=normalize), wide.gather(0, first, count, normalize=normalize)
            ok = ok and all(torch.equal(p, q) for p, q in zip(x, y))
            if first == 0:
                want = tb.stacks(x.index.long(), False)
                if normalize:          # the correctly rounded quotient, as numpy divides
                    want = torch.from_numpy(want.cpu().numpy().astype(np.float32) / np.float32(255)).to(dev)
                e, t = x.index.long() // T, x.index.long() % T
                planes = single.planes()
                same["torch_" + tag] = bool(torch.equal(x.observations.reshape(count, -1), want) and torch.equal(x.actions, tb.actions[t, e])
                                            and torch.equal(x.old_log_prob, tb.log_prob[t, e]) and torch.equal(x.advantages, planes["advantage"][t, e]))
                if not normalize:
                    slots = x.observations.reshape(count, k, -1).max(dim=2).values == 0          # an all-zero slot: before the episode
                    depth_hist = [int((slots.sum(dim=1) == z).sum()) for z in range(k)]
                    res["first_minibatch"] = {"samples_by_empty_slots": depth_hist, "steps_below_k_minus_1": int((t < k - 1).sum())}
        same["wide_" + tag] = bool(ok)
    res["equal"] = same
    print(json.dumps({"equal": same, "first_minibatch": res["first_minibatch"]}), flush=True)

    def report(name, r, nb):
        r["bytes"] = nb
        r["gbps"] = nb / (r["median_ms"] * 1e-3) / 1e9
        r["of_hbm_spec"], r["of_hbm_copy"] = r["gbps"] / HBM_SPEC_GBPS, r["gbps"] / HBM_COPY_GBPS
        res["cases"][name] = r
        print(json.dumps({name: r}), flush=True)

    lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # ---- the gather: the two kernels alone in alternating rounds, then the PyTorch formulation
    small = {"action": torch.empty(B, A, device=dev), "old_value": torch.empty(B, device=dev), "old_log_prob": torch.empty(B, device=dev),
             "advantage": torch.empty(B, device=dev), "returns": torch.empty(B, device=dev), "index": torch.empty(B, dtype=torch.int32, device=dev)}
    full = [f for f in firsts if M - f >= B]
    for normalize in (False, True):
        tag = "f32" if normalize else "u8"
        w = 4 if normalize else 1
        pix = torch.empty(B, k * P, dtype=torch.float32 if normalize else torch.uint8, device=dev)
        out = _abi.McgRolloutImgBatch(**{"pix_f32" if normalize else "pix": pix.data_ptr()}, **{k_: v.data_ptr() for k_, v in small.items()})
        cyc = itertools.cycle(full)

        def stacked_raw():
            _abi.check(lib.mcg_rollout_img_gather_stacked(C.byref(single._cbuf), k, 0, 1, next(cyc), B, C.byref(out), stream),
                       "mcg_rollout_img_gather_stacked")

        def wide_raw():
            _abi.check(lib.mcg_rollout_img_gather(C.byref(wide._cbuf), 0, 1, next(cyc), B, C.byref(out), stream), "mcg_rollout_img_gather")
        for rnd in range(args.rounds):
            suffix = f"{tag}_round{rnd}"
            report("gather_stacked_raw_" + suffix, timed(stacked_raw, warmup=5, reps=args.reps, inner=300), (k + k * w) * B * P)
            report("gather_wide_raw_" + suffix, timed(wide_raw, warmup=5, reps=args.reps, inner=300), (k + k * w) * B * P)
        report("torch_stacked_" + tag, timed(lambda: tb.minibatch(B, normalize), warmup=3, reps=args.reps, inner=30), (k + k * w) * B * P)
    # ---- the carry at pos = n_steps (it leaves what it found: the rows it reads are not the rows it writes there)
    def carry_stacked_raw():
        _abi.check(lib.mcg_rollout_img_carry_stacked(C.byref(single._cbuf), T, k, stream), "mcg_rollout_img_carry_stacked")

    def carry_wide_raw():
        _abi.check(lib.mcg_rollout_img_carry(C.byref(wide._cbuf), T, stream), "mcg_rollout_img_carry")
    if T >= 2 * k:
        for rnd in range(args.rounds):
            report(f"carry_stacked_raw_round{rnd}", timed(carry_stacked_raw, warmup=5, reps=args.reps, inner=500), 2 * k * n * P)
            report(f"carry_wide_raw_round{rnd}", timed(carry_wide_raw, warmup=5, reps=args.reps, inner=500), 2 * k * n * P)
    # ---- insertion, last: it overwrites the rollout
    raw = [(a, v, lp, fv, o[0], o[1].double(), o[2], o[3]) for a, v, lp, fv, o in kept]
    rcycle, pos = itertools.cycle(raw), itertools.cycle(range(T))

    def add_single_raw():
        a, v, lp, fv, o, rew, term, trunc = next(rcycle)
        o = o[:, (k - 1) * Cc:]
        _abi.check(lib.mcg_rollout_img_add(C.byref(single._cbuf), next(pos), p(a), p(v), p(lp), p(fv), p(o), o.stride(0), o.stride(1), p(rew),
                                           p(term), p(trunc), stream), "mcg_rollout_img_add")

    def add_wide_raw():
        a, v, lp, fv, o, rew, term, trunc = next(rcycle)
        _abi.check(lib.mcg_rollout_img_add(C.byref(wide._cbuf), next(pos), p(a), p(v), p(lp), p(fv), p(o), o.stride(0), o.stride(1), p(rew),
                                           p(term), p(trunc), stream), "mcg_rollout_img_add")
    for rnd in range(args.rounds):
        report(f"add_single_raw_round{rnd}", timed(add_single_raw, warmup=5, reps=args.reps, inner=1000), 2 * n * P)
        report(f"add_wide_raw_round{rnd}", timed(add_wide_raw, warmup=5, reps=args.reps, inner=500), 2 * k * n * P)
    c = res["cases"]
    best = lambda prefix: min(r["median_ms"] for name, r in c.items() if name.startswith(prefix))
    res["stacked_time_over_wide_time"] = {f"{tag}_round{rnd}": c[f"gather_stacked_raw_{tag}_round{rnd}"]["median_ms"] / c[f"gather_wide_raw_{tag}_round{rnd}"]["median_ms"]
                                          for tag in ("u8", "f32") for rnd in range(args.rounds)}
    res["torch_time_over_stacked_time"] = {tag: c["torch_stacked_" + tag]["median_ms"] / best(f"gather_stacked_raw_{tag}_") for tag in ("u8", "f32")}
    res["add_wide_time_over_add_single_time"] = best("add_wide_raw_") / best("add_single_raw_")
    if T >= 2 * k:
        res["carry_stacked_time_over_carry_wide_time"] = best("carry_stacked_raw_") / best("carry_wide_raw_")
    res["wide_pixel_bytes_over_single"] = pixel_bytes["wide"] / pixel_bytes["single"]
    print(json.dumps({k_: v for k_, v in res.items() if k_.endswith("_time") or k_.endswith("_single")}), flush=True)
    fs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    bad = [k_ for k_, v in same.items() if not v]
    sys.exit("a comparison failed: " + ", ".join(bad) if bad else 0)


if __name__ == "__main__":
    main()
