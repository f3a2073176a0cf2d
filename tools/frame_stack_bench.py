#!/usr/bin/env python3
"""Device-event timing of frame stacking for the pictures: the act-time push, insertion into the single-frame ring against insertion
of whole stacks into a ring k times as wide, and stacked sampling against two yardsticks that write the same output bytes -- the
existing sampling kernel on the wide ring, and the stacked rule written with stock PyTorch ops -- all in one process.

    python tools/frame_stack_bench.py [--envs 8192] [--size 64] [--stack 4] [--capacity 250] [--batch 4096] [--reps 20] [--out profiles/frame_stack/frame_stack_bench.json]

Setup: a FrameStack of --stack frames around --envs environments of MyCobotReach-Dense-joint-v1 (one camera, --size x --size, the
registered time limit of 50) driven by a seeded random policy for capacity + 8 steps into ImageReplayBuffer(fs, capacity) (single
frames, capacity + k rows) and into an ImageReplayBuffer of k * C channels fed the same stacks (capacity + 1 rows, k times as wide), so
both rings have wrapped and hold real time-limit ends.  The two buffers share seed and window, so they make the same draws: before any
timing, a batch of each is compared, bit for bit, and with the PyTorch formulation on the same draws.  The last 8 step outputs are kept
and cycled through by the push and insertion paths, which run last.  Every path: warm-up calls, then `reps` windows of `inner`
back-to-back calls between two events on the launch stream; the two sampling kernels are timed in alternating rounds.  Reported:
median and min / max of the per-call time, and the algorithmic bytes over the median (N environments, B samples, P bytes of a frame):

    push_raw                    mcg_frame_stack_push alone                                    (k + 1) N P read, 2 k N P written
    add_stacked_raw             mcg_replay_img_add, the stack's newest frame into the single-frame ring      2 N P (+ 2 P per time-limit end)
    add_wide_raw                mcg_replay_img_add, the whole stack into the wide ring                       2 k N P (+ 2 k P per end)
    sample_stacked_raw_u8/_f32  mcg_replay_img_sample_stacked alone     at most (k + 1) B P read; 2 k B P / 8 k B P written
    sample_wide_raw_u8/_f32     mcg_replay_img_sample on the wide ring  2 k B P read; 2 k B P / 8 k B P written
    torch_stacked_u8/_f32       index arithmetic, masks and gathers on the single-frame ring [R, N, P]

The PyTorch formulation lives in this tool only: it is what a user writes without mcg_replay_img_sample_stacked.  It draws with
torch.randint and does not reject transitions that lost their next picture.
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


class TorchStackedReplay:
    """The stacked rule on the device buffer's own single-frame ring, from stock PyTorch ops: the flags as one int32 tensor [R, N]."""

    def __init__(self, buf, k):
        self.buf, self.k, self.K, self.R, self.n, self.Tm = buf, k, buf.capacity, buf.rows, buf.num_envs, buf.max_episode_steps
        self.pixels, self.finals, self.final_time, self.F = buf._t["pixels"], buf._t["finals"], buf._t["final_time"], buf.final_rows
        A = buf.act_dim
        self.flags = buf.records()[:, :, 4 * (A + 1):4 * (A + 2)].contiguous().view(torch.int32)[:, :, 0]

    def stacks(self, a, e, normalize):
        """-> (stack, next stack) [B, k * P] of the transitions at times `a` (int64 [B]) of environments `e`."""
        k, R, P = self.k, self.R, self.pixels.shape[2]
        valid, slots = torch.ones_like(a, dtype=torch.bool), []
        for i in range(k):          # i = 0: the newest
            slots.append(torch.where(valid[:, None], self.pixels[(a - i) % R, e], 0))
            valid = valid & ~((a - i == 0) | (self.flags[(a - i - 1) % R, e] != 0))
        obs = torch.cat(slots[::-1], dim=1)
        rows, frow = a % R, (a // self.Tm) % self.F
        fl = self.flags[rows, e]
        use = ((fl & 2) != 0) & (self.final_time[frow, e] == a)
        newest = torch.where(use[:, None], self.finals[frow, e], self.pixels[(rows + 1) % R, e])
        keep = ((fl & 3) == 0) | use
        nxt = torch.cat([torch.where(keep[:, None], obs[:, P:], 0), newest], dim=1)
        if normalize:
            obs, nxt = obs.float() / 255, nxt.float() / 255
        return obs, nxt

    def sample(self, B, normalize):
        n_written, dev = self.buf.n_written, self.pixels.device
        W = min(n_written, self.K)
        a = n_written - W + torch.randint(0, W, (B,), device=dev)
        e = torch.randint(0, self.n, (B,), device=dev)
        return self.stacks(a, e, normalize)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--stack", type=int, default=4)
    ap.add_argument("--capacity", type=int, default=250)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=2, help="alternating rounds of the two sampling kernels")
    ap.add_argument("--machine", default=None, help="a name for the machine the numbers come from (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("frame_stack_bench needs the GPU: a timing taken anywhere else says nothing")
    k, K, B = args.stack, args.capacity, args.batch
    fs = mg.FrameStack(mg.make(ENV_ID, num_envs=args.envs, image_size=args.size, seed=1), k)
    n, A, dev, Tm, Cc, S = fs.num_envs, fs.action_dim, fs.device, fs.max_episode_steps, fs.frame_channels, fs.image_size
    single = mg.ImageReplayBuffer(fs, capacity=K, seed=0)
    wide = mg.ImageReplayBuffer(capacity=K, seed=0, num_envs=n, channels=k * Cc, image_size=S, act_dim=A, max_episode_steps=Tm, device=dev)
    P = single.picture_bytes
    if P != single.row_bytes:
        sys.exit("the PyTorch formulation here reads unpadded rows: choose a picture whose bytes are a multiple of 16")
    stack, _ = fs.reset(seed=1)
    single.start(stack); wide.start(stack)
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    kept, timeouts = [], 0
    for t in range(K + 8):
        a = (torch.rand(n, A, generator=g) * 2 - 1).to(dev)
        out = fs.step(a)
        single.add(a, *out); wide.add(a, *out)
        timeouts += int((out[3] & ~out[2]).sum())
        kept = (kept + [(a, out)])[-8:]
        if (t + 1) % 50 == 0:
            print(f"filled {t + 1} of {K + 8} steps, {timeouts} time-limit ends", flush=True)
    res = {"env_id": ENV_ID, "envs": n, "size": S, "frame_channels": Cc, "frame_stack": k, "capacity": K, "max_episode_steps": Tm, "batch": B,
           "frame_bytes": P, "single_frame_ring_bytes": single.nbytes, "wide_ring_bytes": wide.nbytes, "time_limit_ends_in_fill": timeouts,
           "device": torch.cuda.get_device_name(0), "machine": args.machine, "hbm_spec_gbps": HBM_SPEC_GBPS, "hbm_copy_gbps": HBM_COPY_GBPS,
           "cases": {}}
    print(json.dumps({"single_frame_ring_bytes": single.nbytes, "wide_ring_bytes": wide.nbytes}), flush=True)
    # ---- the same draws three ways, before any timing
    tb = TorchStackedReplay(single, k)
    same = {}
    for normalize in (False, True):
        x, y = single.sample(B, normalize=normalize, check=False), wide.sample(B, normalize=normalize, check=False)
        W = min(single.n_written, K)
        time_of_row = torch.full((single.rows,), -1, dtype=torch.int64, device=dev)
        times = torch.arange(single.n_written - W, single.n_written, device=dev)
        time_of_row[times % single.rows] = times
        at, e = time_of_row[x.index[:, 0].long()], x.index[:, 1].long()
        obs, nxt = tb.stacks(at, e, False)
        if normalize:          # the correctly rounded quotient, as numpy divides
            obs, nxt = (torch.from_numpy(v.cpu().numpy().astype(np.float32) / np.float32(255)).to(dev) for v in (obs, nxt))
        tag = "f32" if normalize else "u8"
        same["wide_" + tag] = bool(torch.equal(x.observations, y.observations) and torch.equal(x.next_observations, y.next_observations)
                                   and torch.equal(x.dones, y.dones) and torch.equal(x.actions, y.actions) and torch.equal(x.rewards, y.rewards)
                                   and torch.equal(x.index[:, 1:], y.index[:, 1:]) and torch.equal(at % (K + 1), y.index[:, 0].long()))
        same["torch_" + tag] = bool(torch.equal(x.observations.reshape(B, -1), obs) and torch.equal(x.next_observations.reshape(B, -1), nxt))
        if not normalize:
            res["sampled"] = {"from_finals": int((x.index[:, 2] == 1).sum()), "terminal": int(x.dones.sum()),
                              "empty_oldest_slot": int((x.observations[:, :Cc].reshape(B, -1).max(dim=1).values == 0).sum())}
    res["equal"] = same
    print(json.dumps({"equal": same, "sampled": res["sampled"]}), flush=True)

    def report(name, r, nbytes):
        r["bytes"] = nbytes
        r["gbps"] = nbytes / (r["median_ms"] * 1e-3) / 1e9
        r["of_hbm_spec"], r["of_hbm_copy"] = r["gbps"] / HBM_SPEC_GBPS, r["gbps"] / HBM_COPY_GBPS
        res["cases"][name] = r
        print(json.dumps({name: r}), flush=True)

    lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # ---- sampling: the two kernels alone in alternating rounds, then the PyTorch formulation
    small = {"action": torch.empty(B, A, device=dev), "reward": torch.empty(B, device=dev), "done": torch.empty(B, device=dev),
             "index": torch.empty(B, 3, dtype=torch.int32, device=dev)}
    for normalize in (False, True):
        tag = "f32" if normalize else "u8"
        w = 4 if normalize else 1
        pix, nxt = (torch.empty(B, k * P, dtype=torch.float32 if normalize else torch.uint8, device=dev) for _ in range(2))
        out = _abi.McgReplayImgBatch(**{"pix_f32" if normalize else "pix": pix.data_ptr(), "next_pix_f32" if normalize else "next_pix": nxt.data_ptr()},
                                     **{k_: v.data_ptr() for k_, v in small.items()})
        state = {"call": 0}

        def stacked_raw():
            _abi.check(lib.mcg_replay_img_sample_stacked(C.byref(single._cbuf), single.n_written, 0, state["call"], B, k, C.byref(out), stream),
                       "mcg_replay_img_sample_stacked")
            state["call"] += 1

        def wide_raw():
            _abi.check(lib.mcg_replay_img_sample(C.byref(wide._cbuf), wide.n_written, 0, state["call"], B, C.byref(out), stream), "mcg_replay_img_sample")
            state["call"] += 1
        for rnd in range(args.rounds):
            suffix = f"{tag}_round{rnd}"
            report("sample_stacked_raw_" + suffix, timed(stacked_raw, warmup=5, reps=args.reps, inner=300), ((k + 1) + 2 * k * w) * B * P)
            report("sample_wide_raw_" + suffix, timed(wide_raw, warmup=5, reps=args.reps, inner=300), (2 * k + 2 * k * w) * B * P)
        report("torch_stacked_" + tag, timed(lambda: tb.sample(B, normalize), warmup=3, reps=args.reps, inner=30), ((k + 1) + 2 * k * w) * B * P)
    res["give_ups_and_lost_finals"] = {"single": single.counters(), "wide": wide.counters()}
    # ---- the push and insertion, last: cycling the kept outputs puts time-limit ends at times the engine would not
    ends = sum(int((o[3] & ~o[2]).sum()) for _, o in kept) / len(kept)
    raw = [(a, o[0], o[1].double(), o[2], o[3], o[4]["final_observation"], (o[2] | o[3]).to(torch.uint8)) for a, o in kept]
    rcycle = itertools.cycle(raw)
    mine, final = torch.zeros_like(raw[0][1]), torch.zeros_like(raw[0][1])

    def push_raw():
        _, o, _, _, _, fin, done = next(rcycle)
        img, fin = o[:, (k - 1) * Cc:], fin[:, (k - 1) * Cc:]          # the step's picture and the finished episode's last
        _abi.check(lib.mcg_frame_stack_push(p(mine), p(final), n, Cc, S, k, p(img), img.stride(0), img.stride(1), p(fin), fin.stride(0), fin.stride(1),
                                            p(done), None, stream), "mcg_frame_stack_push")
    report("push_raw", timed(push_raw, warmup=5, reps=args.reps, inner=500), (3 * k + 1) * n * P)
    sstate, wstate = {"n": single.n_written}, {"n": wide.n_written}

    def add_stacked_raw():
        a, o, rew, term, trunc, fin, _ = next(rcycle)
        o, fin = o[:, (k - 1) * Cc:], fin[:, (k - 1) * Cc:]
        _abi.check(lib.mcg_replay_img_add(C.byref(single._cbuf), sstate["n"], p(a), p(o), o.stride(0), o.stride(1), p(fin), fin.stride(0), fin.stride(1),
                                          p(rew), p(term), p(trunc), stream), "mcg_replay_img_add")
        sstate["n"] += 1

    def add_wide_raw():
        a, o, rew, term, trunc, fin, _ = next(rcycle)
        _abi.check(lib.mcg_replay_img_add(C.byref(wide._cbuf), wstate["n"], p(a), p(o), o.stride(0), o.stride(1), p(fin), fin.stride(0), fin.stride(1),
                                          p(rew), p(term), p(trunc), stream), "mcg_replay_img_add")
        wstate["n"] += 1
    report("add_stacked_raw", timed(add_stacked_raw, warmup=5, reps=args.reps, inner=1000), int(2 * n * P + 2 * P * ends))
    report("add_wide_raw", timed(add_wide_raw, warmup=5, reps=args.reps, inner=500), int(2 * k * n * P + 2 * k * P * ends))
    c = res["cases"]
    res["wide_time_over_stacked_time"] = {name[len("sample_stacked_raw_"):]: c["sample_wide_raw_" + name[len("sample_stacked_raw_"):]]["median_ms"] / r["median_ms"]
                                          for name, r in c.items() if name.startswith("sample_stacked_raw_")}
    res["torch_time_over_stacked_time"] = {t: c["torch_stacked_" + t]["median_ms"] / min(c[f"sample_stacked_raw_{t}_round{r}"]["median_ms"] for r in range(args.rounds))
                                           for t in ("u8", "f32")}
    res["add_wide_time_over_add_stacked_time"] = c["add_wide_raw"]["median_ms"] / c["add_stacked_raw"]["median_ms"]
    print(json.dumps({k_: res[k_] for k_ in ("wide_time_over_stacked_time", "torch_time_over_stacked_time", "add_wide_time_over_add_stacked_time")}), flush=True)
    fs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    bad = [k_ for k_, v in same.items() if not v]
    sys.exit("a comparison failed: " + ", ".join(bad) if bad else 0)


if __name__ == "__main__":
    main()
