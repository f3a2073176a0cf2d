#!/usr/bin/env python3
"""Device-event timing of the picture replay buffer: insertion and sampling (uint8 and normalised), the same rule written with stock
PyTorch ops, and the picture rollout buffer's insertion and gather as yardsticks, all in one process; and a check of the byte offsets
above 4 GiB.

    python tools/replay_img_bench.py [--envs 8192] [--size 64] [--capacity 1000] [--batch 4096] [--reps 20] [--out profiles/replay_img/replay_img_bench.json]

Setup: --envs environments of MyCobotReach-Dense-joint-v1 (one camera, --size x --size, the registered time limit of 50) driven by a
seeded random policy for capacity + 8 steps into an ImageReplayBuffer and into the PyTorch formulation, so the ring has wrapped and
holds real time-limit ends; the last 8 step outputs are kept and cycled through by the insertion paths, which run last.  Every path:
warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch stream; reported: median and
min / max of the per-call time, and the algorithmic bytes over the median (N environments, B samples, P bytes of a picture):

    sample_raw_u8 / _f32    mcg_replay_img_sample alone into preallocated outputs            4 B P / 10 B P bytes
    sample_u8 / _f32        ImageReplayBuffer.sample(B, check=False): Python and the output allocations included
    torch_sample_u8 / _f32  randint, index ops on [R, N, P], a `where` for the final pictures (and .float() / 255)
    gather_raw_u8 / _f32    mcg_rollout_img_gather alone (a 32-step ImageRolloutBuffer of the same pictures)   2 B P / 5 B P bytes
    add_raw                 mcg_replay_img_add alone on the kept outputs                    2 N P + 2 P per time-limit end
    add                     ImageReplayBuffer.add(...): the public call, Python included
    torch_add               row assignments and a `where` for the final pictures
    rollout_add_raw         mcg_rollout_img_add alone on the same kept outputs              2 N P bytes

The PyTorch formulation lives in this tool only: it is what a user writes without the mcg_replay_img_* calls.  It draws with
torch.randint and does not reject transitions that lost their next picture.

Large offsets (`big_offsets`; needs pixels beyond 4 GiB, as the default shape's 33.6 GB are): the top row of the ring is written by the
fill; batches are drawn until one holds a transition of the top row (its successor is row 0), and the whole batch -- picture, successor
from the ring or the final pictures, action, reward, done -- is compared with stock int64 indexing on the device, the top-row
transition with a host copy of its rows as well.
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


class TorchImageReplay:
    """The same ring from stock PyTorch ops: uint8 [R, N, P] pixels, [F, N, P] final pictures with their stamps, one tensor per field."""

    def __init__(self, n, P, A, K, Tm, dev):
        self.n, self.P, self.K, self.R, self.Tm, self.F, self.written = n, P, K, K + 1, Tm, -(-K // Tm) + 1, 0
        self.pixels = torch.zeros(self.R, n, P, dtype=torch.uint8, device=dev)
        self.finals = torch.zeros(self.F, n, P, dtype=torch.uint8, device=dev)
        self.final_time = torch.full((self.F, n), -1, dtype=torch.int64, device=dev)
        self.act = torch.zeros(self.R, n, A, device=dev)
        self.rew = torch.zeros(self.R, n, device=dev)
        self.flags = torch.zeros(self.R, n, dtype=torch.int32, device=dev)

    def add(self, a, img, r, term, trunc, info):
        t, n = self.written, self.n
        row, frow = t % self.R, (t // self.Tm) % self.F
        timeout = trunc & ~term
        self.pixels[(t + 1) % self.R] = img.reshape(n, -1)
        self.act[row] = a; self.rew[row] = r.float(); self.flags[row] = term.int() + 2 * timeout.int()
        self.finals[frow] = torch.where(timeout[:, None], info["final_observation"].reshape(n, -1), self.finals[frow])
        self.final_time[frow] = torch.where(timeout, t, self.final_time[frow])
        self.written += 1

    def successor(self, rows, e, a):
        """-> (next picture, done, from the final pictures) of the transitions at time `a` (int64 [B]) in (rows, e), by int64 indexing."""
        fl = self.flags[rows, e]
        frow = (a // self.Tm) % self.F
        use = ((fl & 2) != 0) & (self.final_time[frow, e] == a)
        nxt = torch.where(use[:, None], self.finals[frow, e], self.pixels[(rows + 1) % self.R, e])
        done = ((fl & 1) != 0) | (((fl & 2) != 0) & ~use)
        return nxt, done.float(), use

    def sample(self, B, normalize):
        W, dev = min(self.written, self.K), self.pixels.device
        a = self.written - W + torch.randint(0, W, (B,), device=dev)
        e = torch.randint(0, self.n, (B,), device=dev)
        rows = a % self.R
        obs = self.pixels[rows, e]
        nxt, done, _ = self.successor(rows, e, a)
        if normalize:
            obs, nxt = obs.float() / 255, nxt.float() / 255
        return obs, self.act[rows, e], nxt, done, self.rew[rows, e]


def big_offsets(buf, tb, B):
    """A batch holding a transition of the ring's top row against stock int64 indexing (and a host copy) -> a dict of what was compared."""
    px, R, n, P = buf._t["pixels"], buf.capacity + 1, buf.num_envs, buf.row_bytes
    res = {"pixels_bytes": int(px.numel()), "top_row_first_byte": (R - 1) * n * P, "n_written": buf.n_written}
    W = min(buf.n_written, buf.capacity)
    time_of_row = torch.full((R,), -1, dtype=torch.int64, device=px.device)
    times = torch.arange(buf.n_written - W, buf.n_written, device=px.device)
    time_of_row[times % R] = times
    for tries in range(1, 21):
        raw = buf.sample(B, normalize=False, check=False)
        top = (raw.index[:, 0] == R - 1).nonzero()
        if len(top):
            break
    else:
        return dict(res, found=False)
    buf.n_sampled -= 1
    norm = buf.sample(B, check=False)
    rows, e = raw.index[:, 0].long(), raw.index[:, 1].long()
    a = time_of_row[rows]
    want_next, want_done, use = tb.successor(rows, e, a)
    shape = raw.observations.shape
    k = int(top[0, 0])
    host_pic = px[R - 1, int(e[k])].cpu().numpy()[:buf.picture_bytes]
    host_next = (buf._t["finals"][int((a[k] // buf.max_episode_steps) % buf.final_rows), int(e[k])] if bool(use[k]) else px[0, int(e[k])]).cpu().numpy()
    res.update(found=True, batches_drawn=tries, sample=k, top_row_samples=int(len(top)), from_finals=int(use.sum()),
               highest_byte_read=int(((rows * n + e) * P + P - 1).max()),
               pix_equal=bool(torch.equal(raw.observations, px[rows, e][:, :buf.picture_bytes].reshape(shape))),
               next_pix_equal=bool(torch.equal(raw.next_observations, want_next[:, :buf.picture_bytes].reshape(shape))),
               source_equal=bool(torch.equal(raw.index[:, 2].bool(), use)),
               done_equal=bool(torch.equal(raw.dones[:, 0], want_done)),
               action_equal=bool(torch.equal(raw.actions, tb.act[rows, e])), reward_equal=bool(torch.equal(raw.rewards[:, 0], tb.rew[rows, e])),
               host_copy_equal=bool((raw.observations[k].cpu().numpy().reshape(-1) == host_pic).all()
                                    and (raw.next_observations[k].cpu().numpy().reshape(-1) == host_next[:buf.picture_bytes]).all()))
    q = lambda x: x.cpu().numpy().astype(np.float32) / np.float32(255)
    res["f32_equal"] = bool((norm.observations.cpu().numpy().view(np.uint32) == q(raw.observations).view(np.uint32)).all()
                            and (norm.next_observations.cpu().numpy().view(np.uint32) == q(raw.next_observations).view(np.uint32)).all())
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--capacity", type=int, default=1000)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rollout-steps", type=int, default=32)
    ap.add_argument("--machine", default=None, help="a name for the machine the numbers come from (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("replay_img_bench needs the GPU: a timing taken anywhere else says nothing")
    envs = mg.make(ENV_ID, num_envs=args.envs, image_size=args.size, seed=1)
    img, _ = envs.reset(seed=1)
    n, A, K, dev, B, Tm = envs.num_envs, envs.action_dim, args.capacity, envs.device, args.batch, envs.max_episode_steps
    buf = mg.ImageReplayBuffer(envs, capacity=K, seed=0)
    P = buf.picture_bytes
    if P != buf.row_bytes:
        sys.exit("the PyTorch formulation here stores unpadded rows: choose a picture whose bytes are a multiple of 16")
    tb = TorchImageReplay(n, buf.row_bytes, A, K, Tm, dev)
    buf.start(img)
    tb.pixels[0] = buf._t["pixels"][0]
    g = torch.Generator(device="cpu"); g.manual_seed(0)
    kept, timeouts = [], 0
    for t in range(K + 8):
        a = (torch.rand(n, A, generator=g) * 2 - 1).to(dev)
        out = envs.step(a)
        buf.add(a, *out)
        tb.add(a, *out)
        timeouts += int((out[3] & ~out[2]).sum())
        kept = (kept + [(a, out)])[-8:]
        if (t + 1) % 100 == 0:
            print(f"filled {t + 1} of {K + 8} steps, {timeouts} time-limit ends", flush=True)
    same = {k: bool(torch.equal(getattr(tb, k), buf._t[k])) for k in ("pixels", "finals", "final_time")}
    print(json.dumps({"fill_equal": same}), flush=True)
    res = {"env_id": ENV_ID, "envs": n, "size": args.size, "channels": buf.channels, "capacity": K, "max_episode_steps": Tm, "batch": B,
           "picture_bytes": P, "buffer_bytes": buf.nbytes, "time_limit_ends_in_fill": timeouts, "fill_equal": same,
           "device": torch.cuda.get_device_name(0), "machine": args.machine, "hbm_spec_gbps": HBM_SPEC_GBPS, "hbm_copy_gbps": HBM_COPY_GBPS,
           "cases": {}}

    def report(name, r, nbytes=None):
        if nbytes is not None:
            r["bytes"] = nbytes
            r["gbps"] = nbytes / (r["median_ms"] * 1e-3) / 1e9
            r["of_hbm_spec"], r["of_hbm_copy"] = r["gbps"] / HBM_SPEC_GBPS, r["gbps"] / HBM_COPY_GBPS
        res["cases"][name] = r
        print(json.dumps({name: r}), flush=True)

    if buf._t["pixels"].numel() > 2 ** 32 + n * buf.row_bytes:
        res["big_offsets"] = big_offsets(buf, tb, B)
        print(json.dumps({"big_offsets": res["big_offsets"]}), flush=True)
    lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    p = lambda t: C.c_void_p(t.data_ptr())
    # ---- sampling: the kernel alone, the public call, the PyTorch formulation
    small = {"action": torch.empty(B, A, device=dev), "reward": torch.empty(B, device=dev), "done": torch.empty(B, device=dev),
             "index": torch.empty(B, 3, dtype=torch.int32, device=dev)}
    for normalize, factor in ((False, 4), (True, 10)):
        tag = "f32" if normalize else "u8"
        pix, nxt = (torch.empty(B, P, dtype=torch.float32 if normalize else torch.uint8, device=dev) for _ in range(2))
        out = _abi.McgReplayImgBatch(**{"pix_f32" if normalize else "pix": pix.data_ptr(), "next_pix_f32" if normalize else "next_pix": nxt.data_ptr()},
                                     **{k: v.data_ptr() for k, v in small.items()})
        state = {"call": 0}

        def sample_raw():
            _abi.check(lib.mcg_replay_img_sample(C.byref(buf._cbuf), buf.n_written, 0, state["call"], B, C.byref(out), stream), "mcg_replay_img_sample")
            state["call"] += 1
        report("sample_raw_" + tag, timed(sample_raw, warmup=5, reps=args.reps, inner=1000), factor * B * P)
        report("sample_" + tag, timed(lambda: buf.sample(B, normalize=normalize, check=False), warmup=5, reps=args.reps, inner=500), factor * B * P)
        report("torch_sample_" + tag, timed(lambda: tb.sample(B, normalize), warmup=5, reps=args.reps, inner=100), factor * B * P)
    res["give_ups_and_lost_finals"] = buf.counters()
    # ---- the rollout buffer's gather and insertion on the same pictures: the kernels this one was derived from
    T = args.rollout_steps
    rb = mg.ImageRolloutBuffer(envs, n_steps=T, seed=0)
    for t in range(T + 1):
        rb._t["pixels"][t] = buf._t["pixels"][t]
    M = T * n
    for normalize, factor in ((False, 2), (True, 5)):
        pix = torch.empty(B, P, dtype=torch.float32 if normalize else torch.uint8, device=dev)
        out = _abi.McgRolloutImgBatch(**{"pix_f32" if normalize else "pix": pix.data_ptr()})
        state = {"k": 0}

        def gather_raw():
            _abi.check(lib.mcg_rollout_img_gather(C.byref(rb._cbuf), 0, 0, state["k"] * B, B, C.byref(out), stream), "mcg_rollout_img_gather")
            state["k"] = (state["k"] + 1) % (M // B)
        report("gather_raw_f32" if normalize else "gather_raw_u8", timed(gather_raw, warmup=5, reps=args.reps, inner=1000), factor * B * P)
    # ---- insertion, last: cycling the kept outputs puts time-limit ends at times the engine would not
    ends = sum(int((o[3] & ~o[2]).sum()) for _, o in kept) / len(kept)
    add_bytes = int(2 * n * P + 2 * P * ends)
    raw = [(a, o[0], o[1].double(), o[2], o[3], o[4]["final_observation"]) for a, o in kept]
    rcycle, cycle = itertools.cycle(raw), itertools.cycle(kept)
    state = {"n": buf.n_written}

    def add_raw():
        a, o, rew, term, trunc, fin = next(rcycle)
        _abi.check(lib.mcg_replay_img_add(C.byref(buf._cbuf), state["n"], p(a), p(o), o.stride(0), o.stride(1), p(fin), fin.stride(0), fin.stride(1),
                                          p(rew), p(term), p(trunc), stream), "mcg_replay_img_add")
        state["n"] += 1
    report("add_raw", timed(add_raw, warmup=5, reps=args.reps, inner=2000), add_bytes)

    def add():
        a, out = next(cycle)
        buf.add(a, *out)
    report("add", timed(add, warmup=5, reps=args.reps, inner=500), add_bytes)

    def torch_add():
        a, out = next(cycle)
        tb.add(a, *out)
    report("torch_add", timed(torch_add, warmup=5, reps=args.reps, inner=200), add_bytes)
    z = torch.zeros(n, device=dev)
    rstate = {"pos": 0}

    def rollout_add_raw():
        a, o, rew, term, trunc, _ = next(rcycle)
        _abi.check(lib.mcg_rollout_img_add(C.byref(rb._cbuf), rstate["pos"], p(a), p(z), p(z), None, p(o), o.stride(0), o.stride(1), p(rew), p(term),
                                           p(trunc), stream), "mcg_rollout_img_add")
        rstate["pos"] = (rstate["pos"] + 1) % T
    report("rollout_add_raw", timed(rollout_add_raw, warmup=5, reps=args.reps, inner=2000), 2 * n * P)
    c = res["cases"]
    res["ratio_to_torch"] = {k: c["torch_" + k]["median_ms"] / c[k]["median_ms"] for k in ("add", "sample_u8", "sample_f32")}
    res["sample_rate_over_gather_rate"] = {t: c["sample_raw_" + t]["gbps"] / c["gather_raw_" + t]["gbps"] for t in ("u8", "f32")}
    res["add_rate_over_rollout_add_rate"] = c["add_raw"]["gbps"] / c["rollout_add_raw"]["gbps"]
    print(json.dumps({k: res[k] for k in ("ratio_to_torch", "sample_rate_over_gather_rate", "add_rate_over_rollout_add_rate")}), flush=True)
    envs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    bad = [k for k, v in res.get("big_offsets", {}).items() if (k.endswith("_equal") or k == "found") and not v] + [k for k, v in same.items() if not v]
    sys.exit("a comparison failed: " + ", ".join(bad) if bad else 0)


if __name__ == "__main__":
    main()
