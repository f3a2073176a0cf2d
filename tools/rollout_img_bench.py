#!/usr/bin/env python3
"""Device-event timing of the picture rollout buffer: insertion, the advantage recursion, one epoch of minibatches (uint8 and
normalised), and the same written with stock PyTorch ops, all in one process; and a check of the byte offsets above 2 GiB.

    python tools/rollout_img_bench.py [--envs 8192] [--size 64] [--steps 32] [--batch 4096] [--reps 20] [--out profiles/rollout_img/rollout_img_bench.json]

Setup: --envs environments of MyCobotReach-Dense-joint-v1 (one camera, --size x --size) driven by a seeded random policy (random values
and log-probabilities) for --steps steps into an ImageRolloutBuffer; 8 further step outputs are kept and cycled through.  Every path:
warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch stream (`inner` chosen per path so
that a window is some 10 ms or more); reported: median and min / max of the per-call time, and for the three data-movement kernels the algorithmic bytes over the median (N environments, B samples
of a minibatch, P bytes of a picture):

    add          ImageRolloutBuffer.add(...) on kept step outputs (the step itself is not in the window): the public call, Python included
    add_raw      mcg_rollout_img_add alone, on the same kept outputs                                      2 N P bytes
    gae          ImageRolloutBuffer.finish(last_values): mcg_rollout_img_gae over the full buffer
    get_u8       one epoch, `for mb in buf.get(batch, normalize=False)`: launches and output allocations   2 B P bytes per minibatch
    get_f32      the same with normalize=True                                                             5 B P bytes per minibatch
    torch_add    a row assignment of the picture and one indexed store per field into preallocated [T, N, ...] tensors
    torch_gae    the backward loop of T steps in torch ops on [N] rows (tools/rollout_bench.py's)
    torch_get_u8 / torch_get_f32    torch.randperm(M), pixels.view(-1, P)[perm[k:k + B]] (and .float() / 255) and one index op per field
    gather_raw_u8 / gather_raw_f32  mcg_rollout_img_gather alone, one minibatch into a preallocated picture output: the kernel's own rate

The PyTorch formulations live in this tool only: they are what a user writes without the mcg_rollout_img_* calls.

Large offsets (--big-steps, default 64 and 96): a buffer of that many steps of 8192 x 4096-byte pictures, filled with random bytes.  The
insertion into the last row and the carry from it, and the minibatch that contains the transition at the highest byte offset, are
compared with stock indexing on the device and, for that one transition, with a host copy.  At 64 steps the gather's highest byte is
2^31 - 1 and the last row lies above 2 GiB; at 96 steps a third of the gathered rows do.
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
GAMMA, LAMBDA = 0.99, 0.95


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


class TorchImageRollout:
    """The buffer from stock PyTorch ops: uint8 [T + 1, N, P] pixels and one preallocated [T, N, ...] tensor per field."""

    def __init__(self, n, P, A, T, dev):
        f = dict(dtype=torch.float32, device=dev)
        self.n, self.T, self.P = n, T, P
        self.pixels = torch.zeros(T + 1, n, P, dtype=torch.uint8, device=dev)
        self.act = torch.zeros(T, n, A, **f)
        self.logp, self.val, self.rew, self.adv, self.ret, self.start = (torch.zeros(T, n, **f) for _ in range(6))
        self.last_start = torch.ones(n, **f)

    def add(self, pos, a, v, lp, fv, out):
        img, r, term, trunc, _ = out
        self.pixels[pos + 1] = img.reshape(self.n, -1)
        self.act[pos] = a; self.logp[pos] = lp; self.val[pos] = v; self.start[pos] = self.last_start
        self.rew[pos] = torch.where(trunc & ~term, r.float() + GAMMA * fv, r.float())
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

    def get(self, batch, normalize):
        M = self.T * self.n
        perm = torch.randperm(M, device=self.pixels.device)
        flat = [x.view(M, *x.shape[2:]) for x in (self.act, self.val, self.logp, self.adv, self.ret)]
        pix = self.pixels[:self.T].view(M, self.P)
        for first in range(0, M, batch):
            idx = perm[first:first + batch]
            obs = pix[idx]
            if normalize:
                obs = obs.float() / 255
            yield (obs,) + tuple(x[idx] for x in flat) + (idx,)


def big_offsets(steps, n, size, batch, dev):
    """The accesses above 2 GiB of a `steps`-step buffer against stock indexing and a host copy -> a dict of what was compared."""
    buf = mg.ImageRolloutBuffer(n_steps=steps, num_envs=n, channels=1, image_size=size, act_dim=7, seed=0, device=dev)
    P, T, M = buf.row_bytes, steps, steps * n
    px = buf._t["pixels"]
    gen = torch.Generator(device=dev); gen.manual_seed(steps)
    for t in range(T + 1):                                         # row by row: no temporary of the buffer's size
        px[t] = torch.randint(0, 256, (n, P), generator=gen, dtype=torch.uint8, device=dev)
    # the insertion into the last row and the carry from it
    last = torch.randint(0, 256, (n, 1, size, size), generator=gen, dtype=torch.uint8, device=dev)
    z = torch.zeros(n, device=dev)
    buf.pos = T - 1
    buf.add(torch.zeros(n, 7, device=dev), z, z, last, z.double(), z.bool(), z.bool())
    add_ok = bool(torch.equal(px[T], last.reshape(n, -1))) and bool(torch.equal(buf.pixels()[T], last))
    buf.finish(z)
    index = torch.empty(M, dtype=torch.int32, device=dev)          # the whole epoch's indices alone: where did the last transition go?
    out = _abi.McgRolloutImgBatch(index=index.data_ptr())
    _abi.check(_abi.load().mcg_rollout_img_gather(C.byref(buf._cbuf), buf.seed, 0, 0, M, C.byref(out),
                                                  C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), "mcg_rollout_img_gather")
    k = int((index == M - 1).nonzero()[0, 0])
    first = k // batch * batch
    count = min(batch, M - first)
    res = {"steps": steps, "pixels_bytes": int(px.numel()), "highest_gathered_byte": (M - 1) * P + P - 1, "last_row_first_byte": T * n * P,
           "sample": k, "add_into_last_row_equal": add_ok}
    mb = buf.gather(0, first, count, normalize=False)
    idx = mb.index.long()
    rows = (idx % T) * n + idx // T                                # int64 on the device
    want = px[:T].view(M, P)[rows].view(count, 1, size, size)
    assert int(mb.index[k - first]) == M - 1
    host = px[T - 1, n - 1].cpu().numpy().reshape(1, size, size)   # the transition at the highest offset, from a host copy of its row
    res["gather_u8_equal"] = bool(torch.equal(mb.observations, want)) and bool((mb.observations[k - first].cpu().numpy() == host).all())
    # normalised: against numpy's float32 quotient of the stock-indexed bytes, on the host.  (Stock `.float() / 255` on the device is
    # counted next to it: PyTorch divides a tensor by a Python scalar as a product with the scalar's reciprocal.)
    got = buf.gather(0, first, count, normalize=True).observations
    quotient = want.cpu().numpy().astype(np.float32) / np.float32(255)
    res["gather_f32_equal"] = bool((got.cpu().numpy().view(np.uint32) == quotient.view(np.uint32)).all())
    res["stock_device_quotient_differs_in"] = int((want.float() / 255 != got).sum())
    res["of_elements"] = int(got.numel())
    buf.reset()                                                    # the carry: row T (above 2 GiB) to row 0
    res["carry_equal"] = bool(torch.equal(px[0], last.reshape(n, -1)))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--size", type=int, default=64)
    ap.add_argument("--steps", type=int, default=32)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--big-steps", type=int, nargs="*", default=[64, 96])
    ap.add_argument("--machine", default=None, help="a name for the machine the numbers come from (recorded as given)")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("rollout_img_bench needs the GPU: a timing taken anywhere else says nothing")
    envs = mg.make(ENV_ID, num_envs=args.envs, image_size=args.size, seed=1)
    img, _ = envs.reset(seed=1)
    n, A, T, dev, B = envs.num_envs, envs.action_dim, args.steps, envs.device, args.batch
    buf = mg.ImageRolloutBuffer(envs, n_steps=T, gamma=GAMMA, gae_lambda=LAMBDA, seed=0)
    P, M = buf.picture_bytes, T * n
    buf.start(img)
    first_rollout = rollout(envs, T, 0, buf)
    lv = torch.randn(n, device=dev)
    buf.finish(lv)
    kept = rollout(envs, 8, 1)
    tb = TorchImageRollout(n, P, A, T, dev)
    tb.pixels[0] = img.reshape(n, -1)
    for pos, k in enumerate(first_rollout):
        tb.add(pos, *k)
    tb.gae(lv)
    assert torch.equal(tb.pixels, buf.pixels().reshape(T + 1, n, P))          # both formulations hold the same pictures
    del first_rollout
    res = {"env_id": ENV_ID, "envs": n, "size": args.size, "channels": buf.channels, "steps": T, "batch": B, "picture_bytes": P,
           "device": torch.cuda.get_device_name(0), "machine": args.machine, "hbm_spec_gbps": HBM_SPEC_GBPS, "hbm_copy_gbps": HBM_COPY_GBPS,
           "cases": {}}

    def report(name, r, nbytes=None):
        if nbytes is not None:
            r["bytes"] = nbytes
            r["gbps"] = nbytes / (r["median_ms"] * 1e-3) / 1e9
            r["of_hbm_spec"], r["of_hbm_copy"] = r["gbps"] / HBM_SPEC_GBPS, r["gbps"] / HBM_COPY_GBPS
        res["cases"][name] = r
        print(json.dumps({name: r}), flush=True)

    # ---- insertion
    cycle = itertools.cycle(kept)

    def add():
        if buf.full:
            buf.pos = 0          # (not reset(): the carry is a launch of its own and is not what is timed here)
        a, v, lp, fv, out = next(cycle)
        buf.add(a, v, lp, *out, final_values=fv)
    report("add", timed(add, warmup=5, reps=args.reps, inner=500), 2 * n * P)
    lib, stream = _abi.load(), C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    raw = []
    for a, v, lp, fv, (o, rew, term, trunc, info) in kept:
        raw.append((a, v, lp, fv, o, rew.double(), term, trunc))
    rcycle, state = itertools.cycle(raw), {"pos": 0}
    p = lambda t: C.c_void_p(t.data_ptr())

    def add_raw():
        a, v, lp, fv, o, rew, term, trunc = next(rcycle)
        _abi.check(lib.mcg_rollout_img_add(C.byref(buf._cbuf), state["pos"], p(a), p(v), p(lp), p(fv), p(o), o.stride(0), o.stride(1), p(rew),
                                           p(term), p(trunc), stream), "mcg_rollout_img_add")
        state["pos"] = (state["pos"] + 1) % T
    report("add_raw", timed(add_raw, warmup=5, reps=args.reps, inner=2000), 2 * n * P)
    tstate = {"pos": 0}

    def torch_add():
        tb.add(tstate["pos"], *next(cycle))
        tstate["pos"] = (tstate["pos"] + 1) % T
    report("torch_add", timed(torch_add, warmup=5, reps=args.reps, inner=200), 2 * n * P)
    # ---- the recursion
    buf.pos = T
    report("gae", timed(lambda: buf.finish(lv), warmup=3, reps=args.reps, inner=500))
    report("torch_gae", timed(lambda: tb.gae(lv), warmup=3, reps=args.reps, inner=10))
    # ---- an epoch of minibatches
    def epoch(get, **kw):
        def run():
            for _ in get(B, **kw):
                pass
        return run
    per_epoch = -(-M // B)
    for name, fn, factor in (("get_u8", epoch(buf.get, normalize=False), 2), ("get_f32", epoch(buf.get, normalize=True), 5),
                             ("torch_get_u8", epoch(tb.get, normalize=False), 2), ("torch_get_f32", epoch(tb.get, normalize=True), 5)):
        r = timed(fn, warmup=3, reps=args.reps, inner=10)
        r["launches_per_epoch"] = per_epoch
        report(name, r, factor * M * P)
    # ---- one launch of the gather alone, outputs preallocated: the kernel's own rate
    for normalize, factor in ((False, 2), (True, 5)):
        pix = torch.empty(B, P, dtype=torch.float32 if normalize else torch.uint8, device=dev)
        out = _abi.McgRolloutImgBatch(**{"pix_f32" if normalize else "pix": pix.data_ptr()})
        kstate = {"k": 0}

        def gather_raw():
            _abi.check(lib.mcg_rollout_img_gather(C.byref(buf._cbuf), 0, 0, kstate["k"] * B, B, C.byref(out), stream), "mcg_rollout_img_gather")
            kstate["k"] = (kstate["k"] + 1) % (M // B)
        report("gather_raw_f32" if normalize else "gather_raw_u8", timed(gather_raw, warmup=5, reps=args.reps, inner=1000), factor * B * P)
    c = res["cases"]
    res["ratio_to_torch"] = {k: c["torch_" + k]["median_ms"] / c[k]["median_ms"] for k in ("add", "gae", "get_u8", "get_f32")}
    print(json.dumps({"ratio_to_torch": res["ratio_to_torch"]}), flush=True)
    envs.close()
    del buf, tb, kept, raw
    torch.cuda.empty_cache()
    res["big_offsets"] = [big_offsets(s, 8192, 64, B, dev) for s in args.big_steps]
    print(json.dumps({"big_offsets": res["big_offsets"]}), flush=True)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1); f.write("\n")
    ok = all(v for b in res["big_offsets"] for k, v in b.items() if k.endswith("_equal"))
    sys.exit(0 if ok else "big offsets: a comparison failed")


if __name__ == "__main__":
    main()
