"""Stacked gathers from the picture rollout buffer (mcg_rollout_img_carry_stacked, mcg_rollout_img_gather_stacked,
ImageRolloutBuffer(frame_stack=k)) against wide storage, bit for bit: tests/indep_rollout_img_stacked.WideStackedRollout, the existing
rule with k * C channels fed the act-time rule's stacks.  The history rows are compared with the restated single-frame rule of the
same file, which tests/test_rollout_img_stacked_cpu.py holds equal to the wide one on these event lists.

The event schedule, the shapes (byte, 4-byte, 16-byte-partial and registered paths) and the layouts are tests/test_gpu_rollout_img.py's:
40 environments, 7 steps, episode lengths 1 .. 7, a masked restart before step 3, minibatches of 64 with a short last one -- over three
rollouts, so that a history row is itself a carried row once.  The second schedule has n_steps = 2 at k = 4: every carry overlaps its
own source, a stack reaches across two earlier rollouts, and one reset() comes at pos = 1 on an unfinished rollout.
"""
import functools

import numpy as np
import pytest

from tests.common import bits
from tests.indep_rollout import PERM_SEED
from tests.indep_frame_stack import StackRule
from tests.indep_rollout_img_stacked import FrameRollout, WideStackedRollout
from tests.test_gpu_rollout_img import (A, GAMMA, LAMBDA, N, PLANES, T, assert_epoch_equals, batch_arrays, guards_intact, make_buffer,
                                        minibatches, picture, synthetic_events)

pytestmark = pytest.mark.gpu

PICTURES = [(2, 5), (2, 6), (3, 20), (1, 64)]
SHORT_T = 2


@functools.lru_cache(maxsize=None)
def schedule(C, S, kind):
    """("start", img, mask), ("add", ...), ("finish", last_values) as synthetic_events makes them, and ("reset",).  "main": three rollouts
    of 7 steps, reset() after every finish.  "short": n_steps = 2; rollouts of steps 0-1, 2-3, then step 4 alone and a reset() at
    pos = 1, then 5-6 and 7-8."""
    if kind == "main":
        out = []
        for ev in synthetic_events(C, S, rollouts=3):
            out.append(ev)
            if ev[0] == "finish":
                out.append(("reset",))
        return tuple(out)
    ev = synthetic_events(C, S, steps=SHORT_T, rollouts=5, restart_at=None)
    adds = [e for e in ev if e[0] == "add"]
    fins = [e for e in ev if e[0] == "finish"]
    r = ("reset",)
    return (ev[0], adds[0], adds[1], fins[0], r, adds[2], adds[3], fins[1], r, adds[4], r, adds[5], adds[6], fins[2], r, adds[7], adds[8],
            fins[3], r)


@functools.lru_cache(maxsize=None)
def stack_inputs(C, S, k, kind):
    """Per event of the schedule: the whole stack a FrameStack would hand the buffer there (None for finish and reset)."""
    rule, out = StackRule(N, C, S, k), []
    for ev in schedule(C, S, kind):
        if ev[0] == "start":
            out.append(rule.reset(ev[1], ev[2]))
        elif ev[0] == "add":
            o = ev[5]
            out.append(rule.step(o["img"], o["final_img"], o["terminated"] | o["truncated"])[0])
        else:
            out.append(None)
    return tuple(out)


def feed_rule(R, ev):
    if ev[0] == "start":
        R.start(ev[1], ev[2])
    elif ev[0] == "add":
        o = ev[5]
        R.add(ev[1], ev[2], ev[3], o["img"], o["reward"], o["terminated"], o["truncated"], final_values=ev[4])
    elif ev[0] == "finish":
        R.finish(ev[1])
    else:
        R.reset()


@functools.lru_cache(maxsize=None)
def rule_snapshots(C, S, k, kind, batch=64):
    """Both rules on the schedule.  After every finish: the wide rule's newest frames, planes, last_start and minibatches, and the
    single-frame rule's minibatches beside them.  After every reset: row 0, the history rows with their padding and their flags.
    Computed once per (shape, k, schedule), shared between the layouts and the two ways of feeding, not modified."""
    steps = T if kind == "main" else SHORT_T
    W = WideStackedRollout(N, C, S, A, steps, GAMMA, LAMBDA, k)
    F = FrameRollout(N, C, S, A, steps, GAMMA, LAMBDA, k)
    finished, carried = [], []
    for ev in schedule(C, S, kind):
        feed_rule(W, ev); feed_rule(F, ev)
        if ev[0] == "finish":
            epoch = len(finished)
            mbs = minibatches(steps * N, batch)
            finished.append({"frames": W.frames(), "planes": W.planes(), "last_start": W.last_start(),
                             "batches": [W.gather(PERM_SEED, epoch, first, count) for first, count in mbs],
                             "single": [F.gather(PERM_SEED, epoch, first, count) for first, count in mbs]})
        elif ev[0] == "reset":
            carried.append({"row0": W.frames()[0], "history": F.history(), "history_start": F.history_start(), "last_start": W.last_start()})
    return tuple(finished), tuple(carried)


def feed(buf, ev, layout, stack=None):
    """One event into the device buffer; `stack`: the whole stack in place of the single frame."""
    import torch
    t = lambda x: torch.as_tensor(x, device=buf.device)
    if ev[0] == "start":
        buf.start(picture(ev[1] if stack is None else stack, buf.device, layout), mask=None if ev[2] is None else t(ev[2]))
    elif ev[0] == "add":
        o = ev[5]
        buf.add(t(ev[1]), t(ev[2]), t(ev[3]), picture(o["img"] if stack is None else stack, buf.device, layout), t(o["reward"]),
                t(o["terminated"]), t(o["truncated"]), {"final_observation": None}, final_values=t(ev[4]))
    elif ev[0] == "finish":
        buf.finish(t(ev[1]))
    else:
        buf.reset()


def assert_history_equals(buf, want):
    sd = buf.state_dict()
    k = buf.frame_stack
    assert tuple(sd["history"].shape) == (k - 1, buf.num_envs, buf.row_bytes) and tuple(sd["history_start"].shape) == (k - 1, buf.num_envs)
    assert sd["history"].cpu().numpy().tobytes() == want["history"].tobytes()                  # padding included
    assert np.array_equal(sd["history_start"].cpu().numpy(), want["history_start"])
    view = buf.history()
    assert tuple(view.shape) == (k - 1, buf.num_envs, buf.channels, buf.image_size, buf.image_size)
    assert np.array_equal(view.cpu().numpy().reshape(k - 1, buf.num_envs, -1), want["history"][:, :, :buf.picture_bytes])


def assert_rollout_equals(buf, snap, history):
    """pixels(), history(), the planes and last_start after a finish; `history`: what the reset before this rollout left (None: the
    first rollout, whose history rows are the zeros they were allocated as)."""
    px = buf.pixels()
    assert tuple(px.shape) == (buf.n_steps + 1, buf.num_envs, buf.channels, buf.image_size, buf.image_size)
    assert np.array_equal(px.cpu().numpy(), snap["frames"])
    sd = buf.state_dict()
    assert tuple(sd["pixels"].shape) == (buf.n_steps + 1, buf.num_envs, buf.row_bytes)
    assert not sd["pixels"][:, :, buf.picture_bytes:].any()                                      # the padding of every row
    if history is None:
        assert not sd["history"].any() and not sd["history_start"].any()
    else:
        assert_history_equals(buf, history)
    P = {name: v.cpu().numpy() for name, v in buf.planes().items()}
    for name in PLANES:
        assert P[name].shape == (buf.n_steps, buf.num_envs) and np.array_equal(bits(P[name]), bits(snap["planes"][name])), name
    assert np.array_equal(sd["last_start"].cpu().numpy(), snap["last_start"])


def run_schedule(C, S, k, kind, layout, stacks, batch=64):
    finished, carried = rule_snapshots(C, S, k, kind, batch)
    steps = T if kind == "main" else SHORT_T
    buf = make_buffer(C, S, N, steps, A, guard_rows=1, frame_stack=k)
    whole = stack_inputs(C, S, k, kind) if stacks else None
    fin = res = 0
    for i, ev in enumerate(schedule(C, S, kind)):
        feed(buf, ev, layout, None if whole is None else whole[i])
        if ev[0] == "finish":
            assert_rollout_equals(buf, finished[fin], carried[res - 1] if res else None)
            got = assert_epoch_equals(buf, finished[fin], batch)
            assert got[0]["pix"].shape[1:] == (k * C, S, S)
            assert guards_intact(buf)
            fin += 1
        elif ev[0] == "reset":
            want = carried[res]
            assert buf.pos == 0 and np.array_equal(buf.pixels()[0].cpu().numpy(), want["row0"])
            assert_history_equals(buf, want)
            assert np.array_equal(buf.state_dict()["last_start"].cpu().numpy(), want["last_start"])
            assert guards_intact(buf)
            res += 1
    assert fin == len(finished) and res == len(carried)
    return buf


CASES = [(k, C, S, layout, stacks) for k in (2, 4) for C, S in PICTURES
         for layout, stacks in ([("env", False), ("contiguous", True)] + ([("env", True), ("contiguous", False)] if S == 20 else []))]


@pytest.mark.parametrize("k,C,S,layout,stacks", CASES)
def test_main_schedule_matches_wide_storage(built, k, C, S, layout, stacks):
    """Three rollouts of 7 steps with reset() between them, a masked restart before step 3: after every finish pixels(), history(),
    the planes, last_start and every tensor of the five minibatches of get(64) (float32 and uint8 stacks) equal the wide rule's byte
    for byte; after every reset() row 0, the history rows and their flags; the guard rows stay untouched.  At k = 4 the shape (3, 20) is
    12 channels, which wide storage on the device refuses."""
    buf = run_schedule(C, S, k, "main", layout, stacks)
    assert (buf.channels, buf.frame_stack) == (C, k) and buf.epoch == 3
    if k * C > 8:
        import torch
        from mycobotgym_amd import _abi
        with pytest.raises(_abi.McgError, match="channels must be <= 8"):
            make_buffer(k * C, S).start(torch.zeros(N, k * C, S, S, dtype=torch.uint8, device=buf.device))


@pytest.mark.parametrize("C,S,layout,stacks", [(2, 5, "env", False), (3, 20, "contiguous", True), (1, 64, "env", False)])
def test_overlapping_carry(built, C, S, layout, stacks):
    """n_steps = 2, k = 4, four rollouts and a reset() at pos = 1 on an unfinished one: every carry has pos < k - 1, so its source and
    destination rows overlap, and a stack of full depth at step 0 spans three rollouts (the census of the inputs is in
    tests/test_rollout_img_stacked_cpu.py)."""
    buf = run_schedule(C, S, 4, "short", layout, stacks, batch=64)
    assert buf.n_steps == SHORT_T and buf.epoch == 4


@pytest.mark.parametrize("C,S,k", [(2, 6, 4), (1, 64, 4), (2, 5, 2)])
def test_against_wide_storage_on_the_device(built, C, S, k):
    """An ImageRolloutBuffer of k * C <= 8 channels and the same seed, fed the act-time rule's stacks, beside the single-frame buffer fed
    the frames: every tensor of every minibatch is equal, `index` too."""
    import torch
    single = make_buffer(C, S, guard_rows=1, frame_stack=k)
    wide = make_buffer(k * C, S, guard_rows=1)
    whole = stack_inputs(C, S, k, "main")
    done = 0
    for ev, stack in zip(schedule(C, S, "main"), whole):
        feed(single, ev, "env")
        feed(wide, ev, "env", stack)
        if ev[0] == "finish":
            for normalize in (True, False):
                e0, e1 = single.epoch, wide.epoch
                assert e0 == e1
                for a, b in zip(single.get(64, normalize=normalize), wide.get(64, normalize=normalize)):
                    for name in a._fields:
                        x, y = getattr(a, name), getattr(b, name)
                        assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x, y), (done, name)      # (no nan: bytes and normal draws)
            done += 1
    assert done == 3 and guards_intact(single) and guards_intact(wide)
    assert single.pixels().numel() * k == wide.pixels().numel()


def test_frame_stack_one_is_the_existing_entries(built):
    """frame_stack = 1 through the two new entries called directly: the gather's eight outputs equal mcg_rollout_img_gather's tensor
    for tensor, uint8 and float32, and the carry leaves what mcg_rollout_img_carry leaves."""
    import ctypes as Ct
    import torch
    from mycobotgym_amd import _abi
    C, S = 3, 20
    a, b = make_buffer(C, S, guard_rows=1), make_buffer(C, S, guard_rows=1)
    for ev in schedule(C, S, "main"):
        if ev[0] == "reset":
            break
        feed(a, ev, "env"); feed(b, ev, "env")
    M = T * N
    f32 = dict(dtype=torch.float32, device=a.device)
    for first, count in minibatches(M, 64):
        for normalize in (True, False):
            want = a.gather(0, first, count, normalize=normalize)
            t = {"pix_f32" if normalize else "pix": torch.empty(count, C, S, S, dtype=torch.float32 if normalize else torch.uint8, device=a.device),
                 "action": torch.empty(count, A, **f32), "old_value": torch.empty(count, **f32), "old_log_prob": torch.empty(count, **f32),
                 "advantage": torch.empty(count, **f32), "returns": torch.empty(count, **f32),
                 "index": torch.empty(count, dtype=torch.int32, device=a.device)}
            out = _abi.McgRolloutImgBatch(**{name: v.data_ptr() for name, v in t.items()})
            a._call("mcg_rollout_img_gather_stacked", 1, Ct.c_uint64(a.seed), Ct.c_uint64(0), first, count, Ct.byref(out))
            got = (t["pix_f32" if normalize else "pix"], t["action"], t["old_value"], t["old_log_prob"], t["advantage"], t["returns"], t["index"])
            for name, x, y in zip(want._fields, got, want):
                assert torch.equal(x, y), (first, normalize, name)
    a.reset()
    b._call("mcg_rollout_img_carry_stacked", b.pos, 1)
    sa, sb = a.state_dict(), b.state_dict()
    for name in sa:
        if torch.is_tensor(sa[name]):
            assert torch.equal(sa[name], sb[name]), name
    assert guards_intact(a) and guards_intact(b)


def test_checkpoint_round_trip(built):
    """state_dict() three steps into the second rollout at k = 3 into a new buffer: the history rows and their flags travel with it, and
    the third rollout's minibatches equal those of the run that was not interrupted, and the rule's."""
    import torch
    C, S, k = 2, 6, 3
    events = schedule(C, S, "main")
    cut = [i for i, ev in enumerate(events) if ev[0] == "reset"][0] + 1 + 3
    buf = make_buffer(C, S, frame_stack=k)
    for ev in events[:cut]:
        feed(buf, ev, "env")
        if ev[0] == "finish":
            list(buf.get(64))
    sd = buf.state_dict()
    assert {name: v for name, v in sd.items() if not torch.is_tensor(v)} == {"pos": 3, "epoch": 1, "seed": PERM_SEED, "finished": False}
    assert len(sd) == 14 and sd["history"].any() and sd["history_start"].any()
    other = make_buffer(C, S, frame_stack=k)
    other.seed = 99
    other.load_state_dict(sd)
    with pytest.raises(ValueError, match="history"):
        make_buffer(C, S, frame_stack=k + 1).load_state_dict(sd)
    fin = 0
    finished, _ = rule_snapshots(C, S, k, "main")
    for ev in events[cut:]:
        feed(buf, ev, "env"); feed(other, ev, "env")
        if ev[0] == "finish":
            fin += 1
            assert buf.epoch == other.epoch == fin
            for x, y in zip(buf.get(64), other.get(64)):
                x, y = batch_arrays(x), batch_arrays(y)
                for name in x:
                    assert np.array_equal(bits(x[name]), bits(y[name])), name
            other.epoch = fin                  # the same epoch once more, against the rule
            assert_epoch_equals(other, finished[fin], 64)
    assert fin == 2
    a, b = buf.state_dict(), other.state_dict()
    for name in a:
        assert torch.equal(a[name], b[name]) if torch.is_tensor(a[name]) else a[name] == b[name], name


def test_class_refusals(built):
    import torch
    from mycobotgym_amd import FrameStack, ImageRolloutBuffer, make
    for bad in (0, -1, 9):
        with pytest.raises(ValueError, match=r"frame_stack must be in \[1, 8\]"):
            ImageRolloutBuffer(n_steps=4, num_envs=3, channels=2, image_size=5, act_dim=7, frame_stack=bad)
    envs = make("MyCobotReach-Dense-joint-v1", num_envs=2, image_size=16)
    fs = FrameStack(envs, 3)
    with pytest.raises(ValueError, match="the FrameStack stacks 3 frames"):
        ImageRolloutBuffer(fs, n_steps=4, frame_stack=2)
    assert ImageRolloutBuffer(fs, n_steps=4).channels == 3 and ImageRolloutBuffer(fs, n_steps=4, frame_stack=1).channels == 3      # wide, as before
    buf = ImageRolloutBuffer(fs, n_steps=4, frame_stack=3)
    assert (buf.channels, buf.frame_stack, buf.num_envs, buf.image_size) == (1, 3, 2, 16)
    assert tuple(buf.pixels().shape) == (5, 2, 1, 16, 16) and tuple(buf.history().shape) == (2, 2, 1, 16, 16)
    plain = ImageRolloutBuffer(envs, n_steps=4, frame_stack=3)          # a plain env: channels as it gives them
    assert (plain.channels, plain.frame_stack) == (1, 3)
    envs.close()
    for channels in (2, 4):          # neither C = 1 nor k * C = 3
        with pytest.raises(ValueError, match="expected shape"):
            buf.start(torch.zeros(2, channels, 16, 16, dtype=torch.uint8, device=buf.device))
    buf.start(torch.zeros(2, 3, 16, 16, dtype=torch.uint8, device=buf.device))
    buf.start(torch.zeros(2, 1, 16, 16, dtype=torch.uint8, device=buf.device))


def test_with_the_real_engine(built):
    """FrameStack(make(..., num_envs=64), 3), two rollouts of 8 steps into ImageRolloutBuffer(fs, n_steps=8, frame_stack=3): every
    gathered stack is the stack the wrapper handed out for that (env, step), found through `index`; so the second rollout's first steps
    reach into the carried rows."""
    import torch
    from mycobotgym_amd import FrameStack, ImageRolloutBuffer, make
    n, steps, k = 64, 8, 3
    fs = FrameStack(make("MyCobotReach-Dense-joint-v1", num_envs=n), k)
    buf = ImageRolloutBuffer(fs, n_steps=steps, frame_stack=k, seed=PERM_SEED, guard_rows=1)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(0xA5)
    Cc, S, Aa = fs.frame_channels, fs.image_size, fs.action_dim
    assert (buf.channels, buf.image_size, buf.act_dim) == (Cc, S, Aa)
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    stack, _ = fs.reset(seed=0)
    buf.start(stack)
    deep = 0
    for rollout in range(2):
        seen_from = []
        for _ in range(steps):
            seen_from.append(stack.cpu().numpy())
            a = (torch.rand(n, Aa, generator=gen) * 2 - 1).to(fs.device)
            stack, r, term, trunc, info = fs.step(a)
            buf.add(a, torch.zeros(n), torch.zeros(n), stack, r, term, trunc, info)
        buf.finish(torch.zeros(n))
        count = 0
        for mb in buf.get(128, normalize=False):
            pix, idx = mb.observations.cpu().numpy(), mb.index.cpu().numpy()
            assert pix.shape[1:] == (k * Cc, S, S)
            for j, i in enumerate(idx.tolist()):
                e, t = divmod(i, steps)
                assert np.array_equal(pix[j], seen_from[t][e]), (rollout, e, t)
                deep += int(rollout == 1 and t < k - 1 and seen_from[t][e][:(k - 1 - t) * Cc].any())
            count += len(idx)
        assert count == steps * n
        buf.reset()
    print(f"{deep} samples of the second rollout hold frames of the first")
    assert deep >= n          # a condition of the inputs: no episode ends within 16 steps of a 50-step limit unless the arm succeeds
    assert guards_intact(buf)
    fs.envs.close()
