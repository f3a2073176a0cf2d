"""Frame stacking on the device (mcg_frame_stack_push, mcg_replay_img_sample_stacked; mycobotgym_amd/frame_stack.py and
ImageReplayBuffer(frame_stack=k)) against the rules restated in tests/indep_frame_stack.py, and on the real engine.  The inputs are the
synthetic events of tests/test_gpu_replay_img.py: 40 environments, a time limit of 5, 30 steps with masked restarts of five
environments before steps 3 and 17, A = 7, K = 12 sampleable transitions (a ring of K + k rows, which wraps), batches of 101, k = 2
and 4, and the four picture shapes at which the kernels take each of their paths (byte, 4-byte, 16-byte-partial, registered).

Wide storage is the specification: the stacked replay rule stores whole stacks in a ring k times as wide; the kernels must rebuild
the same stacks from single frames.
"""
import ctypes as C_
import functools

import numpy as np
import pytest

from tests.common import bits
from tests.indep_frame_stack import StackedReplay, StackRule
from tests.indep_replay_img import MAX_DRAWS, TERMINATED, TIMEOUT
from tests.test_gpu_replay_img import A, BATCH, GUARD, K, N, SNAP_AFTER, STEPS, TM, apply_event, batch_arrays, guards_intact, synthetic_events
from tests.test_gpu_rollout_img import picture

pytestmark = pytest.mark.gpu

KS = (2, 4)
SHAPES = [(2, 5), (2, 6), (3, 20), (1, 64)]
# The sampling seed.  The census conditions below were settled on the rule alone, on the CPU, before any GPU run
# (tests/test_frame_stack_cpu.py asserts them without a GPU).  Seed 0, the existing test's, misses one for k = 4: no sample's history
# crosses the ring's row 0 (the one place is time 18 at depth 4 after 30 steps).  Seed 1 is the first that gives all of them for both k.
SEED = 1


def run_stacked_rule(events, n, C, S, A, K, Tm, k, snap_after, batch, seed=SEED):
    """The stacked replay rule on the events: after each step of `snap_after` its cumulative counters and two batches (calls 2 i and
    2 i + 1: the test takes the normalised pictures of the first and the uint8 ones of the second)."""
    R = StackedReplay(n, C, S, A, K, Tm, k)
    snaps, give_ups, lost = [], 0, 0
    for ev in events:
        if ev[0] == "start":
            R.start(ev[1], ev[2])
            continue
        o = ev[2]
        R.add(ev[1], o["img"], o["final_img"], o["reward"], o["terminated"], o["truncated"])
        if R.n in snap_after:
            b = [R.sample(seed, 2 * len(snaps) + c, batch) for c in (0, 1)]
            give_ups += sum(x["give_ups"] for x in b)
            lost += sum(x["lost"] for x in b)
            snaps.append(dict(batches=b, give_ups=give_ups, lost=lost, n=R.n))
    return tuple(snaps)


@functools.lru_cache(maxsize=None)
def stacked_snapshots(C, S, k):
    """Computed once per shape and k, shared between the input layouts, not modified."""
    return run_stacked_rule(synthetic_events(C, S), N, C, S, A, K, TM, k, SNAP_AFTER, BATCH)


def census(snaps, k, K=K):
    """What the sampled inputs exercise.  A sample at time a of depth d uses the frames of times a - d + 1 .. a: its history lies
    before the sampling window where a - d + 1 < n - W, and crosses the ring's row 0 where a % (K + k) < d - 1."""
    c = {"samples": 0, "give_ups": 0, "timeout_from_finals": 0, "terminated": 0, "more_than_one_draw": 0, "before_window": 0,
         "across_row_0": 0, "lost": snaps[-1]["lost"], "depth": {d: 0 for d in range(1, k + 1)}}
    for s in snaps:
        n, W = s["n"], min(s["n"], K)
        for b in s["batches"]:
            took = b["draws"] <= MAX_DRAWS
            c["samples"] += len(b["draws"])
            c["give_ups"] += int((~took).sum())
            c["timeout_from_finals"] += int((((b["flags"] & TIMEOUT) != 0) & (b["index"][:, 2] == 1))[took].sum())
            c["terminated"] += int(((b["flags"] & TERMINATED) != 0)[took].sum())
            c["more_than_one_draw"] += int((b["draws"] > 1)[took].sum())
            c["before_window"] += int((b["time"] - b["depth"] + 1 < n - W)[took].sum())
            c["across_row_0"] += int((b["row"] < b["depth"] - 1)[took].sum())
            for d in range(1, k + 1):
                c["depth"][d] += int((b["depth"] == d)[took].sum())
    return c


def assert_census(c, k):
    assert c["give_ups"] == 0 and c["timeout_from_finals"] >= 10 and c["terminated"] >= 10 and c["more_than_one_draw"] >= 1, c
    assert all(c["depth"][d] >= 10 for d in range(1, k + 1)), c
    assert c["before_window"] >= 1 and c["across_row_0"] >= 1, c


# ----------------------------------------------------------------------------------------------------------------- push
PAD = 64          # guard bytes before and after each stack (a multiple of 16: the stack keeps the allocation's alignment)


class DeviceStack:
    """The caller's side of mcg_frame_stack_push as FrameStack does it, on tensors with guard bytes around them."""

    def __init__(self, n, C, S, k, device):
        import torch
        from mycobotgym_amd import _abi
        self.lib, self.abi, self.n, self.C, self.S, self.k, self.device = _abi.load(), _abi, n, C, S, k, device
        size = n * k * C * S * S
        self.raw = [torch.full((size + 2 * PAD,), GUARD, dtype=torch.uint8, device=device) for _ in range(2)]
        self.stack, self.final = (r[PAD:PAD + size].view(n, k * C, S, S) for r in self.raw)
        self.stack.zero_(); self.final.zero_()
        self.ones = torch.ones(n, dtype=torch.uint8, device=device)

    def push(self, img, final_img=None, done=None, mask=None):
        import torch
        p = lambda t: None if t is None else C_.c_void_p(t.data_ptr())
        f = final_img
        with torch.cuda.device(self.device):
            self.abi.check(self.lib.mcg_frame_stack_push(
                p(self.stack), None if f is None else p(self.final), self.n, self.C, self.S, self.k, p(img), img.stride(0), img.stride(1),
                p(f), 0 if f is None else f.stride(0), 0 if f is None else f.stride(1), p(done), p(mask),
                C_.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)), "mcg_frame_stack_push")

    def guards_intact(self):
        return all(bool((r[:PAD] == GUARD).all()) and bool((r[-PAD:] == GUARD).all()) for r in self.raw)


@pytest.mark.parametrize("layout", ["env", "contiguous"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("C,S", SHAPES)
def test_push_matches_the_rule(built, C, S, k, layout):
    """The 30 steps of the synthetic schedule, the initial reset and the masked restarts before steps 3 and 17: after every call the
    stack, and after every step the final stack, equal the act-time rule's bit for bit; the guard bytes around both stay intact."""
    import torch
    dev = torch.device("cuda:0")
    rule, got = StackRule(N, C, S, k), DeviceStack(N, C, S, k, dev)
    t = lambda x: torch.as_tensor(x, device=dev)
    steps = dones = 0
    for ev in synthetic_events(C, S):
        if ev[0] == "start":
            want = rule.reset(ev[1], ev[2])
            got.push(picture(ev[1], dev, layout), mask=got.ones if ev[2] is None else t(ev[2]).to(torch.uint8))
        else:
            o = ev[2]
            done = o["terminated"] | o["truncated"]
            want, want_final = rule.step(o["img"], o["final_img"], done)
            got.push(picture(o["img"], dev, layout), picture(o["final_img"], dev, layout), done=t(done).to(torch.uint8))
            assert np.array_equal(got.final.cpu().numpy(), want_final), (steps, "final stack")
            steps += 1
            dones += int(done.sum())
        assert np.array_equal(got.stack.cpu().numpy(), want), (steps, "stack")
        assert got.guards_intact(), steps
    assert steps == STEPS and dones >= N          # every environment's stack was cut, on average, more than once


def test_push_without_a_mask_restarts_where_done(built):
    """done = 1 everywhere and no final stack: what a reset of every environment gives."""
    import torch
    dev, (C, S, k) = torch.device("cuda:0"), (2, 6, 3)
    ev = synthetic_events(C, S)
    rule, got = StackRule(N, C, S, k), DeviceStack(N, C, S, k, dev)
    got.stack.fill_(7)
    got.push(picture(ev[0][1], dev, "env"), done=got.ones)
    assert np.array_equal(got.stack.cpu().numpy(), rule.reset(ev[0][1])) and not got.final.any() and got.guards_intact()


# ------------------------------------------------------------------------------------------------------ stacked sampling
def make_buffer(C, S, k, n=N, A=A, K=K, Tm=TM, seed=SEED, guard_rows=2):
    from mycobotgym_amd import ImageReplayBuffer
    buf = ImageReplayBuffer(capacity=K, seed=seed, num_envs=n, channels=C, image_size=S, act_dim=A, max_episode_steps=Tm, guard_rows=guard_rows,
                            frame_stack=k)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(GUARD)
    return buf


def apply_stacked(buf, ev, stacks: StackRule):
    """The event as whole stacks, contiguous [N, k * C, S, S]: the buffer takes their newest C channels as a strided view."""
    import torch
    t = lambda x: torch.as_tensor(x, device=buf.device)
    if ev[0] == "start":
        buf.start(t(stacks.reset(ev[1], ev[2])), mask=None if ev[2] is None else t(ev[2]))
    else:
        o = ev[2]
        stack, final = stacks.step(o["img"], o["final_img"], o["terminated"] | o["truncated"])
        buf.add(t(ev[1]), t(stack), t(o["reward"]), t(o["terminated"]), t(o["truncated"]), {"final_observation": t(final)})


def assert_stacked_batch_equals(got, want, normalize):
    suffix = "_f32" if normalize else ""
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"][:, 1:], want["index"][:, 1:])
    assert np.array_equal(got["index"][:, 0], want["row"])          # through the absolute time: a % (K + k), the rule's a % (K + 1)
    for name in ("pix", "next_pix"):
        w = want[name + suffix]
        assert got[name].dtype == w.dtype and got[name].shape == w.shape, name
        assert np.array_equal(bits(got[name]), bits(w)), name
    for name in ("action", "reward", "done"):
        assert got[name].dtype == np.float32 and got[name].shape == want[name].shape, name
        assert np.array_equal(bits(got[name]), bits(want[name])), name


def assert_stacked_samples_equal(buf, snap):
    """Both forms of a batch (normalised: the rule's call 2 i, uint8: call 2 i + 1), never synchronising, then the two counters."""
    for want, normalize in zip(snap["batches"], (True, False)):
        got = batch_arrays(buf.sample(len(want["draws"]), normalize=normalize, check=False))
        assert_stacked_batch_equals(got, want, normalize)
    assert buf.counters() == {"sample_give_ups": snap["give_ups"], "finals_overwritten": snap["lost"]}


@pytest.mark.parametrize("layout", ["env", "stacks"])
@pytest.mark.parametrize("k", KS)
@pytest.mark.parametrize("C,S", SHAPES)
def test_stacked_sampling_matches_the_rule(built, C, S, k, layout):
    """After steps 1, 4, 12, 13 and 30 every output of two batches of 101 (float32 and uint8 stacks of both observations) equals the
    wide-storage rule's bit for bit, the counters the rule's counts, and the guard rows around every array are intact.  "env": single
    frames in the environment's layout go in; "stacks": contiguous stacks, of which the buffer stores the newest frame."""
    snaps = stacked_snapshots(C, S, k)
    c = census(snaps, k)          # conditions of the inputs, settled on the rule before the GPU is touched
    print(f"{C} x {S} x {S}, k = {k}: {c}")
    assert_census(c, k)
    assert [s["n"] for s in snaps] == list(SNAP_AFTER) and snaps[-1]["n"] > K + k          # the ring has wrapped
    buf, stacks, done = make_buffer(C, S, k), StackRule(N, C, S, k), 0
    assert buf.pixels().shape[0] == K + k and buf.records().shape[0] == K + k and buf.frame_stack == k
    for ev in synthetic_events(C, S):
        if layout == "env":
            apply_event(buf, ev, "env")
        else:
            apply_stacked(buf, ev, stacks)
        if ev[0] == "add" and buf.n_written in SNAP_AFTER:
            assert_stacked_samples_equal(buf, snaps[done])
            assert buf.n_sampled == 2 * (done + 1) and guards_intact(buf)
            done += 1
    assert done == len(SNAP_AFTER) and guards_intact(buf)


@pytest.mark.parametrize("C,S", [(2, 5), (1, 64)])
def test_frame_stack_1_is_the_existing_entry(built, C, S):
    """mcg_replay_img_sample_stacked with frame_stack = 1 on an existing buffer: every output tensor equals mcg_replay_img_sample's."""
    import torch
    from mycobotgym_amd import _abi
    from tests.test_gpu_replay_img import make_buffer as make_plain
    buf = make_plain(C, S)
    assert buf.frame_stack == 1
    checked = 0
    for ev in synthetic_events(C, S):
        apply_event(buf, ev, "env")
        if ev[0] != "add" or buf.n_written not in SNAP_AFTER:
            continue
        for normalize in (True, False):
            call = buf.n_sampled
            want = batch_arrays(buf.sample(BATCH, normalize=normalize, check=False))
            dt = torch.float32 if normalize else torch.uint8
            t = {"pix_f32" if normalize else "pix": torch.empty(BATCH, C, S, S, dtype=dt, device=buf.device),
                 "next_pix_f32" if normalize else "next_pix": torch.empty(BATCH, C, S, S, dtype=dt, device=buf.device),
                 "action": torch.empty(BATCH, A, device=buf.device), "reward": torch.empty(BATCH, 1, device=buf.device),
                 "done": torch.empty(BATCH, 1, device=buf.device), "index": torch.empty(BATCH, 3, dtype=torch.int32, device=buf.device)}
            out = _abi.McgReplayImgBatch(**{k: v.data_ptr() for k, v in t.items()})
            buf._call("mcg_replay_img_sample_stacked", buf.n_written, C_.c_uint64(buf.seed), C_.c_uint64(call), BATCH, 1, C_.byref(out))
            got = {"pix": t["pix_f32" if normalize else "pix"], "next_pix": t["next_pix_f32" if normalize else "next_pix"],
                   "action": t["action"], "reward": t["reward"], "done": t["done"], "index": t["index"]}
            for name, w in want.items():
                assert np.array_equal(bits(got[name].cpu().numpy()), bits(w)), (buf.n_written, normalize, name)
            checked += 1
    assert checked == 2 * len(SNAP_AFTER) and guards_intact(buf)


def test_stamp_mismatch_with_stacks(built):
    """tests/test_gpu_replay_img.py's test_stamp_mismatch with k = 3: two timeouts of environment 0 inside one block of Tm (times 5 and
    7).  The older comes out with done = 1, counted in counters[1], and its next stack is zeros and the ring's successor; the newer
    keeps its stack, shifted, under its final picture."""
    n, C, S, Tm, K_, k = 4, 1, 8, 5, 8, 3
    rng = np.random.default_rng(1)
    pic = lambda: rng.integers(0, 200, (n, C, S, S), dtype=np.uint8)
    final = {5: np.full((n, C, S, S), 250, np.uint8), 7: np.full((n, C, S, S), 251, np.uint8)}          # no other picture has these bytes
    events = [("start", pic(), None)]
    for a in range(9):
        trunc = np.zeros(n, bool)
        trunc[0] = a in final
        events.append(("add", rng.uniform(-1, 1, (n, A)).astype(np.float32),
                       {"img": pic(), "final_img": final.get(a, pic()), "reward": rng.normal(size=n), "terminated": np.zeros(n, bool), "truncated": trunc}))
    snap = run_stacked_rule(events, n, C, S, A, K_, Tm, k, (9,), 256)[0]
    b = snap["batches"][1]
    older, newer = (b["time"] == 5) & (b["index"][:, 1] == 0), (b["time"] == 7) & (b["index"][:, 1] == 0)
    print(f"stamp mismatch, k = {k}: {int(older.sum())} samples of the older timeout, {int(newer.sum())} of the newer, lost {snap['lost']}")
    assert older.sum() >= 3 and newer.sum() >= 3 and snap["lost"] >= older.sum()
    assert (b["done"][older] == 1).all() and (b["index"][older, 2] == 0).all() and (b["done"][newer] == 0).all() and (b["index"][newer, 2] == 1).all()
    buf = make_buffer(C, S, k, n, A, K_, Tm)
    for ev in events:
        apply_event(buf, ev)
    assert_stacked_samples_equal(buf, snap)          # counters[1] == the rule's count among them
    buf.n_sampled = 1
    got = batch_arrays(buf.sample(256, normalize=False, check=False))
    ring = buf.pixels().cpu().numpy()
    R = K_ + k
    assert not got["next_pix"][older][:, :k - 1].any() and (got["next_pix"][older][:, k - 1] == ring[6 % R, 0, 0]).all()
    assert (got["done"][older] == 1).all() and not (got["next_pix"] == 250).any() and not (got["pix"] >= 250).any()
    assert (got["next_pix"][newer][:, k - 1] == 251).all() and (got["next_pix"][newer][:, :k - 1] == got["pix"][newer][:, 1:]).all()
    assert (got["pix"][newer][:, k - 1] == ring[7 % R, 0, 0]).all() and (got["pix"][newer][:, k - 2] == ring[6 % R, 0, 0]).all()
    assert not got["pix"][newer][:, 0].any()          # time 5 ended an episode: the stack of time 7 is two frames deep
    assert guards_intact(buf)


def test_buffer_checkpoint(built):
    """state_dict() in mid-ring (14 steps) into a new buffer of the same shape: the rest of the run and the next batch are identical,
    and they are the rule's."""
    import torch
    C, S, k = 3, 20, 4
    events = synthetic_events(C, S)
    cut = [i for i, ev in enumerate(events) if ev[0] == "add"][13] + 1
    buf = make_buffer(C, S, k)
    for ev in events[:cut]:
        apply_event(buf, ev)
        if ev[0] == "add" and buf.n_written in SNAP_AFTER:
            buf.sample(BATCH, check=False); buf.sample(BATCH, normalize=False, check=False)
    sd = buf.state_dict()
    assert {k_: v for k_, v in sd.items() if not torch.is_tensor(v)} == {"n_written": 14, "n_sampled": 8, "seed": SEED}
    other = make_buffer(C, S, k, seed=99)
    other.load_state_dict(sd)
    for ev in events[cut:]:
        apply_event(buf, ev); apply_event(other, ev)
    x, y = batch_arrays(buf.sample(BATCH)), batch_arrays(other.sample(BATCH))
    for name in x:
        assert np.array_equal(bits(x[name]), bits(y[name])), name
    assert_stacked_batch_equals(y, stacked_snapshots(C, S, k)[-1]["batches"][0], True)
    with pytest.raises(ValueError, match="pixels: expected"):
        make_buffer(C, S, 2).load_state_dict(sd)          # another frame_stack: another number of rows
    assert guards_intact(other)


def test_class_refusals(built):
    import torch
    from mycobotgym_amd import FrameStack, HerBuffer, ImageReplayBuffer, ImageRolloutBuffer, RolloutBuffer, make
    kw = dict(capacity=4, num_envs=3, channels=2, image_size=5, act_dim=7, max_episode_steps=5)
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"frame_stack must be in \[1, 8\]"):
            ImageReplayBuffer(frame_stack=k, **kw)
    buf = ImageReplayBuffer(frame_stack=3, **kw)
    assert buf.pixels().shape == (4 + 3, 3, 2, 5, 5)
    for c in (4, 8):          # neither a frame (2 channels) nor a stack (6)
        with pytest.raises(ValueError, match="img: expected shape"):
            buf.start(torch.zeros(3, c, 5, 5, dtype=torch.uint8, device=buf.device))
    buf.start(torch.zeros(3, 6, 5, 5, dtype=torch.uint8, device=buf.device))
    buf.start(torch.zeros(3, 2, 5, 5, dtype=torch.uint8, device=buf.device))
    v1 = make("MyCobotReach-Dense-joint-v1", num_envs=2, image_size=16, max_episode_steps=9, camera=("sideview", "gripper_camera_rgb"))
    for k in (0, 9):
        with pytest.raises(ValueError, match=r"frame_stack must be in \[1, 8\]"):
            FrameStack(v1, k)
    fs = FrameStack(v1, 3)
    assert (fs.channels, fs.frame_channels, fs.frame_stack, fs.num_envs, fs.image_size, fs.max_episode_steps) == (6, 2, 3, 2, 16, 9)
    assert fs.single_observation_space.shape == (6, 16, 16) and fs.observation_space.shape == (2, 6, 16, 16) and fs.envs is v1
    rb = ImageReplayBuffer(fs, capacity=4)
    assert (rb.channels, rb.frame_stack, rb.num_envs, rb.image_size, rb.act_dim, rb.max_episode_steps) == (2, 3, 2, 16, v1.action_dim, 9)
    assert ImageRolloutBuffer(fs, n_steps=4).channels == 6          # wide storage until the rollout buffer gathers stacks
    with pytest.raises(ValueError, match="the -v1 image ids carry no goals in their observation"):
        HerBuffer(fs)
    with pytest.raises(ValueError):
        RolloutBuffer(fs)
    v1.close()
    v0 = make("MyCobotReach-Dense-joint-v0", num_envs=2)
    with pytest.raises(ValueError, match="FrameStack wraps a MyCobotImgVecEnv"):
        FrameStack(v0, 2)
    v0.close()


# ------------------------------------------------------------------------------------------------------------ real engine
def test_with_the_real_engine(built):
    """FrameStack(make(...-v1, num_envs=64), 3) for 60 steps (the 50-step time limit passes) into ImageReplayBuffer(fs, capacity=20).
    The stacks handed out equal the act-time rule applied to their own newest-channel slices and the done flags; every sampled
    `observations` equals the stack the wrapper handed out at that time, every `next_observations` the next one, or the stacked
    final_observation where the time limit ended the episode."""
    import torch
    from mycobotgym_amd import FrameStack, ImageReplayBuffer, make
    n, k, K_, steps, env_id = 64, 3, 20, 60, "MyCobotReach-Dense-joint-v1"
    fs = FrameStack(make(env_id, num_envs=n, seed=3), k)
    buf = ImageReplayBuffer(fs, capacity=K_, seed=SEED, guard_rows=1)
    Cc, S, Aa = fs.frame_channels, fs.image_size, fs.action_dim
    assert (Cc, S, fs.channels, fs.max_episode_steps) == (1, 64, 3, 50) and buf.pixels().shape[:2] == (K_ + k, n)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(GUARD)
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    host = lambda x: x.cpu().numpy()
    stack, _ = fs.reset(seed=0)
    assert tuple(stack.shape) == (n, k * Cc, S, S) and stack.dtype == torch.uint8
    buf.start(stack)
    rule = StackRule(n, Cc, S, k)
    assert np.array_equal(host(stack), rule.reset(host(stack)[:, (k - 1) * Cc:]))
    handed, log, timeouts = [host(stack)], [], 0
    for t in range(steps):
        a = (torch.rand(n, Aa, generator=gen) * 2 - 1).to(fs.device)
        stack, r, term, trunc, info = fs.step(a)
        buf.add(a, stack, r, term, trunc, info)
        s = {"terminated": host(term), "truncated": host(trunc), "final": host(info["final_observation"]), "action": host(a)}
        want, want_final = rule.step(host(stack)[:, (k - 1) * Cc:], s["final"][:, (k - 1) * Cc:], s["terminated"] | s["truncated"])
        assert np.array_equal(host(stack), want), (t, "stack")
        assert np.array_equal(s["final"], want_final), (t, "final stack")
        handed.append(host(stack)); log.append(s)
        timeouts += int((s["truncated"] & ~s["terminated"]).sum())
        if t + 1 in (10, steps):
            m = t + 1
            W = min(m, K_)
            time_of_row = {a_ % (K_ + k): a_ for a_ in range(m - W, m)}
            raw = batch_arrays(buf.sample(512, normalize=False))
            sampled_timeouts = shallow = 0
            for j, (row, e, src) in enumerate(raw["index"].tolist()):
                at = time_of_row[row]
                w = log[at]
                timeout = bool(w["truncated"][e]) and not bool(w["terminated"][e])
                sampled_timeouts += timeout
                shallow += not raw["pix"][j, 0].any()
                assert src == int(timeout), (j, "source")
                assert np.array_equal(raw["pix"][j], handed[at][e]), (j, "stack")
                assert np.array_equal(raw["next_pix"][j], w["final"][e] if timeout else handed[at + 1][e]), (j, "next stack")
                assert np.array_equal(bits(raw["action"][j]), bits(w["action"][e])), (j, "action")
                assert raw["done"][j, 0] == float(w["terminated"][e]), (j, "done")
            print(f"after {m} steps: {sampled_timeouts} of 512 samples are time-limit ends, {shallow} have an empty oldest slot")
            if m == steps:
                assert sampled_timeouts >= 10 and shallow >= 10
    assert timeouts >= n // 2
    assert buf.counters() == {"sample_give_ups": 0, "finals_overwritten": 0} and guards_intact(buf)
    fs.close()


def test_frame_stack_checkpoint_and_masked_reset(built):
    """state_dict() after five steps into a fresh FrameStack: the same action gives the same stack and final stack.  A masked reset
    restarts the stacks of the mask alone."""
    import torch
    from mycobotgym_amd import FrameStack, make
    kw = dict(num_envs=8, image_size=16, max_episode_steps=4, seed=3)
    env_id, k = "MyCobotReach-Dense-joint-v1", 4
    fs, other = FrameStack(make(env_id, **kw), k), FrameStack(make(env_id, **kw), k)
    gen = torch.Generator(device="cpu"); gen.manual_seed(1)
    act = lambda: (torch.rand(8, fs.action_dim, generator=gen) * 2 - 1).to(fs.device)
    fs.reset(seed=0); other.reset(seed=1)
    for _ in range(5):          # the time limit of 4 passes: the stacks are two frames deep
        stack = fs.step(act())[0]
    assert not stack[:, :2].any() and stack[:, 2].any() and stack[:, 3].any()
    sd = fs.state_dict()
    assert set(sd) == {"envs", "stack"} and torch.equal(sd["stack"], stack)
    other.load_state_dict(sd)
    a = act()
    x, y = fs.step(a), other.step(a)
    assert torch.equal(x[0], y[0]) and torch.equal(x[4]["final_observation"], y[4]["final_observation"])
    assert torch.equal(x[0][:, :3], stack[:, 1:]) and x[0][:, 1].any()
    mask = torch.tensor([1, 0, 0, 1, 0, 0, 0, 0], dtype=torch.bool, device=fs.device)
    z, _ = fs.reset(mask=mask)
    assert torch.equal(z[~mask], x[0][~mask]) and not z[mask][:, :3].any() and z[mask][:, 3].any()
    live, own = fs.step(a, copy=False)[0], fs.step(a)[0]
    assert live.data_ptr() == fs._stack.data_ptr() and own.data_ptr() != live.data_ptr() and torch.equal(live, own)
    with pytest.raises(ValueError, match="stack: expected"):
        FrameStack(fs.envs, 2).load_state_dict(sd)
    fs.close(); other.close()


def test_sb3_adapter_over_a_frame_stack(built):
    """MyCobotSB3VecEnv(FrameStack(...)) through the pass-through: stacked numpy observations and a stacked terminal_observation."""
    from mycobotgym_amd import FrameStack, make
    from mycobotgym_amd.sb3_adapter import MyCobotSB3VecEnv
    fs = FrameStack(make("MyCobotReach-Dense-joint-v1", num_envs=4, image_size=16, max_episode_steps=3, seed=3), 2)
    venv = MyCobotSB3VecEnv(fs)
    assert venv.num_envs == 4 and tuple(venv.observation_space.shape) == (2, 16, 16)
    obs = venv.reset()
    assert obs.shape == (4, 2, 16, 16) and obs.dtype == np.uint8 and not obs[:, 0].any() and obs[:, 1].any()
    prev = obs
    for t in range(3):
        obs, rew, dones, infos = venv.step(np.zeros((4, fs.action_dim), np.float32))
        assert obs.shape == (4, 2, 16, 16) and rew.shape == (4,) and dones.shape == (4,)
        for e in np.nonzero(dones)[0]:
            term = infos[e]["terminal_observation"]
            assert term.shape == (2, 16, 16) and np.array_equal(term[0], prev[e, 1]) and not obs[e, 0].any()
        for e in np.nonzero(~dones)[0]:
            assert np.array_equal(obs[e, 0], prev[e, 1])
        prev = obs
    assert dones.all()          # the time limit of 3
    venv.close()
