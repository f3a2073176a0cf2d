"""The device-resident picture replay buffer (mcg_replay_img_*, mycobotgym_amd/replay_img.py) against the rule restated in
tests/indep_replay_img.py, and on the real engine.  Shapes: 40 environments, K = 12 transitions kept (13 rows), a time limit of 5
(F = 4 final rows), 30 steps (the ring wraps twice), A = 7 (a record of 9 words and 12 bytes of zeros; A = 2 in one case: exactly 16
bytes), batches of 101 (25 full blocks of four waves and a ragged one), and the pictures of tests/test_gpu_rollout_img.py, at which
the kernels take each of their paths:

    C = 2, S = 5    P = 50 + 14: planes at odd addresses (byte loads), byte stores in the sample, less than one pass of a wave
    C = 2, S = 6    P = 72 + 8:  planes and rows at multiples of 4 only (4-byte loads and stores)
    C = 3, S = 20   P = 1200:    16-byte loads and stores; two pictures are 150 units: one full pass of 64 lanes and partial ones
    C = 1, S = 64   P = 4096:    the registered shape; two pictures fill the eight loads in flight of every lane exactly
"""
import functools

import numpy as np
import pytest

from tests.common import bits
from tests.indep_replay_img import MAX_DRAWS, NO_NEXT, TERMINATED, TIMEOUT, ImageReplay, record_dtype
from tests.test_gpu_rollout_img import picture

pytestmark = pytest.mark.gpu

N, A, K, TM, STEPS, BATCH = 40, 7, 12, 5, 30, 101
STARTS_BEFORE, RESTARTED = (3, 17), 5
SNAP_AFTER = (1, 4, 12, 13, 30)
# The sampling seed.  The conditions of the inputs (no give-up, >= 10 sampled timeouts, >= 10 sampled terminations, a sample that needed
# more than one draw) were settled on the rule alone, before any GPU run; test_synthetic_events_match_the_rule asserts and prints them.
SEED = 0
GUARD = 0xA5
ARRAYS = ("pixels", "finals", "final_time", "records")


@functools.lru_cache(maxsize=None)
def synthetic_events(C, S, n=N, steps=STEPS, A=A, Tm=TM):
    """("start", img, mask) and ("add", actions, out) events from default_rng(0).  The schedule (episode lengths uniform in 1..Tm, the
    masked starts, the flags, rewards and actions) is drawn first and does not depend on the picture's shape; the pictures after it.
    An episode of exactly Tm steps ends by the time limit (truncated; on a random 30 % of those the engine's other form, terminated
    with it, which is no timeout), a shorter one by termination; before steps 3 and 17 a masked start restarts five environments in
    whatever state they are.  out["final_img"] differs from the post-reset picture out["img"]."""
    rng = np.random.default_rng(0)
    plan = []
    left, age = rng.integers(1, Tm + 1, n), np.zeros(n, int)
    for i in range(steps):
        mask = None
        if i in STARTS_BEFORE:
            mask = np.zeros(n, dtype=bool)
            mask[rng.choice(n, min(RESTARTED, n), replace=False)] = True
            left[mask], age[mask] = rng.integers(1, Tm + 1, int(mask.sum())), 0
        left -= 1
        age += 1
        done = left == 0
        truncated = done & (age == Tm)
        terminated = (done & ~truncated) | (truncated & (rng.random(n) < 0.3))
        plan.append((mask, rng.uniform(-1, 1, (n, A)).astype(np.float32), rng.normal(size=n), terminated, truncated))
        left[done], age[done] = rng.integers(1, Tm + 1, int(done.sum())), 0
    pic = lambda: rng.integers(0, 256, (n, C, S, S), dtype=np.uint8)
    events = [("start", pic(), None)]
    for mask, actions, reward, terminated, truncated in plan:
        if mask is not None:
            events.append(("start", pic(), mask))
        events.append(("add", actions, {"img": pic(), "final_img": pic(), "reward": reward, "terminated": terminated, "truncated": truncated}))
    return tuple(events)


def run_rule(events, n, C, S, A, K, Tm, snap_after, batch, seed=SEED):
    """The rule on the events: after each step of `snap_after` its arrays, its cumulative counters and two batches (calls 2 i and
    2 i + 1: the test takes the normalised pictures of the first and the uint8 ones of the second)."""
    R = ImageReplay(n, C, S, A, K, Tm)
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
            snaps.append(dict(R.arrays(), batches=b, give_ups=give_ups, lost=lost, n=R.n))
    return tuple(snaps)


@functools.lru_cache(maxsize=None)
def rule_snapshots(C, S, n=N, steps=STEPS, A=A, K=K, Tm=TM):
    """Computed once per shape, shared between the input layouts, not modified."""
    return run_rule(synthetic_events(C, S, n, steps, A, Tm), n, C, S, A, K, Tm, SNAP_AFTER, BATCH)


def apply_event(buf, ev, layout="env"):
    import torch
    t = lambda x: torch.as_tensor(x, device=buf.device)
    if ev[0] == "start":
        buf.start(picture(ev[1], buf.device, layout), mask=None if ev[2] is None else t(ev[2]))
    else:
        o = ev[2]
        info = {"final_observation": picture(o["final_img"], buf.device, layout)}
        buf.add(t(ev[1]), picture(o["img"], buf.device, layout), t(o["reward"]), t(o["terminated"]), t(o["truncated"]), info)


def make_buffer(C, S, n=N, A=A, K=K, Tm=TM, seed=SEED, guard_rows=2):
    from mycobotgym_amd import ImageReplayBuffer
    buf = ImageReplayBuffer(capacity=K, seed=seed, num_envs=n, channels=C, image_size=S, act_dim=A, max_episode_steps=Tm, guard_rows=guard_rows)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(GUARD)
    return buf


def guards_intact(buf):
    pairs = buf.guards()
    assert set(pairs) == set(ARRAYS)
    return all(g.numel() > 0 and bool((g == GUARD).all()) for pair in pairs.values() for g in pair)


def batch_arrays(b):
    o = {"pix": b.observations, "next_pix": b.next_observations, "action": b.actions, "reward": b.rewards, "done": b.dones, "index": b.index}
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_state_equals(buf, snap):
    sd = buf.state_dict()
    R, F = buf.capacity + 1, -(-buf.capacity // buf.max_episode_steps) + 1
    px = sd["pixels"].cpu().numpy()
    assert px.dtype == np.uint8 and px.shape == snap["pixels"].shape == (R, buf.num_envs, buf.row_bytes)
    assert px.tobytes() == snap["pixels"].tobytes()                      # padding included
    view = buf.pixels()
    assert tuple(view.shape) == (R, buf.num_envs, buf.channels, buf.image_size, buf.image_size)
    assert np.array_equal(view.cpu().numpy().reshape(R, buf.num_envs, -1), snap["pixels"][:, :, :buf.picture_bytes])
    fin = sd["finals"].cpu().numpy()
    assert fin.shape == snap["finals"].shape == (F, buf.num_envs, buf.row_bytes) and fin.tobytes() == snap["finals"].tobytes()
    ft = sd["final_time"].cpu().numpy()
    assert ft.dtype == np.int64 and np.array_equal(ft, snap["final_time"])
    got = buf.records().cpu().numpy().reshape(R, buf.num_envs, -1).view(record_dtype(buf.act_dim))[..., 0]
    assert got.tobytes() == snap["records"].tobytes()
    assert buf.n_written == snap["n"]


def assert_batch_equals(got, want, normalize):
    suffix = "_f32" if normalize else ""
    assert got["index"].dtype == np.int32 and np.array_equal(got["index"], want["index"])
    for name in ("pix", "next_pix"):
        w = want[name + suffix]
        assert got[name].dtype == w.dtype and got[name].shape == w.shape, name
        assert np.array_equal(bits(got[name]), bits(w)) if normalize else np.array_equal(got[name], w), name
    for name in ("action", "reward", "done"):
        assert got[name].dtype == np.float32 and got[name].shape == want[name].shape, name
        assert np.array_equal(bits(got[name]), bits(want[name])), name


def assert_samples_equal(buf, snap):
    """Both forms of a batch (normalised: the rule's call 2 i, uint8: call 2 i + 1), never synchronising, then the two counters."""
    for want, normalize in zip(snap["batches"], (True, False)):
        got = batch_arrays(buf.sample(len(want["draws"]), normalize=normalize, check=False))
        assert_batch_equals(got, want, normalize)
    assert buf.counters() == {"sample_give_ups": snap["give_ups"], "finals_overwritten": snap["lost"]}


def run_against_rule(C, S, layout, n=N, A=A, K=K, Tm=TM):
    snaps = rule_snapshots(C, S, n, STEPS, A, K, Tm)
    buf = make_buffer(C, S, n, A, K, Tm)
    done = 0
    for ev in synthetic_events(C, S, n, STEPS, A, Tm):
        apply_event(buf, ev, layout)
        if ev[0] == "add" and buf.n_written in SNAP_AFTER:
            assert_state_equals(buf, snaps[done])
            assert_samples_equal(buf, snaps[done])
            assert buf.n_sampled == 2 * (done + 1)
            assert guards_intact(buf)
            done += 1
    assert done == len(SNAP_AFTER) and guards_intact(buf)
    return snaps


def census(snaps):
    b = [x for s in snaps for x in s["batches"]]
    flags, draws = np.concatenate([x["flags"] for x in b]), np.concatenate([x["draws"] for x in b])
    return {"samples": len(draws), "give_ups": int((draws > MAX_DRAWS).sum()), "timeout": int(((flags & TIMEOUT) != 0).sum()),
            "terminated": int(((flags & TERMINATED) != 0).sum()), "more_than_one_draw": int(((draws > 1) & (draws <= MAX_DRAWS)).sum()),
            "from_finals": int(sum((x["index"][:, 2] == 1).sum() for x in b)), "lost": snaps[-1]["lost"]}


SHAPES = [(2, 5, "env"), (2, 5, "contiguous"), (2, 6, "env"), (3, 20, "env"), (3, 20, "contiguous"), (3, 20, "offset4"), (1, 64, "env")]


@pytest.mark.parametrize("C,S,layout", SHAPES)
def test_synthetic_events_match_the_rule(built, C, S, layout):
    """30 steps with masked starts of five environments before steps 3 and 17: after steps 1, 4, 12, 13 and 30 the pixels with their
    padding, the final pictures, their stamps, the records and every output of two batches of 101 (float32 and uint8 pictures) equal
    the rule's byte for byte, the counters the rule's counts, and the guard rows around every array are intact."""
    snaps = rule_snapshots(C, S)
    c = census(snaps)          # conditions of the inputs, settled on the rule before the GPU is touched
    print(f"{C} x {S} x {S}: {c}")
    assert c["give_ups"] == 0 and c["timeout"] >= 10 and c["terminated"] >= 10 and c["more_than_one_draw"] >= 1 and c["lost"] == 0
    assert c["from_finals"] == c["timeout"]
    ev = [e[2] for e in synthetic_events(C, S) if e[0] == "add"]
    assert sum(int((e["truncated"] & e["terminated"]).sum()) for e in ev) >= 3          # the engine's other form occurs
    assert all((e["img"] != e["final_img"]).any(axis=(1, 2, 3)).all() for e in ev)
    assert [s["n"] for s in snaps] == list(SNAP_AFTER) and snaps[-1]["n"] > 2 * (K + 1)
    run_against_rule(C, S, layout)
    seen = np.unique(np.concatenate([b["pix"].reshape(-1) for s in snaps for b in s["batches"]]))
    if C * S * S >= 1200:
        assert len(seen) == 256              # every byte value went through the division


def test_a_record_of_exactly_16_bytes(built):
    """A = 2: action[2], reward, flags and no padding; A = 7 above is 9 words and 12 bytes of zeros."""
    assert record_dtype(2).itemsize == 16 and record_dtype(2)["pad"].shape == (0,) and record_dtype(7)["pad"].shape == (12,)
    run_against_rule(2, 5, "env", A=2)


@pytest.mark.parametrize("K_,n", [(1, 1), (TM - 1, N)])
def test_degenerate_capacities(built, K_, n):
    """(K, N) = (1, 1): two rows, F = 2, every sample is the newest transition.  K = Tm - 1: F = 2, a window shorter than an episode."""
    snaps = run_against_rule(2, 5, "env", n=n, K=K_)
    print(f"(K, N) = ({K_}, {n}): {census(snaps)}")


def test_stamp_mismatch(built):
    """Two timeouts of environment 0 inside one block of Tm (times 5 and 7: what the engine never does, and set_state(elapsed=...)
    can).  The older transition comes out with done = 1 and the ring's row as successor; counters[1] equals the rule's count; no
    output carries the other episode's final picture."""
    import torch
    n, C, S, Tm, K_ = 4, 1, 8, 5, 8
    rng = np.random.default_rng(1)
    pic = lambda: rng.integers(0, 200, (n, C, S, S), dtype=np.uint8)
    final = {5: np.full((n, C, S, S), 250, np.uint8), 7: np.full((n, C, S, S), 251, np.uint8)}          # no other picture has these bytes
    events = [("start", pic(), None)]
    for a in range(9):
        trunc = np.zeros(n, bool)
        trunc[0] = a in final
        events.append(("add", rng.uniform(-1, 1, (n, A)).astype(np.float32),
                       {"img": pic(), "final_img": final.get(a, pic()), "reward": rng.normal(size=n), "terminated": np.zeros(n, bool), "truncated": trunc}))
    snap = run_rule(events, n, C, S, A, K_, Tm, (9,), 256)[0]
    b = snap["batches"][1]
    older, newer = (b["time"] == 5) & (b["index"][:, 1] == 0), (b["time"] == 7) & (b["index"][:, 1] == 0)
    print(f"stamp mismatch: {int(older.sum())} samples of the older timeout, {int(newer.sum())} of the newer, lost {snap['lost']}")
    assert older.sum() >= 3 and newer.sum() >= 3 and snap["lost"] >= older.sum()
    assert (b["done"][older] == 1).all() and (b["index"][older, 2] == 0).all() and (b["done"][newer] == 0).all() and (b["index"][newer, 2] == 1).all()
    buf = make_buffer(C, S, n, A, K_, Tm)
    for ev in events:
        apply_event(buf, ev)
    assert_state_equals(buf, snap)
    assert_samples_equal(buf, snap)          # counters[1] == the rule's count among them
    buf.n_sampled = 1
    got = batch_arrays(buf.sample(256, normalize=False, check=False))
    ring = buf.pixels().cpu().numpy()
    assert (got["next_pix"][older] == ring[6 % (K_ + 1), 0]).all() and (got["done"][older] == 1).all()
    assert not (got["next_pix"][~newer] == 251).any() and not (got["next_pix"] == 250).any() and (got["next_pix"][newer] == 251).all()
    assert not (got["pix"] >= 250).any()
    assert guards_intact(buf)
    assert torch.equal(buf.state_dict()["final_time"][1], torch.tensor([7, -1, -1, -1], device=buf.device))


def test_give_up(built):
    """One add, then a masked start of every environment: every stored transition has lost its next picture."""
    import torch
    from mycobotgym_amd._abi import McgError
    C, S, B = 2, 5, 37
    buf = make_buffer(C, S)
    events = synthetic_events(C, S)
    with pytest.raises(McgError, match="empty"):
        buf.sample(B)
    apply_event(buf, events[0])
    with pytest.raises(McgError, match="empty"):
        buf.sample(B, check=False)
    no = torch.zeros(N, dtype=torch.bool, device=buf.device)
    o = events[1][2]
    buf.add(torch.as_tensor(events[1][1], device=buf.device), picture(o["img"], buf.device, "env"), torch.as_tensor(o["reward"], device=buf.device),
            no, no, {"final_observation": picture(o["final_img"], buf.device, "env")})
    assert buf.sample(B).index.shape == (B, 3)          # nothing lost yet
    buf.start(picture(events[0][1], buf.device, "env"), mask=~no)
    flags = buf.records().cpu().numpy().reshape(K + 1, N, -1).view(record_dtype(A))[..., 0]["flags"]
    assert (flags[0] == NO_NEXT).all() and not flags[1:].any()
    before = buf.counters()["sample_give_ups"]
    for normalize in (True, False):
        got = batch_arrays(buf.sample(B, normalize=normalize, check=False))
        assert (got["index"] == -1).all()
        for name in ("pix", "next_pix", "action", "reward", "done"):
            assert not got[name].any(), name
    assert buf.counters()["sample_give_ups"] == before + 2 * B
    with pytest.raises(RuntimeError, match=f"{B} of {B} samples found no valid transition"):
        buf.sample(B)
    assert guards_intact(buf)


def test_checkpoint(built):
    """state_dict() in mid-ring (14 steps: the ring has wrapped once) into a new buffer: the rest of the run and the next samples are
    identical, and they are the rule's."""
    import torch
    C, S = 3, 20
    events = synthetic_events(C, S)
    cut = [i for i, ev in enumerate(events) if ev[0] == "add"][13] + 1
    buf = make_buffer(C, S)
    for ev in events[:cut]:
        apply_event(buf, ev)
        if ev[0] == "add" and buf.n_written in SNAP_AFTER:
            buf.sample(BATCH, check=False); buf.sample(BATCH, normalize=False, check=False)
    sd = buf.state_dict()
    assert {k: v for k, v in sd.items() if not torch.is_tensor(v)} == {"n_written": 14, "n_sampled": 8, "seed": SEED}
    assert len(sd) == 8
    other = make_buffer(C, S, seed=99)
    other.load_state_dict(sd)
    for ev in events[cut:]:
        apply_event(buf, ev); apply_event(other, ev)
    a, b = buf.state_dict(), other.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    x, y = batch_arrays(buf.sample(BATCH)), batch_arrays(other.sample(BATCH))
    for k in x:
        assert np.array_equal(bits(x[k]), bits(y[k])), k
    want = rule_snapshots(C, S)[-1]
    assert_state_equals(other, want)
    assert_batch_equals(y, want["batches"][0], True)
    assert guards_intact(other)


def test_a_picture_with_strided_planes_is_copied_once(built):
    """A picture whose [S, S] planes are not contiguous (every second column of a wider one) gives what its contiguous copy gives."""
    import torch
    C, S = 2, 5
    a, b = make_buffer(C, S), make_buffer(C, S)
    gen = torch.Generator(device="cpu"); gen.manual_seed(0)
    wide = torch.randint(0, 256, (3, N, C, S, 2 * S), generator=gen, dtype=torch.uint8).to(a.device)
    z = torch.zeros(N, device=a.device)
    trunc = torch.ones(N, dtype=torch.bool, device=a.device)
    for buf, f in ((a, lambda x: x), (b, lambda x: x.contiguous())):
        buf.start(f(wide[0, ..., ::2]))
        buf.add(torch.zeros(N, A, device=a.device), f(wide[1, ..., ::2]), z, ~trunc, trunc, {"final_observation": f(wide[2, ..., ::2])})
    sa, sb = a.state_dict(), b.state_dict()
    for k in ARRAYS:
        assert torch.equal(sa[k], sb[k]), k
    assert bool((a.pixels()[0] == wide[0, ..., ::2]).all()) and bool((a.pixels()[1] == wide[1, ..., ::2]).all())
    assert bool((a.state_dict()["finals"][0, :, :C * S * S] == wide[2, ..., ::2].reshape(N, -1)).all())


def test_class_refusals(built):
    from mycobotgym_amd import HerBuffer, ImageReplayBuffer, make
    v0 = make("MyCobotReach-Dense-joint-v0", num_envs=2)
    with pytest.raises(ValueError, match="HerBuffer is the buffer for them"):
        ImageReplayBuffer(v0, capacity=4)
    v0.close()
    v1 = make("MyCobotReach-Dense-joint-v1", num_envs=2, image_size=16, max_episode_steps=9)
    with pytest.raises(ValueError, match="the -v1 image ids carry no goals in their observation"):
        HerBuffer(v1)
    buf = ImageReplayBuffer(v1, capacity=4)
    assert (buf.num_envs, buf.channels, buf.image_size, buf.act_dim, buf.max_episode_steps) == (2, 1, 16, v1.action_dim, 9)
    assert buf.nbytes >= (5 + 2) * 2 * 256
    with pytest.raises(ValueError, match="needs envs= or"):
        ImageReplayBuffer(capacity=4, num_envs=3)
    v1.close()


def test_with_the_real_engine(built):
    """45 steps of 40 environments (time limit 7), two cameras at 16 x 16, under a fixed linear policy on the flattened picture, into a
    buffer of K = 20.  Every sampled transition's picture, successor, action, reward and done equal the host log of what reset / step
    returned: the successor is info["final_observation"] where the time limit ended the episode and the step's picture otherwise; the
    engine's state is what it is without a buffer."""
    import torch
    from mycobotgym_amd import ImageReplayBuffer, make
    steps, K_, Tm, env_id = 45, 20, 7, "MyCobotReach-Dense-joint-v1"
    kw = dict(num_envs=N, max_episode_steps=Tm, image_size=16, camera=("sideview", "gripper_camera_rgb"), seed=3)
    envs, twin = make(env_id, **kw), make(env_id, **kw)
    buf = ImageReplayBuffer(envs, capacity=K_, seed=SEED, guard_rows=1)
    C, S, Aa = 2, 16, envs.action_dim
    assert (buf.num_envs, buf.channels, buf.image_size, buf.act_dim, buf.max_episode_steps) == (N, C, S, Aa, Tm)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(GUARD)
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    W = (torch.randn(C * S * S, Aa, generator=gen) * 0.5).to(envs.device)
    policy = lambda img: torch.tanh((img.reshape(N, -1).float() / 255 - 0.5) @ W).contiguous()
    host = lambda x: x.cpu().numpy()
    img, _ = envs.reset(seed=0)
    twin.reset(seed=0)
    assert not img.is_contiguous()          # the environment's own layout goes in as it is
    buf.start(img)
    prev, log, timeouts, differ = host(img), [], 0, 0
    for t in range(steps):
        a = policy(img)
        img, r, term, trunc, info = envs.step(a)
        buf.add(a, img, r, term, trunc, info)
        twin.step(a)
        s = {"prev": prev, "action": host(a), "reward": host(r.double()).astype(np.float32), "terminated": host(term), "truncated": host(trunc),
             "img": host(img), "final": host(info["final_observation"])}
        log.append(s)
        prev = s["img"]
        timeout = s["truncated"] & ~s["terminated"]
        timeouts += int(timeout.sum())
        differ += int((s["final"][timeout] != s["img"][timeout]).any(axis=(1, 2, 3)).sum())
        if t + 1 in (10, 45):
            n = t + 1
            W_ = min(n, K_)
            time_of_row = {a_ % (K_ + 1): a_ for a_ in range(n - W_, n)}
            raw = batch_arrays(buf.sample(512, normalize=False))
            buf.n_sampled -= 1
            norm = batch_arrays(buf.sample(512))
            assert np.array_equal(raw["index"], norm["index"])
            for name in ("pix", "next_pix"):
                assert np.array_equal(bits(norm[name]), bits(raw[name].astype(np.float32) / np.float32(255))), name
            sampled_timeouts = 0
            for j, (row, e, src) in enumerate(raw["index"].tolist()):
                w = log[time_of_row[row]]
                timeout = bool(w["truncated"][e]) and not bool(w["terminated"][e])
                sampled_timeouts += timeout
                assert src == int(timeout), (j, "source")
                assert np.array_equal(raw["pix"][j], w["prev"][e]), (j, "picture")
                assert np.array_equal(raw["next_pix"][j], w["final"][e] if timeout else w["img"][e]), (j, "successor")
                assert np.array_equal(bits(raw["action"][j]), bits(w["action"][e])), (j, "action")
                assert bits(raw["reward"][j])[0] == bits(w["reward"][e:e + 1])[0], (j, "reward")
                assert raw["done"][j, 0] == float(w["terminated"][e]), (j, "done")
            print(f"after {n} steps: {sampled_timeouts} of 512 samples are time-limit ends")
            if n == 45:
                assert sampled_timeouts >= 10
    s1, s2 = envs.get_state(), twin.get_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    print(f"{env_id}: {timeouts} time-limit ends, {differ} of them with a final picture other than the post-reset one")
    assert timeouts >= N
    # A condition of the inputs, not of the buffer (tests/test_gpu_rollout_img.py has the same one): the check above can tell the
    # post-reset picture from final_observation only where the two differ.
    assert differ >= timeouts // 2
    assert buf.counters() == {"sample_give_ups": 0, "finals_overwritten": 0} and guards_intact(buf)
    envs.close(); twin.close()
