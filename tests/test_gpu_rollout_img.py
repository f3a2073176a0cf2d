"""The device-resident picture rollout buffer (mcg_rollout_img_*, mycobotgym_amd/rollout_img.py) against the rule restated in
tests/indep_rollout_img.py, and on the real engine.  Shapes: 40 environments, 7 steps (M = 280: the permutation walks), A = 7 (a record of
8 words and no padding; A = 2 in one case: 3 words and 4 bytes of zeros), minibatches of 64 with a short last one, and pictures at
which the kernels take each of their paths:

    C = 2, S = 5    P = 50 + 14: planes at odd addresses (byte loads), byte stores in the gather, less than one pass of a wave
    C = 2, S = 6    P = 72 + 8:  planes and rows at multiples of 4 only (4-byte loads and stores)
    C = 3, S = 20   P = 1200:    16-byte loads and stores, one full pass of 64 lanes x 16 bytes and a partial one
    C = 1, S = 64   P = 4096:    the registered shape, several passes
"""
import functools

import numpy as np
import pytest

from tests.common import bits
from tests.indep_rollout import PERM_SEED
from tests.indep_rollout_img import ImageRollout, record_dtype

pytestmark = pytest.mark.gpu

N, A, T, MAX_STEPS = 40, 7, 7, 7
GAMMA, LAMBDA = 0.99, 0.95
RESTART_AT, RESTARTED = 3, 5
FIELDS = ("action", "old_value", "old_log_prob", "advantage", "returns")
PLANES = ("reward", "value", "episode_start", "advantage", "returns")


@functools.lru_cache(maxsize=None)
def synthetic_events(C, S, n=N, steps=T, rollouts=2, restart_at=RESTART_AT, poison=False, A=A):
    """Step outputs from default_rng(0): ("start", img, mask), ("add", actions, values, log_probs, final_values, out) and
    ("finish", last_values) events, `rollouts` rollouts of `steps` steps.  Pictures are random bytes; out["final_img"] differs from the
    post-reset picture (the buffer must not read it); episode lengths are uniform in 1..7; `terminated` on a random half of the ends;
    before step `restart_at` a masked start restarts five environments.  poison: the values of environment 3 at step 2 and of
    environment 17 at step 4 are inf and nan."""
    rng = np.random.default_rng(0)
    pic = lambda: rng.integers(0, 256, (n, C, S, S), dtype=np.uint8)
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    events = [("start", pic(), None)]
    left = rng.integers(1, MAX_STEPS + 1, n)             # steps the episode in flight still has
    for i in range(rollouts * steps):
        if i == restart_at:
            mask = np.zeros(n, dtype=bool)
            mask[rng.choice(n, min(RESTARTED, n), replace=False)] = True
            events.append(("start", pic(), mask))
            left[mask] = rng.integers(1, MAX_STEPS + 1, int(mask.sum()))
        left -= 1
        done = left == 0
        terminated = done & (rng.random(n) < 0.5)
        truncated = done & (~terminated | (rng.random(n) < 0.5))         # the engine sets truncated with terminated; both forms occur
        out = {"img": pic(), "reward": rng.normal(size=n), "terminated": terminated, "truncated": truncated, "final_img": pic()}
        values = f(n)
        if poison and i == 2:
            values[3] = np.inf
        if poison and i == 4:
            values[17] = np.nan
        events.append(("add", rng.uniform(-1, 1, (n, A)).astype(np.float32), values, f(n), f(n), out))
        left[done] = rng.integers(1, MAX_STEPS + 1, int(done.sum()))
        if (i + 1) % steps == 0:
            events.append(("finish", f(n)))
    return tuple(events)


def minibatches(M, batch):
    return [(first, min(batch, M - first)) for first in range(0, M, batch)]


@functools.lru_cache(maxsize=None)
def rule_snapshots(C, S, n=N, steps=T, rollouts=2, restart_at=RESTART_AT, with_final_values=True, batch=64, poison=False, A=A):
    """The rule on the events: after every finish its pixels, records, planes, last_start and the epoch's minibatches.  Computed once
    per shape, shared between the input layouts, not modified."""
    R = ImageRollout(n, C, S, A, steps, GAMMA, LAMBDA)
    snaps = []
    for ev in synthetic_events(C, S, n, steps, rollouts, restart_at, poison, A):
        if ev[0] == "start":
            R.start(ev[1], ev[2])
        elif ev[0] == "add":
            o = ev[5]
            R.add(ev[1], ev[2], ev[3], o["img"], o["reward"], o["terminated"], o["truncated"], final_values=ev[4] if with_final_values else None)
        else:
            R.finish(ev[1])
            epoch = len(snaps)
            snaps.append({"pixels": R.pixels(), "records": R.records(), "planes": R.planes(), "last_start": R.last_start(),
                          "batches": [R.gather(PERM_SEED, epoch, first, count) for first, count in minibatches(steps * n, batch)]})
            R.reset()
    return tuple(snaps)


def picture(x, device, layout):
    """A host picture [N, C, S, S] as a device tensor in one of the layouts the buffer takes without a copy: "env" -- the [N, C, S, S]
    view of a contiguous [C, N, S, S] buffer, as MyCobotImgVecEnv holds it; "contiguous"; "offset4" -- contiguous, its base address
    4 bytes past an aligned one."""
    import torch
    if layout == "env":
        t = torch.as_tensor(np.ascontiguousarray(x.transpose(1, 0, 2, 3))).to(device).permute(1, 0, 2, 3)
        assert not t.is_contiguous() or x.shape[1] == 1 or x.shape[0] == 1
        return t
    if layout == "contiguous":
        return torch.as_tensor(x).to(device)
    flat = torch.zeros(x.size + 4, dtype=torch.uint8, device=device)
    flat[4:] = torch.as_tensor(x.reshape(-1)).to(device)
    t = flat[4:].view(*x.shape)
    assert t.data_ptr() % 16 == 4
    return t


def apply_event(buf, ev, with_final_values=True, layout="env"):
    import torch
    t = lambda x: torch.as_tensor(x, device=buf.device)
    if ev[0] == "start":
        buf.start(picture(ev[1], buf.device, layout), mask=None if ev[2] is None else t(ev[2]))
    elif ev[0] == "add":
        o = ev[5]
        info = {"final_observation": picture(o["final_img"], buf.device, layout)}
        buf.add(t(ev[1]), t(ev[2]), t(ev[3]), picture(o["img"], buf.device, layout), t(o["reward"]), t(o["terminated"]), t(o["truncated"]), info,
                final_values=t(ev[4]) if with_final_values else None)
    else:
        buf.finish(t(ev[1]))


def make_buffer(C, S, n=N, steps=T, A=A, **kw):
    from mycobotgym_amd import ImageRolloutBuffer
    buf = ImageRolloutBuffer(n_steps=steps, gamma=GAMMA, gae_lambda=LAMBDA, seed=PERM_SEED, num_envs=n, channels=C, image_size=S, act_dim=A, **kw)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(0xA5)
    return buf


def guards_intact(buf):
    pairs = buf.guards()
    assert set(pairs) == {"pixels", "records", *PLANES}
    return all(bool((g == 0xA5).all()) for pair in pairs.values() for g in pair)


def batch_arrays(b):
    o = {"pix": b.observations, "action": b.actions, "old_value": b.old_values, "old_log_prob": b.old_log_prob, "advantage": b.advantages,
         "returns": b.returns, "index": b.index}
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_state_equals(buf, snap, skip_envs=()):
    keep = np.array([e not in skip_envs for e in range(buf.num_envs)])
    sd = buf.state_dict()
    px = sd["pixels"].cpu().numpy()
    assert px.dtype == np.uint8 and px.shape == snap["pixels"].shape == (buf.n_steps + 1, buf.num_envs, buf.row_bytes)
    assert px.tobytes() == snap["pixels"].tobytes()                      # padding included
    view = buf.pixels()
    assert tuple(view.shape) == (buf.n_steps + 1, buf.num_envs, buf.channels, buf.image_size, buf.image_size)
    assert np.array_equal(view.cpu().numpy().reshape(buf.n_steps + 1, buf.num_envs, -1), snap["pixels"][:, :, :buf.picture_bytes])
    got = buf.records().cpu().numpy().reshape(buf.n_steps, buf.num_envs, -1).view(record_dtype(buf.act_dim))[..., 0]
    assert got.tobytes() == snap["records"].tobytes()
    P = {k: v.cpu().numpy() for k, v in buf.planes().items()}
    for name in PLANES:
        assert P[name].dtype == snap["planes"][name].dtype and P[name].shape == (buf.n_steps, buf.num_envs), name
        assert np.array_equal(bits(P[name])[:, keep], bits(snap["planes"][name])[:, keep]), name
    assert np.array_equal(sd["last_start"].cpu().numpy(), snap["last_start"])
    return P


def assert_epoch_equals(buf, snap, batch, skip_fields=()):
    """Both forms of the epoch's minibatches: normalised, and the same epoch's uint8 pictures through gather()."""
    M = buf.n_steps * buf.num_envs
    epoch = buf.epoch
    got = [batch_arrays(mb) for mb in buf.get(batch, normalize=True)]
    raw = [batch_arrays(buf.gather(epoch, first, count, normalize=False)) for first, count in minibatches(M, batch)]
    assert [len(g["index"]) for g in got] == [c for _, c in minibatches(M, batch)] == [len(w["index"]) for w in snap["batches"]]
    for g, r, want in zip(got, raw, snap["batches"]):
        assert g["index"].dtype == np.int32 and np.array_equal(g["index"], want["index"]) and np.array_equal(r["index"], want["index"])
        assert g["pix"].dtype == np.float32 and g["pix"].shape == want["pix_f32"].shape
        assert np.array_equal(bits(g["pix"]), bits(want["pix_f32"]))
        assert r["pix"].dtype == np.uint8 and r["pix"].shape == want["pix"].shape and np.array_equal(r["pix"], want["pix"])
        for name in FIELDS:
            if name in skip_fields:
                continue
            assert g[name].dtype == np.float32 and g[name].shape == want[name].shape, name
            assert np.array_equal(bits(g[name]), bits(want[name])) and np.array_equal(bits(r[name]), bits(want[name])), name
    assert sorted(np.concatenate([g["index"] for g in got]).tolist()) == list(range(M))
    return got


def run_against_rule(C, S, layout, n=N, steps=T, rollouts=2, restart_at=RESTART_AT, with_final_values=True, batch=64, A=A):
    snaps = rule_snapshots(C, S, n, steps, rollouts, restart_at, with_final_values, batch, False, A)
    # the walk's length is a condition of the inputs, settled before the GPU is touched
    longest = max(int(b["passes"].max()) for s in snaps for b in s["batches"])
    print(f"(T, N) = ({steps}, {n}): longest walk {longest} passes")
    assert longest <= 64
    buf = make_buffer(C, S, n, steps, A, guard_rows=2)
    done = 0
    for ev in synthetic_events(C, S, n, steps, rollouts, restart_at, False, A):
        apply_event(buf, ev, with_final_values, layout)
        if ev[0] == "finish":
            assert_state_equals(buf, snaps[done])
            assert_epoch_equals(buf, snaps[done], batch)
            assert buf.epoch == done + 1
            assert guards_intact(buf)
            buf.reset()
            done += 1
    assert done == rollouts and guards_intact(buf)
    return snaps


SHAPES = [(2, 5, "env"), (2, 5, "contiguous"), (2, 6, "env"), (3, 20, "env"), (3, 20, "contiguous"), (3, 20, "offset4"), (1, 64, "env")]


@pytest.mark.parametrize("C,S,layout", SHAPES)
def test_synthetic_events_match_the_rule(built, C, S, layout):
    """Two rollouts of 7 steps with reset() between them (the last picture and last_start carry over), a masked start at step 3: after
    each, the pixels with their padding, the records, the five planes, last_start and every output of the five minibatches of get(64)
    (four of 64, one of 24; float32 and uint8 pictures) equal the rule's byte for byte; the epoch's indices are 0 .. 279 once each; the
    guard rows are intact."""
    snaps = run_against_rule(C, S, layout)
    assert [len(b["index"]) for b in snaps[0]["batches"]] == [64, 64, 64, 64, 24]
    ev = [e for e in synthetic_events(C, S) if e[0] == "add"]
    boot = sum(int((e[5]["truncated"] & ~e[5]["terminated"]).sum()) for e in ev)
    both = sum(int((e[5]["truncated"] & e[5]["terminated"]).sum()) for e in ev)
    assert boot >= 10 and both >= 5          # the bootstrap and its exception both occur
    assert any(s["planes"]["episode_start"][0].sum() not in (0, N) for s in snaps[1:])          # last_start carried over, mixed
    assert not np.array_equal(snaps[0]["pixels"][0], snaps[1]["pixels"][0])                    # and so did the last picture
    assert np.array_equal(snaps[0]["pixels"][T], snaps[1]["pixels"][0])
    seen = np.unique(np.concatenate([b["pix"].reshape(-1) for b in snaps[0]["batches"]]))
    if C * S * S * N * T >= 100000:
        assert len(seen) == 256              # every byte value went through the division


def test_without_final_values_and_a_padded_record(built):
    """No bootstrap (final_values=None), and A = 2: a record of 3 words and 4 bytes of zeros."""
    assert record_dtype(2).itemsize == 16 and record_dtype(2)["pad"].shape == (4,)
    snaps = run_against_rule(2, 5, "env", with_final_values=False, A=2)
    other = rule_snapshots(2, 5, N, T, 2, RESTART_AT, True, 64, False, 2)
    assert not np.array_equal(snaps[0]["planes"]["reward"], other[0]["planes"]["reward"])


@pytest.mark.parametrize("steps,n", [(4, 64), (1, 1)])
def test_no_walk_and_degenerate_shapes(built, steps, n):
    """(4, 64): M = 256 = 2^b, every position lands at once.  (1, 1): b = 2, one transition, three of four values walk on."""
    snaps = run_against_rule(2, 5, "env", n=n, steps=steps, restart_at=None)
    if steps * n == 256:
        assert all(int(b["passes"].max()) == 1 for s in snaps for b in s["batches"])


@pytest.mark.parametrize("steps,n", [(7, 40), (4, 64), (1, 1)])
def test_index_agrees_with_the_state_buffer(built, steps, n):
    """Equal (seed, epoch, T, N): an ImageRolloutBuffer and a RolloutBuffer (of a dummy obs_dim) yield the same `index`, minibatch by
    minibatch, over three epochs and one beyond 2^32."""
    from mycobotgym_amd import RolloutBuffer
    img = make_buffer(2, 5, n, steps)
    state = RolloutBuffer(n_steps=steps, gamma=GAMMA, gae_lambda=LAMBDA, seed=PERM_SEED, num_envs=n, obs_dim=3, act_dim=A)
    M = steps * n
    for epoch in (0, 1, 2, 2 ** 32 + 1):
        seen = []
        for first, count in minibatches(M, 64):
            a = img.gather(epoch, first, count, normalize=False).index.cpu().numpy()
            b = state.gather(epoch, first, count).index.cpu().numpy()
            assert np.array_equal(a, b), (epoch, first)
            seen += a.tolist()
        assert sorted(seen) == list(range(M))


def test_non_finite_policy_outputs(built):
    """A value of inf (environment 3, step 2) and of nan (environment 17, step 4): every call returns, the other environments' planes
    and samples equal the rule's, the pixels and records are untouched by it, the guard rows are intact."""
    import torch
    C, S = 2, 5
    snap = rule_snapshots(C, S, N, T, 1, RESTART_AT, True, 64, True)[0]
    buf = make_buffer(C, S, guard_rows=2)
    for ev in synthetic_events(C, S, N, T, 1, RESTART_AT, True):
        apply_event(buf, ev)
    torch.cuda.synchronize()
    P = assert_state_equals(buf, snap, skip_envs=(3, 17))
    for e, t0 in ((3, 2), (17, 4)):
        for name in ("advantage", "returns"):
            assert not np.isfinite(P[name][:t0 + 1, e]).any(), (name, e)
            assert np.array_equal(np.isfinite(P[name][:, e]), np.isfinite(snap["planes"][name][:, e])), (name, e)
        assert np.isfinite(P["advantage"][t0 + 1:, e]).all()
    got = assert_epoch_equals(buf, snap, 64, skip_fields=("old_value", "advantage", "returns"))
    for g, want in zip(got, snap["batches"]):
        clean = ~np.isin(want["index"] // T, (3, 17))
        for name in ("old_value", "advantage", "returns"):
            assert np.array_equal(bits(g[name])[clean], bits(want[name])[clean]), name
            assert np.array_equal(np.isfinite(g[name]), np.isfinite(want[name])), name
    torch.cuda.synchronize()
    assert guards_intact(buf)


def test_order_of_calls_is_enforced(built):
    C, S = 2, 5
    buf = make_buffer(C, S)
    events = synthetic_events(C, S)
    with pytest.raises(ValueError, match="0 of 7 steps"):
        buf.finish(np.zeros(N, np.float32))
    for ev in events[:4]:
        apply_event(buf, ev)
    with pytest.raises(ValueError, match="3 of 7 steps"):
        buf.get(64)
    adds = [ev for ev in events[4:] if ev[0] == "add"]
    for ev in adds[:4]:
        apply_event(buf, ev)
    assert buf.full and buf.pos == T
    with pytest.raises(ValueError, match=r"finish\(last_values\) comes first"):
        buf.get(64)
    with pytest.raises(ValueError, match="full"):
        apply_event(buf, adds[4])
    buf.finish(np.zeros(N, np.float32))
    assert sum(len(mb.index) for mb in buf.get()) == T * N and buf.epoch == 1
    with pytest.raises(ValueError, match="batch_size must be >= 1"):
        buf.get(0)
    from mycobotgym_amd import ImageRolloutBuffer
    with pytest.raises(ValueError, match="needs envs= or"):
        ImageRolloutBuffer(n_steps=4, num_envs=3)
    import torch
    with pytest.raises(ValueError, match="uint8"):
        buf.start(torch.zeros(N, C, S, S, device=buf.device))
    with pytest.raises(ValueError, match="expected shape"):
        buf.start(torch.zeros(N, C, S, S + 1, dtype=torch.uint8, device=buf.device))


def test_a_picture_with_strided_planes_is_copied_once(built):
    """A picture whose [S, S] planes are not contiguous (every second column of a wider one) gives what its contiguous copy gives."""
    import torch
    C, S = 2, 5
    a, b = make_buffer(C, S), make_buffer(C, S)
    gen = torch.Generator(device="cpu"); gen.manual_seed(0)
    wide = torch.randint(0, 256, (N, C, S, 2 * S), generator=gen, dtype=torch.uint8).to(a.device)
    a.start(wide[..., ::2]); b.start(wide[..., ::2].contiguous())
    assert torch.equal(a.pixels(), b.pixels()) and bool((a.pixels()[0] == wide[..., ::2]).all())


def test_class_refusals(built):
    from mycobotgym_amd import HerBuffer, ImageRolloutBuffer, RolloutBuffer, make
    v0 = make("MyCobotReach-Dense-joint-v0", num_envs=2)
    with pytest.raises(ValueError, match="RolloutBuffer is the buffer for them"):
        ImageRolloutBuffer(v0, n_steps=4)
    v0.close()
    v1 = make("MyCobotReach-Dense-joint-v1", num_envs=2, image_size=16)
    with pytest.raises(ValueError, match="picture records are not supported"):
        RolloutBuffer(v1, n_steps=4)
    with pytest.raises(ValueError, match="the -v1 image ids carry no goals in their observation"):
        HerBuffer(v1)
    buf = ImageRolloutBuffer(v1, n_steps=4)
    assert (buf.num_envs, buf.channels, buf.image_size, buf.act_dim) == (2, 1, 16, v1.action_dim)
    v1.close()


def test_with_the_real_engine(built):
    """Two rollouts of 16 steps of 40 environments (time limit 7), two cameras at 16 x 16, under a fixed linear policy on the flattened
    picture.  Every gathered picture is the host copy of what reset / step returned at its (step, env) -- the row after an episode's
    end the post-reset picture, not final_observation; the reward plane is the recalled bootstrap rule on the host copies; advantages
    and returns equal the rule's bit for bit; the engine's state is what it is without a buffer."""
    import torch
    from mycobotgym_amd import ImageRolloutBuffer, make
    steps, env_id = 16, "MyCobotReach-Dense-joint-v1"
    kw = dict(num_envs=N, max_episode_steps=MAX_STEPS, image_size=16, camera=("sideview", "gripper_camera_rgb"), seed=3)
    envs, twin = make(env_id, **kw), make(env_id, **kw)
    buf = ImageRolloutBuffer(envs, n_steps=steps, gamma=GAMMA, gae_lambda=LAMBDA, seed=PERM_SEED, guard_rows=1)
    C, S, Aa = 2, 16, envs.action_dim
    assert (buf.num_envs, buf.channels, buf.image_size, buf.act_dim) == (N, C, S, Aa)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(0xA5)
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    W = (torch.randn(C * S * S, Aa + 2, generator=gen) * 0.5).to(envs.device)

    def policy(img):        # a fixed linear "policy" on the flattened picture: actions, values, log-probs
        x = (img.reshape(N, -1).float() / 255 - 0.5) @ W
        return torch.tanh(x[:, :Aa]).contiguous(), x[:, Aa].contiguous(), x[:, Aa + 1].contiguous()

    host = lambda x: x.cpu().numpy()
    f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32)
    img, _ = envs.reset(seed=0)
    twin.reset(seed=0)
    assert not img.is_contiguous()          # the environment's own layout goes in as it is
    buf.start(img)
    R = ImageRollout(N, C, S, Aa, steps, GAMMA, LAMBDA)
    R.start(host(img))
    prev, ended, differ = host(img), 0, 0
    for rollout in range(2):
        log = []
        for _ in range(steps):
            a, v, lp = policy(img)
            img, r, term, trunc, info = envs.step(a)
            fv = policy(info["final_observation"])[1]
            buf.add(a, v, lp, img, r, term, trunc, info, final_values=fv)
            twin.step(a)
            s = {"prev": prev, "action": host(a), "value": host(v), "log_prob": host(lp), "reward": host(r.double()), "terminated": host(term),
                 "truncated": host(trunc), "final_values": host(fv), "img": host(img)}
            R.add(s["action"], s["value"], s["log_prob"], s["img"], s["reward"], s["terminated"], s["truncated"], final_values=s["final_values"])
            log.append(s)
            prev = s["img"]
            done = s["truncated"] | s["terminated"]
            ended += int(done.sum())
            differ += int((host(info["final_observation"])[done] != s["img"][done]).any(axis=(1, 2, 3)).sum())
        lv = policy(img)[1]
        buf.finish(lv)
        R.finish(host(lv))
        P = {k: x.cpu().numpy() for k, x in buf.planes().items()}
        for t, s in enumerate(log):          # the reward plane from the host copies, by the recalled rule
            boot = (np.float32(GAMMA) * s["final_values"].astype(np.float32)).astype(np.float32)
            want = np.where(s["truncated"] & ~s["terminated"], f32(s["reward"]) + boot, f32(s["reward"])).astype(np.float32)
            assert np.array_equal(bits(P["reward"][t]), bits(want)), t
            assert np.array_equal(bits(P["value"][t]), bits(s["value"])), t
        ref = R.planes()
        for name in PLANES:
            assert np.array_equal(bits(P[name]), bits(ref[name])), name
        px = buf.pixels().cpu().numpy()
        for t, s in enumerate(log):
            assert np.array_equal(px[t], s["prev"]) and np.array_equal(px[t + 1], s["img"]), t
        seen, epoch = [], buf.epoch
        for k, mb in enumerate(buf.get(256, normalize=False)):
            g = batch_arrays(mb)
            norm = buf.gather(epoch, 256 * k, len(g["index"])).observations.cpu().numpy()
            assert np.array_equal(bits(norm), bits(g["pix"].astype(np.float32) / np.float32(255)))
            for j, i in enumerate(g["index"].tolist()):
                e, t = divmod(i, steps)
                s = log[t]
                assert np.array_equal(g["pix"][j], s["prev"][e]), (i, "picture")
                assert np.array_equal(bits(g["action"][j]), bits(s["action"][e])), (i, "action")
                assert bits(g["old_value"][j:j + 1])[0] == bits(s["value"][e:e + 1])[0], (i, "value")
                assert bits(g["old_log_prob"][j:j + 1])[0] == bits(s["log_prob"][e:e + 1])[0], (i, "log_prob")
                assert bits(g["advantage"][j:j + 1])[0] == bits(ref["advantage"][t, e:e + 1])[0], (i, "advantage")
                assert bits(g["returns"][j:j + 1])[0] == bits(ref["returns"][t, e:e + 1])[0], (i, "returns")
            seen += g["index"].tolist()
        assert sorted(seen) == list(range(steps * N))
        buf.reset(); R.reset()
    s1, s2 = envs.get_state(), twin.get_state()
    for k in s1:
        assert torch.equal(s1[k], s2[k]), k
    print(f"{env_id}: {ended} episodes ended, {differ} of them with a final picture other than the post-reset one")
    assert ended >= N * (2 * steps // MAX_STEPS)          # true by the time limit alone
    # A condition of the inputs, not of the buffer: the check above can tell the post-reset picture from final_observation only where
    # the two differ.  A reset draws a new goal and returns the arm to its initial pose, so they do for any episode in which the arm
    # moved; half of the episodes is asked for, far below what seven steps of a saturated policy give.
    assert differ >= ended // 2
    assert guards_intact(buf)
    envs.close(); twin.close()


def test_checkpoint(built):
    """state_dict() in mid-rollout into a new buffer: the rest of the rollout, finish and the next epoch's minibatches are identical."""
    import torch
    C, S = 3, 20
    events = synthetic_events(C, S)
    cut = [i for i, ev in enumerate(events) if ev[0] == "finish"][0] + 1 + 3          # three steps into the second rollout
    buf = make_buffer(C, S)
    for ev in events[:cut]:
        apply_event(buf, ev)
        if ev[0] == "finish":
            list(buf.get(64)); buf.reset()
    sd = buf.state_dict()
    assert {k: v for k, v in sd.items() if not torch.is_tensor(v)} == {"pos": 3, "epoch": 1, "seed": PERM_SEED, "finished": False}
    assert len(sd) == 12
    other = make_buffer(C, S)
    other.seed = 99
    other.load_state_dict(sd)
    for ev in events[cut:]:
        apply_event(buf, ev); apply_event(other, ev)
    a, b = buf.state_dict(), other.state_dict()
    for k in a:
        assert torch.equal(a[k], b[k]) if torch.is_tensor(a[k]) else a[k] == b[k], k
    for x, y in zip(buf.get(64), other.get(64)):
        x, y = batch_arrays(x), batch_arrays(y)
        for k in x:
            assert np.array_equal(bits(x[k]), bits(y[k])), k
    want = rule_snapshots(C, S)[1]
    assert_state_equals(other, want)          # and it is the rule's second rollout
    assert np.array_equal(batch_arrays(other.gather(1, 0, 64))["index"], want["batches"][0]["index"])
