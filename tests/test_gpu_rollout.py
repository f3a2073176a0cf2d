"""The device-resident on-policy rollout buffer (mcg_rollout_start / _add / _gae / _gather, mycobotgym_amd/rollout.py) against the rule
restated in tests/indep_rollout.py, and on the real engine.  Shapes: the smallest that break a wrong kernel -- 40 environments (neither
a multiple of 64 nor of 32; several blocks of the insertion kernel), 7 steps (M = 280 is no power of two: the permutation walks),
D = 25 and A = 7 (a record of 39 words padded to 40), minibatches of 64 with a short last one."""
import functools

import numpy as np
import pytest

from tests.common import bits
from tests.indep_rollout import PERM_SEED, Rollout, record_dtype

pytestmark = pytest.mark.gpu

N, D, A, T, MAX_STEPS = 40, 25, 7, 7, 7
GAMMA, LAMBDA = 0.99, 0.95
RESTART_AT, RESTARTED = 3, 5
FIELDS = ("obs", "achieved", "desired", "action", "old_value", "old_log_prob", "advantage", "returns")
PLANES = ("reward", "value", "episode_start", "advantage", "returns")


@functools.lru_cache(maxsize=None)
def synthetic_events(n=N, steps=T, rollouts=2, restart_at=RESTART_AT, poison=False, D=D, A=A):
    """Step outputs from default_rng(0): ("start", obs, achieved, desired, mask), ("add", actions, values, log_probs, final_values, out)
    and ("finish", last_values) events, `rollouts` rollouts of `steps` steps.  final_* differ from the post-reset values (the buffer must
    not read them); episode lengths are uniform in 1..7; `terminated` on a random half of the ends; before step `restart_at` a masked
    start restarts five environments.  poison: the values of environment 3 at step 2 and of environment 17 at step 4 are inf and nan."""
    rng = np.random.default_rng(0)
    goal = lambda: rng.uniform(-0.03, 0.03, (n, 3))
    f = lambda *s: rng.normal(size=s).astype(np.float32)
    events = [("start", rng.normal(size=(n, D)), goal(), goal(), None)]
    left = rng.integers(1, MAX_STEPS + 1, n)             # steps the episode in flight still has
    for i in range(rollouts * steps):
        if i == restart_at:
            mask = np.zeros(n, dtype=bool)
            mask[rng.choice(n, RESTARTED, replace=False)] = True
            events.append(("start", rng.normal(size=(n, D)), goal(), goal(), mask))
            left[mask] = rng.integers(1, MAX_STEPS + 1, RESTARTED)
        left -= 1
        done = left == 0
        terminated = done & (rng.random(n) < 0.5)
        truncated = done & (~terminated | (rng.random(n) < 0.5))         # the engine sets truncated with terminated; both forms occur
        out = {"obs": rng.normal(size=(n, D)), "achieved_goal": goal(), "desired_goal": goal(), "reward": rng.normal(size=n),
               "terminated": terminated, "truncated": truncated, "final_obs": rng.normal(size=(n, D)), "final_achieved": goal(),
               "final_desired": goal()}
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
def rule_snapshots(n=N, steps=T, rollouts=2, restart_at=RESTART_AT, with_final_values=True, batch=64, poison=False, D=D, A=A):
    """The rule on the events: after every finish its records, planes, carried state and the epoch's minibatches.  Computed once,
    shared, not modified."""
    R = Rollout(n, D, A, steps, GAMMA, LAMBDA)
    snaps = []
    for ev in synthetic_events(n, steps, rollouts, restart_at, poison, D, A):
        if ev[0] == "start":
            R.start(ev[1], ev[2], ev[3], ev[4])
        elif ev[0] == "add":
            R.add(ev[1], ev[2], ev[3], ev[5], final_values=ev[4] if with_final_values else None)
        else:
            R.finish(ev[1])
            epoch = len(snaps)
            snaps.append({"records": R.records(), "planes": R.planes(), "carried": R.carried(),
                          "batches": [R.gather(PERM_SEED, epoch, first, count) for first, count in minibatches(steps * n, batch)]})
            R.reset()
    return tuple(snaps)


def apply_event(buf, ev, with_final_values=True):
    import torch
    t = lambda x: torch.as_tensor(x, device=buf.device)
    if ev[0] == "start":
        buf.start({"observation": t(ev[1]), "achieved_goal": t(ev[2]), "desired_goal": t(ev[3])}, mask=None if ev[4] is None else t(ev[4]))
    elif ev[0] == "add":
        o = ev[5]
        obs = {"observation": t(o["obs"]), "achieved_goal": t(o["achieved_goal"]), "desired_goal": t(o["desired_goal"])}
        info = {"final_observation": {"observation": t(o["final_obs"]), "achieved_goal": t(o["final_achieved"]), "desired_goal": t(o["final_desired"])}}
        buf.add(t(ev[1]), t(ev[2]), t(ev[3]), obs, t(o["reward"]), t(o["terminated"]), t(o["truncated"]), info,
                final_values=t(ev[4]) if with_final_values else None)
    else:
        buf.finish(t(ev[1]))


def make_buffer(n=N, steps=T, D=D, A=A, **kw):
    from mycobotgym_amd import RolloutBuffer
    buf = RolloutBuffer(n_steps=steps, gamma=GAMMA, gae_lambda=LAMBDA, seed=PERM_SEED, num_envs=n, obs_dim=D, act_dim=A, **kw)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(0xA5)
    return buf


def guards_intact(buf):
    return all(bool((g == 0xA5).all()) for pair in buf.guards().values() for g in pair)


def batch_arrays(b):
    o = {"obs": b.observations["observation"], "achieved": b.observations["achieved_goal"], "desired": b.observations["desired_goal"],
         "action": b.actions, "old_value": b.old_values, "old_log_prob": b.old_log_prob, "advantage": b.advantages, "returns": b.returns,
         "index": b.index}
    return {k: v.cpu().numpy() for k, v in o.items()}


def assert_state_equals(buf, snap, skip_envs=()):
    keep = np.array([e not in skip_envs for e in range(buf.num_envs)])
    got = buf.records().cpu().numpy().reshape(buf.n_steps, buf.num_envs, -1).view(record_dtype(buf.obs_dim, buf.act_dim))[..., 0]
    for name in snap["records"].dtype.names:
        assert np.array_equal(bits(got[name]), bits(snap["records"][name])), name
    assert got.tobytes() == snap["records"].tobytes()
    P = {k: v.cpu().numpy() for k, v in buf.planes().items()}
    for name in PLANES:
        assert P[name].dtype == snap["planes"][name].dtype and P[name].shape == (buf.n_steps, buf.num_envs), name
        assert np.array_equal(bits(P[name])[:, keep], bits(snap["planes"][name])[:, keep]), name
    sd = buf.state_dict()
    for name, ref in snap["carried"].items():
        assert np.array_equal(bits(sd[name].cpu().numpy()), bits(ref)), name
    return P


def assert_epoch_equals(buf, snap, batch, skip_fields=()):
    M = buf.n_steps * buf.num_envs
    got = [batch_arrays(mb) for mb in buf.get(batch)]
    assert [len(g["index"]) for g in got] == [c for _, c in minibatches(M, batch)] == [len(w["index"]) for w in snap["batches"]]
    for g, want in zip(got, snap["batches"]):
        assert g["index"].dtype == np.int32 and np.array_equal(g["index"], want["index"])
        for name in FIELDS:
            if name in skip_fields:
                continue
            assert g[name].dtype == np.float32 and g[name].shape == want[name].shape, name
            assert np.array_equal(bits(g[name]), bits(want[name])), name
    assert sorted(np.concatenate([g["index"] for g in got]).tolist()) == list(range(M))
    return got


def run_against_rule(n, steps, rollouts, restart_at, with_final_values, batch, D=D, A=A):
    snaps = rule_snapshots(n, steps, rollouts, restart_at, with_final_values, batch, False, D, A)
    # the walk's length is a condition of the inputs, settled before the GPU is touched
    longest = max(int(b["passes"].max()) for s in snaps for b in s["batches"])
    print(f"(T, N) = ({steps}, {n}): longest walk {longest} passes")
    assert longest <= 64
    buf = make_buffer(n, steps, D, A, guard_rows=2)
    done = 0
    for ev in synthetic_events(n, steps, rollouts, restart_at, False, D, A):
        apply_event(buf, ev, with_final_values)
        if ev[0] == "finish":
            assert_state_equals(buf, snaps[done])
            assert_epoch_equals(buf, snaps[done], batch)
            assert buf.epoch == done + 1
            buf.reset()
            done += 1
    assert done == rollouts and guards_intact(buf)
    return snaps


@pytest.mark.parametrize("with_final_values", [True, False])
def test_synthetic_events_match_the_rule(built, with_final_values):
    """Two rollouts of 7 steps with reset() between them (last_obs / last_start carry over), a masked start at step 3: after each, the
    records, the five planes, the carried state and every output of the five minibatches of get(64) (four of 64, one of 24) equal
    the rule's byte for byte; the epoch's indices are 0 .. 279 once each; the guard rows are intact."""
    snaps = run_against_rule(N, T, 2, RESTART_AT, with_final_values, 64)
    assert [len(b["index"]) for b in snaps[0]["batches"]] == [64, 64, 64, 64, 24]
    ev = [e for e in synthetic_events() if e[0] == "add"]
    boot = sum(int((e[5]["truncated"] & ~e[5]["terminated"]).sum()) for e in ev)
    both = sum(int((e[5]["truncated"] & e[5]["terminated"]).sum()) for e in ev)
    assert boot >= 10 and both >= 5          # the bootstrap and its exception both occur
    if with_final_values:                    # and the bootstrap changes the reward plane
        other = rule_snapshots(N, T, 2, RESTART_AT, False, 64)
        assert not np.array_equal(snaps[0]["planes"]["reward"], other[0]["planes"]["reward"])
    assert any(s["planes"]["episode_start"][0].sum() not in (0, N) for s in snaps[1:])          # last_start carried over, mixed


@pytest.mark.parametrize("steps,n", [(4, 64), (1, 1)])
def test_no_walk_and_degenerate_shapes(built, steps, n):
    """(4, 64): M = 256 = 2^b, every position lands at once.  (1, 1): b = 2, one transition, three of four values walk on."""
    snaps = run_against_rule(n, steps, 2, None, True, 64)
    if steps * n == 256:
        assert all(int(b["passes"].max()) == 1 for s in snaps for b in s["batches"])


def test_record_of_66_pairs_takes_two_passes_of_the_copy_phase(built):
    """D = 116, A = 7: a record of 130 words padded to 132, 66 pairs -- the smallest at which the copy phase's loop over pairs goes
    round twice, the second pass with two lanes.  One rollout of 3 steps of 11 environments (a masked start before step 1), one epoch
    of get(16): two minibatches of 16 and one of 1."""
    assert record_dtype(116, 7).itemsize == 66 * 8
    snaps = run_against_rule(11, 3, 1, 1, True, 16, D=116, A=7)
    assert [len(b["index"]) for b in snaps[0]["batches"]] == [16, 16, 1]


def test_non_finite_policy_outputs(built):
    """A value of inf (environment 3, step 2) and of nan (environment 17, step 4): every call returns, the other environments' planes
    and samples equal the rule's, the two environments' advantages are non-finite from that step backwards, the guard rows are
    intact.  No address depends on a stored value, so nothing here can fault."""
    import torch
    snap = rule_snapshots(N, T, 1, RESTART_AT, True, 64, True)[0]
    buf = make_buffer(guard_rows=2)
    for ev in synthetic_events(N, T, 1, RESTART_AT, True):
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
    buf = make_buffer()
    events = synthetic_events()
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
    with pytest.raises(ValueError, match="finish"):
        buf.get(64)
    with pytest.raises(ValueError, match="full"):
        apply_event(buf, adds[4])
    buf.finish(np.zeros(N, np.float32))
    assert sum(len(mb.index) for mb in buf.get()) == T * N and buf.epoch == 1
    with pytest.raises(ValueError, match="batch_size"):
        buf.get(0)
    from mycobotgym_amd import RolloutBuffer
    with pytest.raises(ValueError, match="needs envs= or"):
        RolloutBuffer(n_steps=4, num_envs=3)


def test_image_ids_are_refused(built):
    from mycobotgym_amd import RolloutBuffer, make
    envs = make("MyCobotReach-Dense-joint-v1", num_envs=2)
    with pytest.raises(ValueError, match="-v1 image ids"):
        RolloutBuffer(envs, n_steps=4)
    envs.close()


def real_engine_run(env_id, threshold=None, action_seed=None):
    """The checks of test_with_the_real_engine; threshold: a distance threshold other than the default; action_seed: actions from
    default_rng(action_seed) on the host in place of the policy's -> rows ended by the time limit alone, rows ended by success."""
    import torch
    from mycobotgym_amd import RolloutBuffer, make
    steps = 16
    kw = dict(num_envs=N, max_episode_steps=MAX_STEPS, seed=3)
    if threshold is not None:
        kw["distance_threshold"] = threshold
    rng = np.random.default_rng(action_seed) if action_seed is not None else None
    envs, twin = make(env_id, **kw), make(env_id, **kw)
    buf = RolloutBuffer(envs, n_steps=steps, gamma=GAMMA, gae_lambda=LAMBDA, seed=PERM_SEED, guard_rows=1)
    Do, Aa = envs.obs_dim, envs.action_dim
    assert (buf.num_envs, buf.obs_dim, buf.act_dim) == (N, Do, Aa)
    for pair in buf.guards().values():
        for g in pair:
            g.fill_(0xA5)
    gen = torch.Generator(device="cpu"); gen.manual_seed(5)
    W = (torch.randn(Do + 6, Aa + 2, generator=gen) * 0.5).to(envs.device)

    def policy(o):          # a fixed linear "policy": actions, values, log-probs
        x = torch.cat([o["observation"], o["achieved_goal"], o["desired_goal"]], dim=1).float() @ W
        return torch.tanh(x[:, :Aa]).contiguous(), x[:, Aa].contiguous(), x[:, Aa + 1].contiguous()

    host = lambda x: {k: host(v) for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy()
    f32 = lambda x: np.asarray(x, dtype=np.float64).astype(np.float32)
    obs, _ = envs.reset(seed=0)
    twin.reset(seed=0)
    buf.start(obs)
    R = Rollout(N, Do, Aa, steps, GAMMA, LAMBDA)
    first = host(obs)
    R.start(first["observation"], first["achieved_goal"], first["desired_goal"])
    prev, ended, boot_rows, both_rows = first, 0, 0, 0
    for rollout in range(2):
        log = []
        for _ in range(steps):
            a, v, lp = policy(obs)
            if rng is not None:      # seeded host actions, which the CPU oracle can replay
                a = torch.as_tensor(rng.uniform(-1, 1, (N, Aa)).astype(np.float32), device=envs.device)
            obs, r, term, trunc, info = envs.step(a)
            fv = policy(info["final_observation"])[1]
            buf.add(a, v, lp, obs, r, term, trunc, info, final_values=fv)
            twin.step(a)
            s = {"prev": prev, "action": host(a), "value": host(v), "log_prob": host(lp), "reward": host(r.double()), "terminated": host(term),
                 "truncated": host(trunc), "final_values": host(fv), "obs": host(obs)}
            R.add(s["action"], s["value"], s["log_prob"], {"obs": s["obs"]["observation"], "achieved_goal": s["obs"]["achieved_goal"],
                                                            "desired_goal": s["obs"]["desired_goal"], "reward": s["reward"],
                                                            "terminated": s["terminated"], "truncated": s["truncated"]}, final_values=s["final_values"])
            log.append(s)
            prev = s["obs"]
            ended += int((s["truncated"] | s["terminated"]).sum())
            boot_rows += int((s["truncated"] & ~s["terminated"]).sum()); both_rows += int((s["truncated"] & s["terminated"]).sum())
        lv = policy(obs)[1]
        buf.finish(lv)
        R.finish(host(lv))
        P = {k: x.cpu().numpy() for k, x in buf.planes().items()}
        # the reward plane from the host copies, by the recalled rule; float32 numpy arrays round every operation
        for t, s in enumerate(log):
            boot = (np.float32(GAMMA) * s["final_values"].astype(np.float32)).astype(np.float32)
            want = np.where(s["truncated"] & ~s["terminated"], f32(s["reward"]) + boot, f32(s["reward"])).astype(np.float32)
            assert np.array_equal(bits(P["reward"][t]), bits(want)), t
            assert np.array_equal(bits(P["value"][t]), bits(s["value"])), t
        ref = R.planes()
        for name in PLANES:
            assert np.array_equal(bits(P[name]), bits(ref[name])), name
        seen = []
        for mb in buf.get(256):
            g = batch_arrays(mb)
            for j, i in enumerate(g["index"].tolist()):
                e, t = divmod(i, steps)
                s = log[t]
                assert np.array_equal(bits(g["obs"][j]), bits(f32(s["prev"]["observation"][e]))), (i, "obs")
                assert np.array_equal(bits(g["achieved"][j]), bits(f32(s["prev"]["achieved_goal"][e]))), (i, "achieved")
                assert np.array_equal(bits(g["desired"][j]), bits(f32(s["prev"]["desired_goal"][e]))), (i, "desired")
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
    print(f"{env_id}: {ended} episodes ended")
    assert ended >= N * (2 * steps // MAX_STEPS)          # true by the time limit alone
    assert guards_intact(buf)
    envs.close(); twin.close()
    return boot_rows, both_rows


@pytest.mark.parametrize("env_id", ["MyCobotReach-Dense-joint-v0", "MyCobotPickAndPlace-Sparse-IK-v0"])
def test_with_the_real_engine(built, env_id):
    """Two rollouts of 16 steps of 40 environments (time limit 7) under a fixed linear policy.  Every gathered sample is the float32 cast
    of what reset / step returned at its (step, env); the reward plane is the recalled bootstrap rule on the host copies of reward,
    terminated, truncated and final_values; advantages and returns equal the rule's on those inputs bit for bit; the engine's state
    is what it is without a buffer.  Measured on an MI355X: 160 episodes ended in either run (the time limit's 40 * 4)."""
    real_engine_run(env_id)


# threshold per id: the smallest at which the CPU oracle's replay of this very run (seed 3, reset seed 0, default_rng(1) actions, 32 steps of
# 40 environments, time limit 7) ends at least 10 episodes by success and 10 by the time limit alone.  PickAndPlace: 0.12 of
# {0.08, 0.1, 0.12, 0.15} (0.08, 0.1: no success).  Reach: the oracle's run has no success ending at any of the four, nor at 0.2 and
# 0.25, and 9 at 0.3 (a random joint policy does not bring the gripper closer within 7 steps); the list continued in steps of 0.05
# gives 0.35.
SUCCESS_THRESHOLD = {"MyCobotReach-Dense-joint-v0": 0.35, "MyCobotPickAndPlace-Sparse-IK-v0": 0.12}


@pytest.mark.parametrize("env_id", list(SUCCESS_THRESHOLD))
def test_with_the_real_engine_and_success_endings(built, env_id):
    """test_with_the_real_engine's checks on a run in which episodes end both ways, so that `terminated & truncated` from the step
    kernel's tail reaches the buffer: rows without the bootstrap next to time-limit rows with it (the reward plane is asserted row by
    row against the recalled rule, the advantages against tests/indep_rollout.py).  Actions are seeded host draws, so that the CPU
    oracle can replay the run: Reach (0.35) 63 episodes ended by success and 143 by the time limit alone, PickAndPlace (0.12) 34 and
    160; asserted here: at least 5 of each kind (half the oracle's floor of 10: the physics is chaotic, the engine's counts differ).
    Measured on an MI355X: the oracle's counts exactly, 63 / 143 and 34 / 160."""
    boot_rows, both_rows = real_engine_run(env_id, SUCCESS_THRESHOLD[env_id], action_seed=1)
    print(f"{env_id} at threshold {SUCCESS_THRESHOLD[env_id]}: {both_rows} rows ended by success (no bootstrap), {boot_rows} by the time limit alone")
    assert both_rows >= 5 and boot_rows >= 5


def test_checkpoint(built):
    """state_dict() in mid-rollout into a new buffer: the rest of the rollout, finish and the next epoch's minibatches are identical."""
    import torch
    events = synthetic_events()
    cut = [i for i, ev in enumerate(events) if ev[0] == "finish"][0] + 1 + 3          # three steps into the second rollout
    buf = make_buffer()
    for ev in events[:cut]:
        apply_event(buf, ev)
        if ev[0] == "finish":
            list(buf.get(64)); buf.reset()
    sd = buf.state_dict()
    assert {k: v for k, v in sd.items() if not torch.is_tensor(v)} == {"pos": 3, "epoch": 1, "seed": PERM_SEED, "finished": False}
    assert len(sd) == 13
    other = make_buffer()
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
    # and it is the rule's second epoch
    want = rule_snapshots()[1]["batches"][0]
    assert np.array_equal(batch_arrays(other.gather(1, 0, 64))["index"], want["index"])
