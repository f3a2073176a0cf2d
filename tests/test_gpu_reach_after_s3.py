"""GPU parity of what the main wave of the joint controller's three-wave Reach kernel (SplitMainCols) does between barrier S3 and the next S1.

In a remote sub-step the main wave reads, after S3, the acceleration the RNE wave left (abar) and the gear rows' columns z6, z8 the helper
wave left, finishes the gear rows -- the forces of the 2 x 2 complementarity problem from five of those numbers and from what it prepared
before S3 (the slots' D, aref, sign, 1 / D), then abar and the columns applied row by row as they stream in -- and takes the Euler step;
in a wave without a gear row the guard skips all but the read of abar.  Every case below runs one env-step's twenty sub-steps one at a
time (frame_skip = 1): the CPU oracle runs them first, alone; the engine then takes the oracle's state before each sub-step through
set_state, steps, and is compared with the oracle after it -- observation (with achieved goal and reward), qpos, qvel absolute, the warm
start (= qacc) relative to the lane's largest |qacc| (absolute where that is zero: a lane reset in the sub-step).

  none         no gear row in any lane in any sub-step: the guard is skipped, abar is the acceleration;
  row6, row8   one row per lane (row8: slot 0 holds row 8), even lanes below the lower limit, odd lanes above the upper one;
  both_lower, both_upper   both rows, on one side;
  mixed        both / row 6 / row 8 / none by lane % 4, lower / upper by (lane // 4) % 2: lanes without a row pass through the
               application with zero forces next to lanes with rows;
  crossing     lanes that start just inside a limit moving out, and just outside moving in, at either limit: rows appear and go;
  switch       `mixed` with two lanes per workgroup driven across arm joint 0's upper limit and back: remote, main-wave solve, remote;
  reset        `mixed` with max_episode_steps = 50 and elapsed = 40 in a fifth of the lanes: the tenth sub-step truncates and auto-resets
               them, the ten after it run the fresh lanes next to running ones.

165 environments (two full workgroups and a ragged one of 37 lanes), `mixed` once more at 65.  Gear velocities are uniform in +-1 rad/s,
each joint on its own, so that violated rows are active in some lanes and not in others: test_oracle_covers_every_active_set counts, on the
oracle alone, the (lane, sub-step) pairs of remote sub-steps in which each of limit_pair's four active sets is the consistent one, for
rows on the lower limits and on the upper ones, and wants at least MIN_PAIRS of each.

Bounds: 100 x the worst error of the build this change started from (round 9: one batch of 36 reads after S3, gear_rows_solve whole
behind it), measured on an MI355X on these very states in one run of this file (profiles/r10/after_s3_tests_parent.log); the measured
figures are in the comments.
"""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 165
SUBSTEPS = 20
ARM_HI = 2.96706                                     # jnt_range[0][1] of the mycobot280 tables
GEAR_LO, GEAR_HI, FINGER_HI = 0.0, 0.7, 0.872664     # the gear joints' range; the finger joints' is +-FINGER_HI
MIN_PAIRS = 5
SEED = 61

CASES = ("none", "row6", "row8", "both_lower", "both_upper", "mixed", "crossing", "switch", "reset")
RUNS = [(c, N) for c in CASES] + [("mixed", 65)]

BOUNDS = {       # obs, q, v, w: 100 x the parent build's worst error over the twenty sub-steps (the measured figures in the comment)
    ("none", N): dict(obs=7.2e-14, q=7.1e-12, v=3.5e-09, w=3.7e-11),            # 7.216e-16  7.123e-14  3.562e-11  3.719e-13
    ("row6", N): dict(obs=5.5e-14, q=5.6e-12, v=2.8e-09, w=4.6e-11),            # 5.551e-16  5.698e-14  2.849e-11  4.656e-13
    ("row8", N): dict(obs=5.5e-14, q=7.3e-12, v=3.6e-09, w=4.8e-11),            # 5.551e-16  7.372e-14  3.686e-11  4.824e-13
    ("both_lower", N): dict(obs=5.5e-14, q=1.4e-13, v=7.4e-11, w=4.2e-11),      # 5.551e-16  1.498e-15  7.488e-13  4.269e-13
    ("both_upper", N): dict(obs=5.5e-14, q=7.9e-12, v=3.9e-09, w=3.5e-11),      # 5.551e-16  7.944e-14  3.973e-11  3.590e-13
    ("mixed", N): dict(obs=7.7e-14, q=8.3e-12, v=4.1e-09, w=4.1e-11),           # 7.754e-16  8.343e-14  4.172e-11  4.183e-13
    ("crossing", N): dict(obs=5.5e-14, q=8.1e-12, v=4.0e-09, w=3.8e-11),        # 5.551e-16  8.155e-14  4.079e-11  3.832e-13
    ("switch", N): dict(obs=8.2e-14, q=7.6e-12, v=3.8e-09, w=4.7e-11),          # 8.223e-16  7.608e-14  3.804e-11  4.725e-13
    ("reset", N): dict(obs=6.6e-14, q=5.4e-12, v=2.7e-09, w=4.4e-11),           # 6.661e-16  5.473e-14  2.738e-11  4.433e-13
    ("mixed", 65): dict(obs=8.3e-14, q=6.6e-12, v=3.3e-09, w=3.7e-11),          # 8.327e-16  6.654e-14  3.327e-11  3.714e-13
}


def _groups(n):
    return [slice(g, min(g + 64, n)) for g in range(0, n, 64)]


def _outside(rng, n, upper):
    """Gear angles 1e-3 .. 5e-3 rad beyond the lower limit (upper[i] false) or the upper one."""
    d = rng.uniform(1e-3, 5e-3, n)
    return np.where(upper, GEAR_HI + d, GEAR_LO - d)


def _inside(rng, n, upper, near=False):
    """Gear angles inside the range, in its lower or upper part (the gear coupling pulls the two joints together): well inside, or
    (near) 2e-3 .. 8e-3 rad from the limit."""
    d = rng.uniform(2e-3, 8e-3, n) if near else rng.uniform(0.05, 0.3, n)
    return np.where(upper, GEAR_HI - d, GEAR_LO + d)


def _put(case, ora, rng, n):
    """Write the case's state into the oracle; returns the float32 action every sub-step takes."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(n)
    a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
    up = i % 2 == 1
    has6, has8 = np.zeros(n, bool), np.zeros(n, bool)
    if case == "row6": has6[:] = True
    elif case == "row8": has8[:] = True
    elif case in ("both_lower", "both_upper"):
        has6[:] = True; has8[:] = True; up = np.full(n, case == "both_upper")
    elif case in ("mixed", "switch", "reset"):
        has6 = (i % 4 == 0) | (i % 4 == 1); has8 = (i % 4 == 0) | (i % 4 == 2); up = (i // 4) % 2 == 1
    near = case in ("row6", "row8")                  # one row in every lane: the other joint just inside, or the gear coupling lifts the row at once
    q[:, 6] = np.where(has6, _outside(rng, n, up), _inside(rng, n, up, near))
    q[:, 8] = np.where(has8, _outside(rng, n, up), _inside(rng, n, up, near))
    qd[:, 6] = rng.uniform(-1.0, 1.0, n); qd[:, 8] = rng.uniform(-1.0, 1.0, n)
    a[:, 6] = np.where(up, 1.0, -1.0)                # the gripper servo pushes towards the limit the lane's rows are on
    if case == "crossing":
        # lane % 4: 0 inside the lower limit moving out, 1 outside it moving in, 2 inside the upper limit moving out, 3 outside it moving in
        c = i % 4
        start = np.select([c == 0, c == 1, c == 2], [GEAR_LO + 2e-3, GEAR_LO - 3e-3, GEAR_HI - 2e-3], GEAR_HI + 3e-3)
        speed = np.select([c == 0, c == 1, c == 2], [-1.0, 2.0, 1.0], -2.0)
        for j in (6, 8):
            q[:, j] = start + rng.uniform(-5e-4, 5e-4, n); qd[:, j] = speed * rng.uniform(0.8, 1.2, n)
        a[:, 6] = np.where(c >= 2, 1.0, -1.0)
    if case == "switch":
        x = (i % 64 == 5) | (i % 64 == 30)
        q[x, 0] = ARM_HI - 0.02; qd[x, 0] = rng.uniform(7.5, 8.5, int(x.sum())); a[x, 0] = 1.0
    if case == "reset":
        el = s["elapsed"].copy(); el[i % 5 == 2] = 40
        ora.set_state(elapsed=el)
    ora.set_state(qpos=q, qvel=qd)
    return a


def _gear_sets(ora, qpre, lanes):
    """limit_pair's consistent active set of every lane in `lanes` in the sub-step the oracle has just taken from qpos `qpre`, from the
    rows and forces its solver left: -> (sign [n]: +1 every gear row on its lower limit, -1 on its upper one, 0 no gear row or one of
    each; set [n]: 0 none, 1 slot 0 only, 2 slot 1 only, 3 both).  Slot 0 is row 6 where it exists, else row 8."""
    n = qpre.shape[0]
    sign, aset = np.zeros(n, np.int64), np.zeros(n, np.int64)
    for k in lanes:
        d = ora.data(int(k))
        ne, nl = int(d.get("ne", (1,), np.int32)[0]), int(d.get("nl", (1,), np.int32)[0])
        ids = d.get("efc_id", (ne + nl,), np.int32)[ne:]
        force = d.get("efc_force", (ne + nl,))[ne:]
        lo, hi = qpre[k, :10] < np.r_[[-ARM_HI] * 6, GEAR_LO, -FINGER_HI, GEAR_LO, -FINGER_HI], qpre[k, :10] > np.r_[[ARM_HI] * 6, GEAR_HI, FINGER_HI, GEAR_HI, FINGER_HI]
        assert sorted(ids.tolist()) == np.nonzero(lo | hi)[0].tolist(), (k, ids, qpre[k, :10])      # the rows of THIS sub-step
        act = {int(j): bool(f != 0) for j, f in zip(ids, force)}
        rows = [j for j in (6, 8) if j in act]
        if not rows: continue
        sides = {(-1 if hi[j] else +1) for j in rows}
        sign[k] = sides.pop() if len(sides) == 1 else 0
        aset[k] = (1 if act[rows[0]] else 0) + (2 if len(rows) == 2 and act[rows[1]] else 0)
    return sign, aset


@functools.lru_cache(maxsize=None)
def oracle_run(case, n):
    """The case's twenty sub-steps on the CPU oracle alone: dict(action, pre / post = the state before / after every sub-step, out = the
    step's outputs, arm / gear / other [20, groups] = some lane of the workgroup holds an arm row / a gear row / a finger row when the
    sub-step starts, sign / aset [20, n] = _gear_sets of the lanes of remote sub-steps (aset -1 elsewhere and in lanes reset by the sub-step))."""
    from tests.common import make_oracle
    ora = make_oracle(n, controller_type="joint", reward_type="dense", seed=SEED, frame_skip=1,
                      max_episode_steps=50 if case == "reset" else 10 ** 9)
    ora.reset(seed=SEED)
    rng = np.random.default_rng([SEED, CASES.index(case), n])
    ora.step(rng.uniform(-1, 1, (n, ora.act_dim)).astype(np.float32))      # warm start, lagged q and ctrl of a running episode
    a = _put(case, ora, rng, n)
    groups = _groups(n)
    r = dict(action=a, pre=[], post=[], out=[], arm=np.zeros((SUBSTEPS, len(groups)), bool), gear=np.zeros((SUBSTEPS, len(groups)), bool),
             other=np.zeros((SUBSTEPS, len(groups)), bool), sign=np.zeros((SUBSTEPS, n), np.int64), aset=-np.ones((SUBSTEPS, n), np.int64))
    for k in range(SUBSTEPS):
        pre = ora.get_state()
        o = ora.step(a)
        q = pre["qpos"]
        arm = (np.abs(q[:, :6]) > ARM_HI).any(axis=1)
        fing = (np.abs(q[:, [7, 9]]) > FINGER_HI).any(axis=1)
        gear = (q[:, [6, 8]] < GEAR_LO).any(axis=1) | (q[:, [6, 8]] > GEAR_HI).any(axis=1)
        done = o["terminated"].astype(bool) | o["truncated"].astype(bool)
        for g, sl in enumerate(groups):
            r["arm"][k, g], r["gear"][k, g], r["other"][k, g] = arm[sl].any(), gear[sl].any(), fing[sl].any()
            if not (arm[sl].any() or fing[sl].any()):
                lanes = [j for j in range(sl.start, sl.stop) if not done[j]]
                sg, st = _gear_sets(ora, q, lanes)
                r["sign"][k, lanes] = sg[lanes]; r["aset"][k, lanes] = st[lanes]
        r["pre"].append(pre); r["out"].append(o); r["post"].append(ora.get_state())
    for v in r.values():
        for x in (v if isinstance(v, list) else [v]):
            for y in (x.values() if isinstance(x, dict) else [x]): y.flags.writeable = False
    return r


def check_paths(case, n, r):
    """The sub-steps take the paths the case is about."""
    show = lambda m: " | ".join("".join("X" if x else "." for x in m[:, g]) for g in range(m.shape[1]))
    print(f"\n{case} ({n}): sub-steps with an arm row, per workgroup: {show(r['arm'])}\n{case} ({n}): sub-steps with a gear row, per workgroup: {show(r['gear'])}")
    assert not r["other"].any()                                                      # no finger row: the arm rows alone switch the path
    if case != "switch": assert not r["arm"].any()                                   # twenty remote sub-steps in every workgroup
    q = np.stack([s["qpos"] for s in r["pre"]])
    row = (q[:, :, [6, 8]] < GEAR_LO) | (q[:, :, [6, 8]] > GEAR_HI)                   # [20, n, 2]
    if case == "none": assert not r["gear"].any()
    if case in ("row6", "row8"):
        j = 0 if case == "row6" else 1
        assert row[0, :, j].all() and not row[0, :, 1 - j].any()                     # this row alone when the env-step starts, in every lane ...
        assert int((row[:, :, j] & ~row[:, :, 1 - j]).sum()) >= 5 * n                # ... and in a quarter of all (lane, sub-step) pairs at least
    if case in ("both_lower", "both_upper"): assert row[0].all()
    if case in ("mixed", "switch", "reset"):
        for g, sl in enumerate(_groups(n)):
            if sl.stop - sl.start >= 4:
                assert sorted(set((row[0, sl, 0] + 2 * row[0, sl, 1]).tolist())) == [0, 1, 2, 3], g      # all four kinds of lane in the wave
    if case == "crossing":
        appear, vanish = (~row[:-1] & row[1:]), (row[:-1] & ~row[1:])
        lower = q[1:, :, [6, 8]] < 0.35
        for what, m in (("appear", appear), ("vanish", vanish)):
            for side, sm in (("lower", lower), ("upper", ~lower)):
                cnt = int((m & sm).sum())
                print(f"crossing: rows that {what} on the {side} limit: {cnt}")
                assert cnt >= MIN_PAIRS, (what, side, cnt)
    if case == "switch":
        for g in range(r["arm"].shape[1]):
            k_out = np.nonzero(r["arm"][:, g])[0]
            assert not r["arm"][0, g] and k_out.size and k_out[0] >= 2 and k_out[-1] <= 17, (g, k_out)      # remote, main wave, remote again
            assert r["gear"][:, g].all()
    if case == "reset":
        trunc = np.stack([o["truncated"].astype(bool) for o in r["out"]])
        late = np.arange(n) % 5 == 2
        assert np.array_equal(trunc[9], late) and not trunc[:9].any() and not trunc[10:].any()      # the reset lands in the tenth sub-step


def coverage():
    """(sign, set) -> number of (lane, sub-step) pairs of remote sub-steps, over every run of this file."""
    cnt = {(sg, st): 0 for sg in (+1, -1) for st in (0, 1, 2, 3)}
    for case, n in RUNS:
        r = oracle_run(case, n)
        for key in cnt:
            cnt[key] += int(((r["sign"] == key[0]) & (r["aset"] == key[1])).sum())
    return cnt


def _sync(envs, s):
    envs.set_state(qpos=s["qpos"].T.copy(), qvel=s["qvel"].T.copy(), ctrl=s["ctrl"].T.copy(), warm=s["warm"].T.copy(),
                   qpos_lag=s["qpos_lag"].T.copy(), goal=s["goal"].T.copy(), elapsed=s["elapsed"].copy(), episode=s["episode"].copy())


def measure(case, n):
    """Worst errors over the twenty sub-steps and the n lanes: dict(obs, q, v, w)."""
    import torch
    from mycobotgym_amd import MyCobotVecEnv
    r = oracle_run(case, n)
    check_paths(case, n, r)
    envs = MyCobotVecEnv(n, device="cuda:0", has_object=False, controller_type="joint", reward_type="dense", seed=SEED, frame_skip=1,
                         max_episode_steps=50 if case == "reset" else 10 ** 9)
    envs.reset(seed=SEED)
    envs.counters(clear=True)
    a = torch.as_tensor(r["action"].copy())
    w = dict(obs=0.0, q=0.0, v=0.0, w=0.0)
    for k in range(SUBSTEPS):
        _sync(envs, r["pre"][k])
        obs, rew, term, trunc, info = envs.step(a)
        o, so = r["out"][k], r["post"][k]
        assert np.array_equal(obs["desired_goal"].cpu().numpy(), o["desired"]), (case, k)
        assert np.array_equal(term.cpu().numpy(), o["terminated"].astype(bool)) and np.array_equal(trunc.cpu().numpy(), o["truncated"].astype(bool)), (case, k)
        assert np.array_equal(info["is_success"].cpu().numpy(), o["is_success"].astype(bool)), (case, k)
        e = max(float(np.abs(obs["observation"].cpu().numpy() - o["obs"]).max()), float(np.abs(obs["achieved_goal"].cpu().numpy() - o["achieved"]).max()),
                float(np.abs(rew.cpu().numpy() - o["reward"]).max()))
        st = envs.get_state()
        gq, gv, gw = (st[x].cpu().numpy().T for x in ("qpos", "qvel", "warm"))
        assert all(np.isfinite(x).all() for x in (gq, gv, gw))
        assert np.array_equal(st["elapsed"].cpu().numpy(), so["elapsed"]) and np.array_equal(st["episode"].cpu().numpy(), so["episode"]), (case, k)
        ew, den = np.abs(gw - so["warm"]).max(axis=1), np.abs(so["warm"]).max(axis=1)
        ew = np.where(den > 0, ew / np.where(den > 0, den, 1.0), ew)
        w = dict(obs=max(w["obs"], e), q=max(w["q"], float(np.abs(gq - so["qpos"]).max())), v=max(w["v"], float(np.abs(gv - so["qvel"]).max())),
                 w=max(w["w"], float(ew.max())))
    assert envs.counters()["bad_state_resets"] == 0
    envs.close()
    print(f"{case} ({n}): " + " ".join(f"{x} {v:.3e}" for x, v in w.items()))
    return w


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def test_oracle_covers_every_active_set():
    cnt = coverage()
    print("\n(sign of the rows, active set 0 none / 1 slot 0 / 2 slot 1 / 3 both) -> (lane, sub-step) pairs: " + "  ".join(f"{k}: {v}" for k, v in sorted(cnt.items())))
    assert all(v >= MIN_PAIRS for v in cnt.values()), cnt


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_substeps_against_the_oracle(torch_cuda, case, n):
    w, b = measure(case, n), BOUNDS[(case, n)]
    assert w["obs"] <= b["obs"] and w["q"] <= b["q"] and w["v"] <= b["v"] and w["w"] <= b["w"], (w, b)
