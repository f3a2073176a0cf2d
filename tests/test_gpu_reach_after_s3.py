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

from tests import reach_parity as rp
from tests.common import torch_cuda  # noqa: F401
from tests.reach_parity import ARM_HI, FINGER_HI, GEAR_HI, GEAR_LO, N, SEED, SUBSTEPS

pytestmark = pytest.mark.gpu

MIN_PAIRS = 5

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
    rng = np.random.default_rng([SEED, CASES.index(case), n])
    ora = rp.oracle(n, 1, SEED, rp.episode_limit(case), running=rng)
    a = rp.put_gear_case(case, ora, rng, n)
    groups = rp.groups(n)
    r = dict(action=a, arm=np.zeros((SUBSTEPS, len(groups)), bool), gear=np.zeros((SUBSTEPS, len(groups)), bool),
             other=np.zeros((SUBSTEPS, len(groups)), bool), sign=np.zeros((SUBSTEPS, n), np.int64), aset=-np.ones((SUBSTEPS, n), np.int64))

    def rows_and_sets(k, pre, o):
        q = pre["qpos"]
        arm, gear, fing = rp.limit_rows_of(q)
        done = o["terminated"].astype(bool) | o["truncated"].astype(bool)
        for g, sl in enumerate(groups):
            r["arm"][k, g], r["gear"][k, g], r["other"][k, g] = arm[sl].any(), gear[sl].any(), fing[sl].any()
            if not (arm[sl].any() or fing[sl].any()):
                lanes = [j for j in range(sl.start, sl.stop) if not done[j]]
                sg, st = _gear_sets(ora, q, lanes)
                r["sign"][k, lanes] = sg[lanes]; r["aset"][k, lanes] = st[lanes]

    r.update(rp.record_substeps(ora, a, each=rows_and_sets))
    return rp.freeze(r)


def check_paths(case, n, r):
    """The sub-steps take the paths the case is about."""
    print(f"\n{case} ({n}): sub-steps with an arm row, per workgroup: {rp.show(r['arm'])}\n{case} ({n}): sub-steps with a gear row, per workgroup: {rp.show(r['gear'])}")
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
        for g, sl in enumerate(rp.groups(n)):
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


def measure(case, n):
    """Worst errors over the twenty sub-steps and the n lanes: dict(obs, q, v, w)."""
    r = oracle_run(case, n)
    check_paths(case, n, r)
    return rp.measure_substeps(r, lambda frame_skip: rp.engine(n, frame_skip, SEED, rp.episode_limit(case)), f"{case} ({n})")


def test_oracle_covers_every_active_set():
    cnt = coverage()
    print("\n(sign of the rows, active set 0 none / 1 slot 0 / 2 slot 1 / 3 both) -> (lane, sub-step) pairs: " + "  ".join(f"{k}: {v}" for k, v in sorted(cnt.items())))
    assert all(v >= MIN_PAIRS for v in cnt.values()), cnt


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_substeps_against_the_oracle(torch_cuda, case, n):
    w, b = measure(case, n), BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)
