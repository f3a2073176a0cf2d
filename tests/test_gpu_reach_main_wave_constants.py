"""GPU parity of the model constants the main wave of the joint controller's three-wave Reach kernel (SplitMainCols) fetches between the
barriers S1t and S2: the actuators' gains, ranges and biases, each connect side's offsets, anchors, solver parameters and diag, the gear
coupling's, the ten joint ranges, and the solver parameters and diag of every limit row that is taken.  The wave loads each block's
constants in one batch of scalar loads and evaluates the impedance without a branch (impedance_flat).

In the built-in tables, and in tests/common.py's perturbed ones, the limit rows 6-11 and the three equalities all carry the same solref /
solimp: a batch that fetched another row's record, or another side's, would pass every other test.  The table here starts from
perturbed_table("mycobot280_reach") and gives every limit row and every equality a solref / solimp of its own (TABLE_ROWS, TABLE_EQ):
power 1 on gear row 6 and on connect side 1, d0 == dmax on gear row 8 (the impedance's constant arm), arm joint 3's and 4's ctrlrange
narrowed to +-0.5 so that the arm's controls exceed it too.

  gear    gear rows at either limit, violated by 0.1, 0.4, 0.8 and 1.5 x the row's width by lane % 4 (both sides of the impedance's
          midpoint, and beyond its width), lower / upper by (lane // 4) % 2, row 6 / row 8 / both by (lane // 8) % 3;
  none    no gear row in any lane;
  arm     `gear` with two lanes per workgroup beyond arm joint 0's upper limit from the first sub-step on: the main wave solves itself.

In every case the even lanes' controls are uniform in +-1 (servo errors of a radian: every arm servo at its forcerange, joints 3 and 4
beyond their ctrlrange; the gripper's control is +-1, below its ctrlrange in half of the lanes) and the odd lanes' arm controls lie
within 2 mrad of the joint angles (forces inside the forcerange).

Each case runs twice against the CPU oracle, as tests/test_gpu_reach_side_wave_slots.py does: the env-step's twenty sub-steps one at a
time (frame_skip = 1, the oracle's state before each sub-step put into the engine through set_state, compared after it), and one whole
env-step (frame_skip = 20) from the state the first sub-step started from.  165 environments (two full workgroups and a ragged one of
37 lanes), `gear` once more at 65.

Compared: observation (with achieved goal and reward), qpos, qvel absolute, the warm start (= qacc) relative to the lane's largest |qacc|.
Bounds: 100 x the worst error of the build this change started from (branching impedance, constants fetched piece by piece), measured on
an MI355X on these very states in one run of this file's measure functions (profiles/r12/main_wave_constants_parent.log); the measured
figures are in the comments.
"""
import functools
import json

import numpy as np
import pytest

from tests import reach_parity as rp
from tests.common import torch_cuda  # noqa: F401
from tests.reach_parity import GEAR_HI, GEAR_LO, N

pytestmark = pytest.mark.gpu

SEED = 67
CASES = ("gear", "none", "arm")
RUNS = [(c, N) for c in CASES] + [("gear", 65)]

# joint -> (solref, solimp = d0 dmax width midpoint power): one record per limit row, no two alike
TABLE_ROWS = {
    0: ((0.020, 1.00), (0.900, 0.950, 0.0010, 0.50, 2)), 1: ((0.021, 0.98), (0.905, 0.952, 0.0012, 0.45, 2)),
    2: ((0.022, 0.96), (0.910, 0.954, 0.0014, 0.55, 2)), 3: ((0.023, 0.94), (0.915, 0.956, 0.0016, 0.40, 2)),
    4: ((0.024, 0.92), (0.920, 0.958, 0.0018, 0.60, 2)), 5: ((0.025, 0.90), (0.925, 0.960, 0.0020, 0.35, 2)),
    6: ((0.0060, 0.95), (0.940, 0.985, 0.0040, 0.50, 1)),            # gear row 6: power 1
    7: ((0.0070, 1.05), (0.935, 0.980, 0.0030, 0.45, 2)),
    8: ((0.0080, 0.90), (0.970, 0.970, 0.0060, 0.40, 2)),            # gear row 8: d0 == dmax
    9: ((0.0090, 1.10), (0.945, 0.975, 0.0050, 0.55, 2)),
}
TABLE_EQ = (((0.0060, 0.90), (0.930, 0.980, 0.0020, 0.40, 2)),      # connect side 0
            ((0.0055, 1.10), (0.940, 0.985, 0.0015, 0.60, 1)),      # connect side 1: power 1
            ((0.0070, 0.95), (0.920, 0.970, 0.0030, 0.45, 2)))      # the gear coupling
WIDTH = {6: TABLE_ROWS[6][1][2], 8: TABLE_ROWS[8][1][2]}
NARROW = (3, 4)                                                      # arm actuators with ctrlrange +-0.5

SUB_BOUNDS = {      # single sub-steps: obs, q, v, w = 100 x the parent build's worst error (the measured figures in the comment)
    ("gear", N): dict(obs=6.661e-14, q=2.756e-12, v=1.377e-09, w=6.148e-11),                # 6.661e-16  2.756e-14  1.377e-11  6.148e-13
    ("none", N): dict(obs=5.551e-14, q=2.938e-12, v=1.469e-09, w=4.213e-11),                # 5.551e-16  2.938e-14  1.469e-11  4.213e-13
    ("arm", N): dict(obs=6.106e-14, q=3.446e-12, v=1.723e-09, w=5.104e-11),                 # 6.106e-16  3.446e-14  1.723e-11  5.104e-13
    ("gear", 65): dict(obs=5.551e-14, q=2.789e-12, v=1.394e-09, w=4.659e-11),               # 5.551e-16  2.789e-14  1.394e-11  4.659e-13
}
ENV_BOUNDS = {      # whole env-steps: likewise
    ("gear", N): dict(obs=1.466e-11, q=4.078e-11, v=2.873e-09, w=9.398e-10),                # 1.466e-13  4.078e-13  2.873e-11  9.398e-12
    ("none", N): dict(obs=3.672e-12, q=6.473e-12, v=4.388e-10, w=1.813e-10),                # 3.672e-14  6.473e-14  4.388e-12  1.813e-12
    ("arm", N): dict(obs=3.549e-11, q=6.797e-12, v=4.451e-09, w=3.054e-09),                 # 3.549e-13  6.797e-14  4.451e-11  3.054e-11
    ("gear", 65): dict(obs=8.304e-12, q=3.603e-12, v=2.095e-09, w=1.430e-09),               # 8.304e-14  3.603e-14  2.095e-11  1.430e-11
}


@functools.lru_cache(maxsize=None)
def _table_json():
    from tests.common import perturbed_table
    tab = perturbed_table("mycobot280_reach")
    for j, (solref, solimp) in TABLE_ROWS.items():
        tab["jnt_solref"][j] = list(solref); tab["jnt_solimp"][j] = [float(x) for x in solimp]
    for e, (solref, solimp) in zip(tab["eq"], TABLE_EQ):
        e["solref"] = list(solref); e["solimp"] = [float(x) for x in solimp]
    for u in NARROW:
        tab["actuators"][u]["ctrlrange"] = [-0.5, 0.5]
    return json.dumps(tab)


def table():
    return json.loads(_table_json())


def _put(case, ora, rng, n):
    """Write the case's state into the oracle; returns the float32 action every sub-step takes."""
    tab = table()
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(n)
    a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
    odd = i % 2 == 1
    a[odd, :6] = (q[odd, :6] + rng.uniform(-2e-3, 2e-3, (int(odd.sum()), 6))).astype(np.float32)
    up = (i // 4) % 2 == 1
    factor = np.array([0.1, 0.4, 0.8, 1.5])[i % 4]
    kind = (i // 8) % 3                                               # 0: row 6, 1: row 8, 2: both
    has6, has8 = (kind != 1), (kind != 0)
    if case == "none": has6[:] = False; has8[:] = False
    inside = rng.uniform(0.05, 0.3, (n, 2))
    for col, j, has in ((0, 6, has6), (1, 8, has8)):
        out = np.where(up, GEAR_HI + factor * WIDTH[j], GEAR_LO - factor * WIDTH[j])
        q[:, j] = np.where(has, out, np.where(up, GEAR_HI - inside[:, col], GEAR_LO + inside[:, col]))
    qd[:, 6] = rng.uniform(-1.0, 1.0, n); qd[:, 8] = rng.uniform(-1.0, 1.0, n)
    a[:, 6] = np.where(up, 1.0, -1.0)                # the gripper servo pushes towards the limit the lane's rows are on
    if case == "arm":
        x = (i % 64 == 4) | (i % 64 == 30)               # (even lanes: controls of their own)
        q[x, 0] = tab["jnt_range"][0][1] + 0.03; qd[x, 0] = 0.0; a[x, 0] = 1.0
    ora.set_state(qpos=q, qvel=qd)
    return a


@functools.lru_cache(maxsize=None)
def oracle_run(case, n):
    """The case on the CPU oracle alone: dict(action; pre / post / out = state before / after and outputs of each of the twenty single
    sub-steps; env_pre = the state the env-step starts from; env_post / env_out = state and outputs after it)."""
    rng = np.random.default_rng([SEED, 12, CASES.index(case), n])
    ora = rp.oracle(n, 1, SEED, table=table(), running=rng)
    a = _put(case, ora, rng, n)
    r = dict(action=a)
    start = ora.get_state()
    r.update(rp.record_substeps(ora, a))
    r.update(rp.replay_env_steps(rp.oracle(n, 20, SEED, table=table()), start, a))
    for s in r["post"] + r["env_post"]:
        assert all(np.isfinite(s[x]).all() and np.abs(s[x]).max() < 1e6 for x in ("qpos", "qvel", "warm")), case
    return rp.freeze(r)


def check_paths(case, n, r):
    """The states are the ones the case is about."""
    tab = table()
    q0, a = r["pre"][0]["qpos"], r["action"]
    i = np.arange(n)
    viol = np.maximum(GEAR_LO - q0[:, [6, 8]], q0[:, [6, 8]] - GEAR_HI)                    # [n, 2], > 0: the row exists
    arm_hi = np.array([tab["jnt_range"][j][1] for j in range(6)])
    q = np.stack([s["qpos"] for s in r["pre"]])
    arm = (np.abs(q[:, :, :6]) > arm_hi).any(axis=2)                                       # [20, n]
    if case == "none":
        assert not (viol > 0).any()
    else:
        for col, j in ((0, 6), (1, 8)):
            x = viol[:, col] / WIDTH[j]
            for g in (g for g in rp.groups(n) if g.stop - g.start >= 24):      # 24 lanes: one period of the three patterns
                for f in (0.1, 0.4, 0.8, 1.5):
                    for upper in (False, True):
                        m = np.isclose(x[g], f) & ((q0[g, j] > GEAR_HI) == upper)
                        assert m.any(), (case, j, f, upper)                                # every violation, at either limit, in every workgroup
        kinds = (viol[:, 0] > 0) + 2 * (viol[:, 1] > 0)
        assert sorted(set(kinds.tolist())) == [1, 2, 3]
    assert arm[0].any() == (case == "arm")
    if case == "arm":
        for g in rp.groups(n): assert arm[0, g].any()
    else:
        assert not arm.any()
    even = i % 2 == 0
    assert (np.abs(a[even][:, list(NARROW)]) > 0.5).any() and (a[:, 6] < 0).any() and (a[:, 6] > 0).any()      # beyond ctrlrange, both ends
    kp = np.array([-tab["actuators"][u]["biasprm"][1] for u in range(6)]); fr = np.array([tab["actuators"][u]["forcerange"][1] for u in range(6)])
    err = kp * np.abs(a[:, :6] - r["pre"][0]["qpos"][:, :6])
    assert (err[even] > 2 * fr).any(axis=0).all() and (err[~even] < 0.5 * fr).all()       # at the forcerange / well inside it
    assert not any(o["truncated"].any() or o["terminated"].any() for o in r["out"] + r["env_out"])


def _engine(n, frame_skip):
    return rp.engine(n, frame_skip, SEED, table=table())


def measure_substeps(case, n):
    """Worst errors over the twenty single sub-steps and the n lanes."""
    r = oracle_run(case, n)
    check_paths(case, n, r)
    return rp.measure_substeps(r, functools.partial(_engine, n), f"{case} ({n}) sub-steps")


def measure_env_steps(case, n):
    """Worst errors after the whole env-step over the n lanes."""
    return rp.measure_env_steps(oracle_run(case, n), functools.partial(_engine, n), f"{case} ({n}) env-steps")


def test_table_has_a_record_of_its_own_per_row_and_equality(built):
    """The specialised model: no two limit rows and no two equalities share a parameter record or (gear rows, connect sides) a diag."""
    from mycobotgym_amd.model.mjcf import _np_model
    from mycobotgym_amd.model.specialize import specialize
    m = specialize(_np_model(table()))
    lp, ep = np.asarray(m["limit_par"])[:10], np.asarray(m["eq_par"])
    rec = [tuple(x) for x in lp] + [tuple(x) for x in ep]
    assert len(set(rec)) == 13
    assert lp[6][6] == 1 and ep[1][6] == 1 and lp[8][2] == lp[8][3] and all(lp[j][6] == 2 for j in range(10) if j != 6)
    assert m["limit_diag"][6] != m["limit_diag"][8] and m["eq_diag"][0] != m["eq_diag"][1]


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_substeps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_substeps(case, n), SUB_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_env_steps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_env_steps(case, n), ENV_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)
