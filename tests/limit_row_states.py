"""Limit-row states of Reach beyond "gear joints, plus arm joint 0's upper limit", made by the CPU oracle alone (no GPU).

The ten limit rows are dofs 0 to 9: six arm hinges (+-2.96706), the gear joints 6 and 8 ([0, 0.7]) and the finger joints 7 and 9
(+-0.872664), which couple through the connects to the gear row of their side.  Two families, the same for the CPU conditions
(tests/test_reach_limit_states_cpu.py) and the GPU comparisons (tests/test_gpu_reach_limit_families.py, tests/test_gpu_reach_one_wave.py),
165 environments each: two full workgroups of 64 lanes and a ragged one of 37.

* `fingers`, by i % 5: 0 dof 7 above its upper limit; 1 dof 9 below its lower limit; 2 dof 7 below lower and dof 9 above upper (a pair with
  signs +1 / -1); 3 dof 6 below 0 and dof 7 above upper (a gear row and a finger row of the same side); 4 no row.  At most two rows per lane:
  every wave takes the direct solve, and its 2 x 2 enumeration sees pairs other than (6, 8).
* `many`, by i % 8: 3 dof 0 above upper, dof 3 below lower, dofs 6 and 8 below 0, dof 7 above upper (five rows); 6 dof 2 below lower, dof 5
  above upper, dof 9 below lower (three rows); every other lane none.  Every wave takes the general iteration, with lanes of 0, 3 and 5 rows.

Gear angles are uniform in [0.05, 0.3] where not stated, violation depths uniform in [1e-4, 5e-3] rad beyond the range, qvel[:, :10] uniform
in +-2 rad/s; the ranges are the jnt_range of the controller's own model table.  The base state is the one tests/reach_measures.py's limit_run
builds tests/test_gpu_reach_limit_rows.py's kinds on (it calls `put` for these two): reset(seed = 21), one random step, generator default_rng(5).

Nothing here is mutated after it is built (the arrays are read-only): the tests copy what they change."""
from __future__ import annotations

import functools

import numpy as np

from tests.common import load_json, make_oracle, table_name
from tests.reach_parity import N, freeze, groups

FAMILIES = ("fingers", "many")
CONTROLLERS = ("joint", "IK", "mocap")
GROUPS = tuple(groups(N))
SEED = 21
# (dof, side) of every row by lane class; side -1: below the lower limit, +1: above the upper one
ROWS = {
    "fingers": (5, {0: ((7, +1),), 1: ((9, -1),), 2: ((7, -1), (9, +1)), 3: ((6, -1), (7, +1))}),
    "many": (8, {3: ((0, +1), (3, -1), (6, -1), (8, -1), (7, +1)), 6: ((2, -1), (5, +1), (9, -1))}),
}


def jnt_range(controller):
    return np.array(load_json(table_name(False, "legacy", controller == "mocap"))["jnt_range"], dtype=np.float64)


def engine_kw(controller, frame_skip=1):
    """Keyword arguments of tests.common.make_pair / make_oracle, as tests/reach_measures.py's limit_run builds its pair."""
    kw = dict(controller_type=controller, reward_type="dense", seed=SEED, max_episode_steps=10 ** 9, frame_skip=frame_skip)
    if controller == "IK" and frame_skip == 1: kw["control_steps"] = 1
    return kw


def rows_per_lane(qpos, jr):
    """Violated limit rows of every lane, counted from the ranges: (number [n], row below its lower limit [n, 10], above its upper [n, 10])."""
    lo = qpos[:, :10] - jr[:10, 0] < 0
    hi = jr[:10, 1] - qpos[:, :10] < 0
    return (lo | hi).sum(axis=1), lo, hi


def put(ora, kind, rng, jr):
    """Write family `kind` into oracle `ora`'s current state (any number of lanes); returns the rows per lane."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    n = q.shape[0]
    i = np.arange(n)
    inside = rng.uniform(0.05, 0.3, (n, 2))
    depth = rng.uniform(1e-4, 5e-3, (n, 10))
    q[:, 6], q[:, 8] = inside[:, 0], inside[:, 1]
    mod, classes = ROWS[kind]
    for c, rows in classes.items():
        m = i % mod == c
        for j, side in rows:
            q[m, j] = jr[j, 0] - depth[m, j] if side < 0 else jr[j, 1] + depth[m, j]
    qd[:, :10] = rng.uniform(-2.0, 2.0, (n, 10))
    ora.set_state(qpos=q, qvel=qd)
    nrows, lo, hi = rows_per_lane(q, jr)
    want = np.zeros(n, np.int64)
    for c, rows in classes.items(): want[i % mod == c] = len(rows)
    assert np.array_equal(nrows, want), (kind, nrows, want)
    return nrows


@functools.lru_cache(maxsize=None)
def family_state(controller, kind):
    """Family `kind` under `controller` as limit_run reaches it, by the oracle alone: dict(state = the oracle's state arrays [165, ...], action = the
    float32 action limit_run steps it with, rows = violated rows per lane)."""
    ora = make_oracle(N, **engine_kw(controller))
    ora.reset(seed=SEED)
    rng = np.random.default_rng(5)
    ora.step(rng.uniform(-1, 1, (N, ora.act_dim)).astype(np.float32))
    a = rng.uniform(-1, 1, (N, ora.act_dim)).astype(np.float32)
    rows = put(ora, kind, rng, jnt_range(controller))
    return freeze(dict(state=ora.get_state(), action=a, rows=rows))


def twin_state_errors(twin, state, a, ora, o_ref, prng, eps=1e-14):
    """The oracle's own sensitivity on `state` and action `a`: `twin` steps from `state` with qpos +-eps on every column; returns its largest
    differences from oracle `ora`, which has stepped from `state` already with outputs `o_ref`, as dict(obs, q, v, w): the keys limit_run reports."""
    s = {k: v.copy() for k, v in state.items()}
    s["qpos"] = s["qpos"] + eps * np.sign(prng.normal(size=s["qpos"].shape))
    twin.set_state(**s)
    ot = twin.step(a)
    st, so = twin.get_state(), ora.get_state()
    return dict(obs=float(np.abs(ot["obs"] - o_ref["obs"]).max()), q=float(np.abs(st["qpos"] - so["qpos"]).max()),
                v=float(np.abs(st["qvel"] - so["qvel"]).max()), w=float(np.abs(st["warm"] - so["warm"]).max()))
