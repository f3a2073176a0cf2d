"""The conditions of tests/test_gpu_reach_limit_families.py and tests/test_gpu_reach_one_wave.py, checked on the CPU oracle alone (no GPU):

* the states of tests/limit_row_states.py hold the rows they are meant to hold, counted from the controller's own jnt_range: `fingers` 33 / 66
  / 66 lanes with 0 / 1 / 2 rows and none with more (the direct solve in every wave), `many` 124 / 20 / 21 lanes with 0 / 3 / 5 rows, lanes of
  three or more rows in all three workgroups (the general iteration in every wave);
* one sub-step from them raises no bad-state warning and stays finite;
* on `many` the oracle's own Newton iteration needs three or more iterations in some lane of every workgroup: the active set moves, the line
  search is walked;
* the oracle's own sensitivity on these very states and actions -- a twin oracle started +-1e-14 away on qpos -- stays at or below the
  sub-step bounds the GPU files assert, so those bounds are the kernels' to use up, not the reference's.

Measured when the tests were written (the oracle is built for the host's CPU: last digits may differ elsewhere), max over the 165 lanes:

  family   controller  lanes at solver_iter 1 / 2 / 3 / 4   max |qacc|   twin obs   qpos      qvel      warm
  fingers  joint        85 / 80 / 0 / 0                     6.8e4        1.1e-14    6.9e-14   3.4e-11   3.3e-9
  fingers  IK           69 / 96 / 0 / 0                     6.7e4        1.1e-14    8.6e-14   3.8e-11   3.8e-9
  fingers  mocap        71 / 94 / 0 / 0                     7.0e4        1.1e-14    1.2e-13   6.6e-11   5.0e-9
  many     joint       130 / 26 / 6 / 3                     6.9e4        1.2e-14    5.4e-14   3.0e-11   3.3e-9
  many     IK          130 / 27 / 5 / 3                     7.1e4        1.1e-14    7.3e-14   4.2e-11   3.4e-9
  many     mocap       128 / 27 / 8 / 2                     6.9e4        2.1e-14    2.6e-13   1.3e-10   3.1e-8

(profiles/reach_one_wave/t_cpu.log.)  The sub-step bounds: joint obs 1e-13, qpos 1e-12, qvel 3e-10, warm 4e-8; IK and mocap obs 3e-13, qpos
1e-10, qvel 4e-8 (no warm-start bound).  The census is exact, the iteration counts are asserted as conditions (three or more in every
workgroup of `many`), not as these numbers.
"""
import numpy as np
import pytest

from tests import limit_row_states as ls
from tests.common import make_oracle

# the sub-step bounds of tests/test_gpu_reach_limit_rows.py (from test_gpu_parity / test_gpu_mocap)
BOUNDS = {"joint": dict(obs=1e-13, q=1e-12, v=3e-10, w=4e-8), "IK": dict(obs=3e-13, q=1e-10, v=4e-8), "mocap": dict(obs=3e-13, q=1e-10, v=4e-8)}
CENSUS = {"fingers": {0: 33, 1: 66, 2: 66}, "many": {0: 124, 3: 20, 5: 21}}


@pytest.mark.parametrize("controller", ls.CONTROLLERS)
@pytest.mark.parametrize("kind", ls.FAMILIES)
def test_family_census_iterations_and_sensitivity(kind, controller):
    fam = ls.family_state(controller, kind)
    state, a = fam["state"], fam["action"]
    jr = ls.jnt_range(controller)
    nrows, lo, hi = ls.rows_per_lane(state["qpos"], jr)
    census = {int(k): int((nrows == k).sum()) for k in np.unique(nrows)}
    assert census == CENSUS[kind], census
    assert np.array_equal(nrows, fam["rows"])
    depth = np.where(lo, jr[:10, 0] - state["qpos"][:, :10], 0) + np.where(hi, state["qpos"][:, :10] - jr[:10, 1], 0)
    assert depth[lo | hi].min() >= 1e-4 - 1e-15 and depth[lo | hi].max() <= 5e-3 + 1e-15
    assert np.abs(state["qvel"][:, :10]).max() <= 2.0
    if kind == "fingers":
        assert lo[:, 9].any() and hi[:, 9].any() and lo[:, 7].any() and hi[:, 7].any() and (lo[:, 6] & hi[:, 7]).any()
        assert not lo[:, 8].any() and not (lo | hi)[:, :6].any()
    else:
        assert all((nrows[g] >= 3).any() and (nrows[g] == 5).any() and (nrows[g] == 0).any() for g in ls.GROUPS)
        assert lo[:, :6].any() and hi[:, :6].any()                       # a lower arm limit too

    kw = ls.engine_kw(controller)
    ora, twin = make_oracle(ls.N, **kw), make_oracle(ls.N, **kw)
    ora.reset(seed=ls.SEED); twin.reset(seed=ls.SEED)
    ora.set_state(**{k: v.copy() for k, v in state.items()})
    o = ora.step(a)
    iters = np.array([int(ora.data(i).get("solver_iter", (1,), np.int32)[0]) for i in range(ls.N)])
    warn = np.array([int(ora.data(i).get("warning_badstate", (1,), np.int32)[0]) for i in range(ls.N)])
    so = ora.get_state()
    assert all(np.isfinite(so[k]).all() for k in ("qpos", "qvel", "warm")) and np.isfinite(o["obs"]).all()
    t = ls.twin_state_errors(twin, state, a, ora, o, np.random.default_rng(7))
    hist = {int(k): int((iters == k).sum()) for k in np.unique(iters)}
    print(f"\n[{kind} {controller}] rows per lane {census}; solver_iter histogram {hist}, per workgroup max "
          f"{[int(iters[g].max()) for g in ls.GROUPS]}; max |qacc| {np.abs(so['warm']).max():.2e}; bad-state warnings {int(warn.sum())}; "
          "twin (+-1e-14 on qpos) " + " ".join(f"{k} {v:.2e}" for k, v in t.items()))
    assert not warn.any()
    if kind == "many":
        assert all(iters[g].max() >= 3 for g in ls.GROUPS), hist
    b = BOUNDS[controller]
    assert all(t[k] <= b[k] for k in b), (t, b)
