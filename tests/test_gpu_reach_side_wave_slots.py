"""GPU parity of the joint controller's three-wave Reach kernel (SplitMainCols) where its side waves address the lane's column through
windows: the sine / cosine exchange of all three waves, the RNE wave's q, qd, passive - bias and its remote solve (H_eq's upper rows,
the main wave's parked actuation forces and g0, abar), the helper wave's H and its stores of the gear rows' columns.

A wrong window base or a slot served by the wrong window reads or writes another slot of the column, so every state below makes each
of those slots matter, and is run twice against the CPU oracle: the env-step's twenty sub-steps one at a time (frame_skip = 1, the
oracle's state before each sub-step put into the engine through set_state, compared after it), and whole env-steps (frame_skip = 20)
from the state the first sub-step started from -- two of them in `reset`, whose first ends in a truncation and an auto-reset.

  none         no gear row: every sub-step remote, abar is the acceleration;
  row6, row8   one gear row per lane;
  both_lower, both_upper   both gear rows, at either limit;
  arm          two lanes per workgroup start beyond arm joint 0's upper limit: the RNE wave skips its solve and the main wave reads
               LDS_RG0 / LDS_RACT back, from the first sub-step on;
  switch       two lanes per workgroup cross that limit and come back: remote -> main-wave solve -> remote in one workgroup;
  reset        sub-steps: the tenth truncates and auto-resets a fifth of the lanes (test_gpu_reach_after_s3.py's case); env-steps: the
               first env-step does, the second runs the fresh lanes next to running ones.

165 environments (two full workgroups and a ragged one of 37 lanes), `mixed` once more at 65.  The states are those of
tests/test_gpu_reach_after_s3.py (tests/reach_parity.py's put_gear_case), `arm` added on top; tests/reach_measures.py makes and measures them
(slot_oracle_run; tests/test_gpu_reach_factor_order.py runs them too), each case's oracle once per session.

Compared: observation (with achieved goal and reward), qpos, qvel absolute, the warm start (= qacc) relative to the lane's largest |qacc|
(absolute where that is zero).  Bounds: 100 x the worst error of the build this change started from (every wave addressing its column from
slot 0), measured on an MI355X on these very states in one run of this file's measure functions (profiles/r11/side_wave_tests_parent.log);
the measured figures are in the comments.
"""
import pytest

from tests import reach_parity as rp
from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import SLOT_RUNS as RUNS, measure_slot_env_steps, measure_slot_substeps
from tests.reach_parity import N

pytestmark = pytest.mark.gpu

SUB_BOUNDS = {      # single sub-steps: obs, q, v, w = 100 x the parent build's worst error (the measured figures in the comment)
    ("none", N): dict(obs=7.772e-14, q=8.162e-12, v=4.081e-09, w=4.353e-11),                # 7.772e-16  8.162e-14  4.081e-11  4.353e-13
    ("row6", N): dict(obs=5.551e-14, q=8.563e-12, v=4.282e-09, w=4.693e-11),                # 5.551e-16  8.563e-14  4.282e-11  4.693e-13
    ("row8", N): dict(obs=4.996e-14, q=8.632e-12, v=4.317e-09, w=4.046e-11),                # 4.996e-16  8.632e-14  4.317e-11  4.046e-13
    ("both_lower", N): dict(obs=5.551e-14, q=1.823e-13, v=9.116e-11, w=4.663e-11),          # 5.551e-16  1.823e-15  9.116e-13  4.663e-13
    ("both_upper", N): dict(obs=5.551e-14, q=9.628e-12, v=4.813e-09, w=3.359e-11),          # 5.551e-16  9.628e-14  4.813e-11  3.359e-13
    ("arm", N): dict(obs=7.216e-14, q=1.317e-11, v=6.585e-09, w=4.004e-11),                 # 7.216e-16  1.317e-13  6.585e-11  4.004e-13
    ("switch", N): dict(obs=6.939e-14, q=9.420e-12, v=4.711e-09, w=4.222e-11),              # 6.939e-16  9.420e-14  4.711e-11  4.222e-13
    ("reset", N): dict(obs=1.221e-13, q=6.950e-12, v=3.475e-09, w=4.392e-11),               # 1.221e-15  6.950e-14  3.475e-11  4.392e-13
    ("mixed", 65): dict(obs=7.216e-14, q=6.734e-12, v=3.368e-09, w=3.365e-11),              # 7.216e-16  6.734e-14  3.368e-11  3.365e-13
}
ENV_BOUNDS = {      # whole env-steps: likewise
    ("none", N): dict(obs=2.290e-11, q=1.870e-11, v=3.243e-09, w=4.352e-10),                # 2.290e-13  1.870e-13  3.243e-11  4.352e-12
    ("row6", N): dict(obs=3.239e-11, q=2.552e-11, v=4.008e-09, w=1.104e-09),                # 3.239e-13  2.552e-13  4.008e-11  1.104e-11
    ("row8", N): dict(obs=9.566e-12, q=9.176e-12, v=1.630e-09, w=5.113e-10),                # 9.566e-14  9.176e-14  1.630e-11  5.113e-12
    ("both_lower", N): dict(obs=2.241e-11, q=1.221e-11, v=2.792e-09, w=2.518e-10),          # 2.241e-13  1.221e-13  2.792e-11  2.518e-12
    ("both_upper", N): dict(obs=4.006e-11, q=1.077e-11, v=4.034e-09, w=2.686e-09),          # 4.006e-13  1.077e-13  4.034e-11  2.686e-11
    ("arm", N): dict(obs=1.643e-11, q=1.516e-11, v=1.875e-09, w=2.868e-10),                 # 1.643e-13  1.516e-13  1.875e-11  2.868e-12
    ("switch", N): dict(obs=6.636e-12, q=4.283e-12, v=1.659e-09, w=1.960e-10),              # 6.636e-14  4.283e-14  1.659e-11  1.960e-12
    ("reset", N): dict(obs=1.298e-09, q=3.487e-09, v=1.644e-07, w=6.491e-08),               # 1.298e-11  3.487e-11  1.644e-09  6.491e-10
    ("mixed", 65): dict(obs=6.361e-12, q=3.897e-12, v=8.023e-10, w=9.548e-11),              # 6.361e-14  3.897e-14  8.023e-12  9.548e-13
}


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_substeps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_slot_substeps(case, n), SUB_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)


@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_env_steps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_slot_env_steps(case, n), ENV_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)
