"""GPU parity of the split Reach kernels' remote constraint solve (SplitMainCols::cols) where it meets the other paths.

In a sub-step where no lane of a wave violates a limit row other than the gear joints' (dofs 6 and 8), the RNE wave builds and factors
H, solves for the acceleration and the two columns of the closed-form limit solve, and hands the acceleration to the main wave through
the warm-start slots, where the main wave left it the gear rows' numbers before that.  Any other violated row in the wave and the main
wave solves as it always did -- from a warm start that must still be the one the last Euler step left.  Three things the single
sub-steps of test_gpu_reach_limit_rows.py do not reach:

  1. an env-step (20 sub-steps) in which a workgroup goes remote -> main-wave solve -> remote, because arm joint 0 crosses its upper
     limit and comes back, once with at most two violated rows per lane (direct solve) and once with three in one lane (the general
     iteration, which reads the warm start);
  2. one sub-step whose wave mixes lanes with both gear rows, only row 6, only row 8 and none, at joint velocities up to +-10 rad/s on
     all twelve dofs, where passive - bias dominates the right-hand side the two waves now put together;
  3. one sub-step with a lane per workgroup that MuJoCo's checks reset (qvel = 1e12: reset when the step starts; qvel = 9e9: the
     acceleration of the sub-step itself is bad), next to lanes that must not notice.

Every state goes into the engine and the CPU oracle alike through set_state.  165 environments: two full workgroups and a ragged
third of 37 lanes, the special lanes in all three.
"""
import pytest

from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import MIXED_BOUNDS, check_bad_lanes, measure_mixed, measure_switch
from tests.reach_parity import within

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------- 1. remote -> main-wave solve -> remote in one env-step
@pytest.mark.parametrize("rows", ["direct", "general"])
def test_env_step_switches_paths_and_back(torch_cuda, rows):
    """Two lanes per workgroup start 0.02 rad inside arm joint 0's upper limit at about 8 rad/s: outside after two or three sub-steps,
    pulled back in by the limit row and the servo a few sub-steps later.  Every other lane sits below the gear joints' lower limit and
    is commanded to close, so gear rows exist in all twenty sub-steps.  `direct`: the crossing lanes' gear joints are inside their
    range (at most one row in those lanes); `general`: they are below it too -- three violated rows in one lane, the general iteration,
    whose warm start comes from slots that the remote sub-steps before it used for the hand-over.  That the sub-steps take the paths in
    this order is checked on a second oracle stepped one sub-step at a time."""
    worst, flags_equal = measure_switch(rows)
    assert flags_equal
    assert worst < 1e-8                                                             # smoke()'s 20-sub-step bound


# --------------------------------------------------------------------------------------------- 2. one sub-step, mixed lanes, fast dofs
@pytest.mark.parametrize("controller", sorted(MIXED_BOUNDS))
def test_substep_with_mixed_gear_rows(torch_cuda, controller):
    w, b = measure_mixed(controller), MIXED_BOUNDS[controller]
    assert within(w, b), (w, b)


# -------------------------------------------------------------------------------------------------- 3. a bad lane in a remote sub-step
def test_bad_lane_in_a_remote_substep(torch_cuda):
    """Lane 9 of every workgroup arrives with qvel = 1e12 on all twelve dofs: mj_checkVel resets it when the step starts, and the
    sub-step runs from qpos0 -- to the sub-step bounds against the oracle, like every ordinary lane.  Lane 50 (20 in the ragged
    workgroup) arrives with 9e9 rad/s on arm joint 1, which passes that check: the bias forces, the right-hand side and the solve of
    that lane overflow inside the RNE wave's remote solve, the main wave's checks on the new state catch it, and the lane leaves the
    sub-step as mj_resetData leaves it (the oracle then integrates one sub-step from there, the engine does with the next: the lag
    test_gpu_api_round2.py describes, so this lane is compared with the reset state, not with the oracle).  The sub-step is remote:
    gear rows in the other lanes, no other row."""
    check_bad_lanes()
