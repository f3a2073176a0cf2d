"""GPU parity of one Reach sub-step on fast, wide states: the pieces whose inputs change waves in the split Reach kernels.

Since round 6 the three waves of a split Reach workgroup evaluate each joint's sine and cosine once and exchange them through LDS
(SplitMainLocal::reach, trig_exchange): everything downstream -- M from the composite pass, the Coriolis / centrifugal bias, the connect rows -- is
built from values another wave computed.  (The round also tried a fourth wave for the gripper dofs' rows of M; DESIGN.md section 5
says why it was left out.  The file keeps the name the round's plan gave it.)  The existing per-sub-step parity tests run near the
reset pose at servo speeds, where gravity and actuation dominate qacc.  Here the arm angles are uniform within 98 % of their ranges
and the joint velocities are drawn up to +-10 rad/s -- on the six arm dofs, and again on all twelve -- so that the bias and the
gripper <-> arm entries of M dominate: |qacc| reaches 6e3 (mocap 2e4).  One sub-step (frame_skip = 1) from identical state, joint /
IK / mocap, against the CPU oracle; 165 environments: two full workgroups and a ragged third of 37 lanes.  No lane may leave the
comparison through a reset (mj_checkPos / Vel / Acc), on either side.

Bounds: 100 x the error of the build this change started from (every wave its own twelve sincos), measured on an MI355X on these
very states -- the measured figure is written next to each bound.  qpos / qvel / observation are absolute; the warm start (= qacc)
is relative to the lane's largest |qacc|.
"""
import pytest

from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import FAST_WIDE_BOUNDS as BOUNDS, measure_fast_wide
from tests.reach_parity import within

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("all_dofs", [False, True], ids=["arm", "all"])
@pytest.mark.parametrize("controller", ["joint", "IK", "mocap"])
def test_substep_on_fast_wide_states(torch_cuda, controller, all_dofs):
    w, b = measure_fast_wide(controller, all_dofs), BOUNDS[controller, all_dofs]
    assert within(w, b), (w, b)
