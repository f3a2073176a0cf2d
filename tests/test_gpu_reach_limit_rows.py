"""GPU parity of the Reach kernels' closed-form limit solve on states built to exercise each of its paths.

When the only violated limit rows of a wave are the gear joints' (dofs 6 and 8, whose lower limit is their qpos0), the RNE wave
solves for the two columns H^-1 e_6, H^-1 e_8 and hands them to the main wave at an extra barrier; any other limit row in the
wave sends it through the general block.  Every state goes in through set_state, into the engine and the CPU oracle alike, and
one sub-step (frame_skip = 1) or one env-step is compared at the bounds of the existing parity tests.  165 environments: two
full workgroups and a ragged third of 37 lanes, flagged lanes in all three.
"""
import pytest

from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import limit_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kind", ["gear_pair", "gear6", "with_arm", "none"])
def test_joint_substep_on_limit_states(torch_cuda, kind):
    w = limit_run("joint", kind, 1)
    assert w["obs"] < 1e-13 and w["q"] < 1e-12 and w["v"] < 3e-10 and w["w"] < 4e-8       # test_gpu_parity's sub-step bounds


@pytest.mark.parametrize("controller", ["IK", "mocap"])
@pytest.mark.parametrize("kind", ["gear_pair", "gear6", "with_arm", "none"])
def test_ik_mocap_substep_on_limit_states(torch_cuda, controller, kind):
    w = limit_run(controller, kind, 1)
    assert w["obs"] < 3e-13 and w["q"] < 1e-10 and w["v"] < 4e-8                         # test_gpu_mocap's sub-step bounds


@pytest.mark.parametrize("kind", ["gear_pair", "with_arm"])
def test_joint_env_step_on_limit_states(torch_cuda, kind):
    w = limit_run("joint", kind, 20)
    assert w["obs"] < 1e-8                                                                  # smoke()'s 20-sub-step bound
