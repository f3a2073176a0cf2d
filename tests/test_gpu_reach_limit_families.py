"""GPU parity of the Reach kernels on the limit rows no other state reaches: finger rows, lower arm limits, pairs with a negative sign in
the direct solve's 2 x 2 enumeration, and the general iteration with five rows in a lane.

The states are the two families of tests/limit_row_states.py (`fingers`: at most two rows per lane, a non-gear row in every wave, so the main
wave's direct solve runs in the joint kernel too; `many`: lanes of 0, 3 and 5 rows in every wave, the general iteration and its line search),
whose contents tests/test_reach_limit_states_cpu.py pins on the oracle alone.  165 environments -- two full workgroups and a ragged one of 37
lanes, at most one workgroup per CU: the three-wave kernels (tests/test_gpu_reach_one_wave.py runs the same states on the one-wave kernels).

One sub-step (frame_skip = 1; IK with control_steps = 1) from identical state through tests/test_gpu_reach_limit_rows.py's _run, against the
CPU oracle, at that file's bounds (test_gpu_parity's and test_gpu_mocap's sub-step bounds; its `with_arm` case meets them at a 0.01 rad
violation), or 10 x the oracle's own sensitivity on the same states and actions where that is larger (a twin oracle started +-1e-14 away;
10 x is assert_within_oracle_sensitivity's factor).  On the CPU figures the bound itself is the larger of the two in every case.
"""
import pytest

from tests import limit_row_states as ls

pytestmark = pytest.mark.gpu

# obs, qpos, qvel, warm start: the joint controller's from test_gpu_parity, IK's and mocap's from test_gpu_mocap (which has none for warm)
SUBSTEP_BOUNDS = {"joint": dict(obs=1e-13, q=1e-12, v=3e-10, w=4e-8), "IK": dict(obs=3e-13, q=1e-10, v=4e-8), "mocap": dict(obs=3e-13, q=1e-10, v=4e-8)}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def assert_substep(w, controller):
    """_run(..., twin=True)'s figures against the sub-step bounds, each widened to 10 x the twin's figure where that is larger."""
    for k, bound in SUBSTEP_BOUNDS[controller].items():
        limit = max(bound, 10.0 * w["twin_" + k])
        assert w[k] <= limit, (controller, k, w[k], limit, w)
    assert w["bad_state_resets"] == 0


@pytest.mark.parametrize("controller", ls.CONTROLLERS)
@pytest.mark.parametrize("kind", ls.FAMILIES)
def test_substep_on_limit_families(torch_cuda, kind, controller):
    from tests.test_gpu_reach_limit_rows import _run
    assert_substep(_run(controller, kind, 1, twin=True), controller)          # flags_equal is asserted inside _run


def test_joint_env_step_on_many_rows(torch_cuda):
    from tests.test_gpu_reach_limit_rows import _run
    w = _run("joint", "many", 20)
    assert w["obs"] < 1e-8                                                     # smoke()'s 20-sub-step bound
