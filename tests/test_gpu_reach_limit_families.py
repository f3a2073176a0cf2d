"""GPU parity of the Reach kernels on the limit rows no other state reaches: finger rows, lower arm limits, pairs with a negative sign in
the direct solve's 2 x 2 enumeration, and the general iteration with five rows in a lane.

The states are the two families of tests/limit_row_states.py (`fingers`: at most two rows per lane, a non-gear row in every wave, so the main
wave's direct solve runs in the joint kernel too; `many`: lanes of 0, 3 and 5 rows in every wave, the general iteration and its line search),
whose contents tests/test_reach_limit_states_cpu.py pins on the oracle alone.  165 environments -- two full workgroups and a ragged one of 37
lanes, at most one workgroup per CU: the three-wave kernels (tests/test_gpu_reach_one_wave.py runs the same states on the one-wave kernels).

One sub-step (frame_skip = 1; IK with control_steps = 1) from identical state through tests/reach_measures.py's limit_run, against the
CPU oracle, at tests/test_gpu_reach_limit_rows.py's bounds (test_gpu_parity's and test_gpu_mocap's sub-step bounds, SUBSTEP_BOUNDS of
tests/reach_measures.py; its `with_arm` case meets them at a 0.01 rad violation), or 10 x the oracle's own sensitivity on the same states
and actions where that is larger (a twin oracle started +-1e-14 away; 10 x is assert_within_oracle_sensitivity's factor).  On the CPU figures the bound itself is the larger of the two in every case.
"""
import pytest

from tests import limit_row_states as ls
from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import assert_substep, limit_run

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("controller", ls.CONTROLLERS)
@pytest.mark.parametrize("kind", ls.FAMILIES)
def test_substep_on_limit_families(torch_cuda, kind, controller):
    assert_substep(limit_run(controller, kind, 1, twin=True), controller)     # flags_equal is asserted inside limit_run


def test_joint_env_step_on_many_rows(torch_cuda):
    w = limit_run("joint", "many", 20)
    assert w["obs"] < 1e-8                                                     # smoke()'s 20-sub-step bound
