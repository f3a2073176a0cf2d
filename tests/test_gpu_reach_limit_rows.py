"""GPU parity of the Reach kernels' closed-form limit solve on states built to exercise each of its paths.

When the only violated limit rows of a wave are the gear joints' (dofs 6 and 8, whose lower limit is their qpos0), the RNE wave
solves for the two columns H^-1 e_6, H^-1 e_8 and hands them to the main wave at an extra barrier; any other limit row in the
wave sends it through the general block.  Every state goes in through set_state, into the engine and the CPU oracle alike, and
one sub-step (frame_skip = 1) or one env-step is compared at the bounds of the existing parity tests.  165 environments: two
full workgroups and a ragged third of 37 lanes, flagged lanes in all three.
"""
import numpy as np
import pytest

from tests import limit_row_states as ls

pytestmark = pytest.mark.gpu

N = 165
GEAR_LO, GEAR_HI, ARM_HI = 0.0, 0.7, 2.96706        # jnt_range of dofs 6 / 8 and of arm joint 0 (mycobot280 tables)


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _state(ora, kind, rng, controller="joint"):
    """The oracle's state after a reset and two random steps, with the gear / arm angles of `kind` written into qpos.  The families of
    tests/limit_row_states.py (finger rows, lower arm limits, five rows in a lane) are written by that module, on `controller`'s ranges."""
    if kind in ls.FAMILIES:
        ls.put(ora, kind, rng, ls.jnt_range(controller))                 # asserts its own census
        q = ora.get_state()["qpos"]
        return int((q[:, 6] < GEAR_LO).sum()), int((q[:, 8] < GEAR_LO).sum())
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(q.shape[0])
    inside = rng.uniform(0.05, 0.3, (q.shape[0], 2))
    below = -rng.uniform(1e-4, 5e-3, (q.shape[0], 2))
    q[:, 6], q[:, 8] = inside[:, 0], inside[:, 1]
    if kind in ("gear_pair", "with_arm"):
        both, only6, only8 = i % 3 == 0, i % 3 == 1, i % 5 == 2
        q[both, 6], q[both, 8] = below[both, 0], below[both, 1]
        q[only6 & ~both, 6] = below[only6 & ~both, 0]
        q[only8 & ~both & ~only6, 8] = below[only8 & ~both & ~only6, 1]
    elif kind == "gear6":
        m = i % 2 == 0
        q[m, 6] = below[m, 0]
    if kind == "with_arm":                          # one lane per workgroup past arm joint 0's upper limit: the general block
        q[i % 64 == 5, 0] = ARM_HI + 0.01
    qd[:, 6] = rng.uniform(-2.0, 2.0, q.shape[0]); qd[:, 8] = rng.uniform(-2.0, 2.0, q.shape[0])
    ora.set_state(qpos=q, qvel=qd)
    n6 = int((q[:, 6] < GEAR_LO).sum()); n8 = int((q[:, 8] < GEAR_LO).sum())
    return n6, n8


def _run(controller, kind, frame_skip, twin=False):
    """Worst errors against the oracle over the step from the `kind` state and the one after it: dict(obs, q, v, w).  `twin`: also the
    oracle's own sensitivity on the same states and actions (a second oracle started +-1e-14 away on qpos), under the keys twin_obs, twin_q,
    twin_v, twin_w; and the engine's bad-state counter over the two steps under `bad_state_resets`."""
    from tests.common import make_oracle, make_pair, sync_oracle_to, step_errors
    kw = dict(controller_type=controller, reward_type="dense", seed=21, max_episode_steps=10 ** 9, frame_skip=frame_skip)
    if controller == "IK" and frame_skip == 1: kw["control_steps"] = 1
    envs, ora = make_pair(N, **kw)
    envs.reset(seed=21); ora.reset(seed=21)
    rng = np.random.default_rng(5)
    worst = dict(obs=0.0, q=0.0, v=0.0, w=0.0)
    if twin:
        two = make_oracle(N, **kw); two.reset(seed=21)
        prng = np.random.default_rng(7)
        worst.update(twin_obs=0.0, twin_q=0.0, twin_v=0.0, twin_w=0.0)
    for t in range(3):
        a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
        if t == 1:
            n6, n8 = _state(ora, kind, rng, controller)
            if kind == "none": assert n6 == 0 and n8 == 0
            elif kind not in ls.FAMILIES: assert n6 > 0 and (kind == "gear6" or n8 > 0)
            if twin: envs.counters(clear=True)
        sync_oracle_to(envs, ora)
        before = ora.get_state() if twin and t > 0 else None
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        if t == 0: continue
        if twin:
            for k, v in ls.twin_state_errors(two, before, a, ora, o, prng).items(): worst["twin_" + k] = max(worst["twin_" + k], v)
        st, so = envs.get_state(), ora.get_state()
        worst["obs"] = max(worst["obs"], float(e.max()))
        worst["q"] = max(worst["q"], float(np.abs(st["qpos"].cpu().numpy().T - so["qpos"]).max()))
        worst["v"] = max(worst["v"], float(np.abs(st["qvel"].cpu().numpy().T - so["qvel"]).max()))
        worst["w"] = max(worst["w"], float(np.abs(st["warm"].cpu().numpy().T - so["warm"]).max()))
    if twin: worst["bad_state_resets"] = envs.counters()["bad_state_resets"]
    envs.close()
    print(f"\n{controller} {kind} frame_skip={frame_skip}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


@pytest.mark.parametrize("kind", ["gear_pair", "gear6", "with_arm", "none"])
def test_joint_substep_on_limit_states(torch_cuda, kind):
    w = _run("joint", kind, 1)
    assert w["obs"] < 1e-13 and w["q"] < 1e-12 and w["v"] < 3e-10 and w["w"] < 4e-8       # test_gpu_parity's sub-step bounds


@pytest.mark.parametrize("controller", ["IK", "mocap"])
@pytest.mark.parametrize("kind", ["gear_pair", "gear6", "with_arm", "none"])
def test_ik_mocap_substep_on_limit_states(torch_cuda, controller, kind):
    w = _run(controller, kind, 1)
    assert w["obs"] < 3e-13 and w["q"] < 1e-10 and w["v"] < 4e-8                         # test_gpu_mocap's sub-step bounds


@pytest.mark.parametrize("kind", ["gear_pair", "with_arm"])
def test_joint_env_step_on_limit_states(torch_cuda, kind):
    w = _run("joint", kind, 20)
    assert w["obs"] < 1e-8                                                                  # smoke()'s 20-sub-step bound
