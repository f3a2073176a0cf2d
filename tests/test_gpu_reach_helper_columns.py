"""GPU parity of the joint controller's three-wave Reach kernel with the gear rows' columns on the helper wave (SplitMainCols::cols).

Between the barriers S2 and S3 of every sub-step the helper wave factors H and solves the columns z6 = H^-1 e_6, z8 = H^-1 e_8 into 24
slots of the factor region, the RNE wave's remote solve ends at the unconstrained acceleration, and the main wave factors M + hB
itself; after S3 the main wave finishes the gear rows from the columns -- in a remote sub-step with a gear row in some lane of the wave,
and in no other.  Whole env-steps (20 sub-steps each) that the single sub-steps of test_gpu_reach_remote_solve.py do not reach:

  a. lanes with both gear rows, row 6 only, row 8 only and none, mixed within every wave, the gripper commanded to close in some lanes
     and to open in others: the first and the ragged workgroup read the columns in all twenty sub-steps, the second one (every lane
     opening) in the first sub-steps only -- the slots are written in every sub-step, next to the sine / cosine exchange;
  b. the same with two lanes per workgroup driven across arm joint 0's upper limit and back: remote -> main-wave solve -> remote.  In
     the sub-steps between, the main wave must still come out with a valid factor of M + hB, after its own solve, and the helper's
     columns must be ignored;
  c. three env-steps with max_episode_steps = 50 and elapsed = 48 in some lanes (49 when the middle step starts): the middle step
     truncates and auto-resets them, and the last one runs freshly reset lanes, which sit on both gear limits, next to running ones.

Every state goes into the engine and the CPU oracle alike through set_state.  165 environments: two full workgroups and a ragged
third of 37 lanes.  The bounds are 100 x the errors of the build this change started from (round 7: columns and gear rows on the RNE
wave, the factor of M + hB on the helper wave), measured on an MI355X on these very states; the measured figures are in the comments.
qpos / qvel / observation absolute, the warm start (= qacc) relative to the lane's largest |qacc|.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 165
ARM_HI = 2.96706                                     # jnt_range[0][1] of the mycobot280 tables; the gear joints' range is [0, 0.7]
GEAR_HI, FINGER_HI = 0.7, 0.872664
GROUPS = [slice(0, 64), slice(64, 128), slice(128, N)]

BOUNDS = {
    "mixed": dict(obs=5.7e-11, q=9.9e-11, v=1.3e-08, w=5.1e-10),      # 5.732e-13  9.947e-13  1.380e-10  5.174e-12
    "cross": dict(obs=5.7e-11, q=9.9e-11, v=1.3e-08, w=5.1e-10),      # 5.732e-13  9.947e-13  1.380e-10  5.174e-12 (the worst lane does not cross)
    "reset": dict(obs=1.7e-06, q=6.0e-06, v=1.8e-04, w=1.1e-05),      # 1.724e-08  6.089e-08  1.805e-06  1.116e-07 (three free-running env-steps)
}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _pair(seed, max_episode_steps=10 ** 9):
    """Engine and oracle after a reset and one ordinary step: warm start, lagged q and ctrl are those of a running episode."""
    from tests.common import make_pair, step_errors, sync_oracle_to
    envs, ora = make_pair(N, controller_type="joint", reward_type="dense", seed=seed, max_episode_steps=max_episode_steps, frame_skip=20)
    envs.reset(seed=seed); ora.reset(seed=seed)
    rng = np.random.default_rng(seed)
    sync_oracle_to(envs, ora)
    _, flags_equal, _ = step_errors(envs, ora, rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32))
    assert flags_equal
    return envs, ora, rng


def _state_errors(envs, ora):
    st, so = envs.get_state(), ora.get_state()
    gq, gv, gw = (st[k].cpu().numpy().T for k in ("qpos", "qvel", "warm"))
    assert all(np.isfinite(x).all() for x in (gq, gv, gw, so["qpos"], so["qvel"], so["warm"]))
    w = np.abs(gw - so["warm"]).max(axis=1) / np.abs(so["warm"]).max(axis=1)
    return float(np.abs(gq - so["qpos"]).max()), float(np.abs(gv - so["qvel"]).max()), float(w.max())


def _mixed_gear_state(ora, rng, cross):
    """Both rows / row 6 / row 8 / none by lane % 4; lanes close or open by (lane // 4) % 2, the second workgroup opens everywhere.
    `cross`: lanes 5 and 30 of every workgroup start 0.02 rad inside arm joint 0's upper limit at about 8 rad/s."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(N)
    below = -rng.uniform(1e-3, 5e-3, (N, 2)); inside = rng.uniform(0.05, 0.3, (N, 2))
    q[:, 6] = np.where((i % 4 == 0) | (i % 4 == 1), below[:, 0], inside[:, 0])
    q[:, 8] = np.where((i % 4 == 0) | (i % 4 == 2), below[:, 1], inside[:, 1])
    a = rng.uniform(-1, 1, (N, 7)).astype(np.float32)
    a[:, 6] = np.where((i // 4) % 2 == 1, 1.0, -1.0)
    a[GROUPS[1], 6] = 1.0
    if cross:
        c = (i % 64 == 5) | (i % 64 == 30)
        q[c, 0] = ARM_HI - 0.02; qd[c, 0] = rng.uniform(7.5, 8.5, int(c.sum())); a[c, 0] = 1.0
    ora.set_state(qpos=q, qvel=qd)
    return a


def _substep_paths(ora, a, seed):
    """Per sub-step and workgroup, from a twin oracle stepped with frame_skip = 1 (the joint controller writes the same ctrl in every
    env-step): does some lane hold an arm row (the main wave solves), a gear row (the columns are read)?"""
    from tests.common import make_oracle
    twin = make_oracle(N, controller_type="joint", reward_type="dense", seed=seed, max_episode_steps=10 ** 9, frame_skip=1)
    twin.reset(seed=seed); twin.set_state(**ora.get_state())
    arm, gear = np.zeros((20, 3), bool), np.zeros((20, 3), bool)
    for k in range(20):
        tq = twin.get_state()["qpos"]
        assert not (np.abs(tq[:, [7, 9]]) > FINGER_HI).any()                        # no finger row: the arm rows alone switch the path
        out = (np.abs(tq[:, :6]) > ARM_HI).any(axis=1)
        row = (tq[:, 6] < 0) | (tq[:, 8] < 0) | (tq[:, 6] > GEAR_HI) | (tq[:, 8] > GEAR_HI)
        for g, sl in enumerate(GROUPS):
            arm[k, g] = out[sl].any(); gear[k, g] = row[sl].any()
        twin.step(a)
    return arm, gear


def measure_env_step(cross):
    """Worst errors of one env-step over the 165 lanes: dict(obs, q, v, w)."""
    from tests.common import step_errors, sync_oracle_to
    seed = 51
    envs, ora, rng = _pair(seed)
    a = _mixed_gear_state(ora, rng, cross)
    arm, gear = _substep_paths(ora, a, seed)
    show = lambda m: " | ".join("".join("X" if x else "." for x in m[:, g]) for g in range(3))
    print(f"\nsub-steps with an arm row, per workgroup: {show(arm)}\nsub-steps with a gear row, per workgroup: {show(gear)}")
    assert gear[:, 0].all() and gear[:, 2].all()                                     # columns read in every sub-step ...
    assert gear[0, 1] and not gear[10:, 1].any()                                     # ... and in the first ones only
    for g in range(3):
        if cross:                                                                    # remote, main wave, remote again
            k_out = np.nonzero(arm[:, g])[0]
            assert not arm[0, g] and k_out.size and k_out[0] >= 2 and k_out[-1] <= 17, (g, k_out)
        else:
            assert not arm[:, g].any()                                               # twenty remote sub-steps
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    e, flags_equal, _ = step_errors(envs, ora, a)
    assert flags_equal
    eq, ev, ew = _state_errors(envs, ora)
    assert envs.counters()["bad_state_resets"] == 0
    envs.close()
    w = dict(obs=float(e.max()), q=eq, v=ev, w=ew)
    print(f"{'cross' if cross else 'mixed'}: " + " ".join(f"{k} {v:.3e}" for k, v in w.items()))
    return w


def measure_auto_reset():
    """Worst errors over three free-running env-steps (observation: of all three; state: after the last): dict(obs, q, v, w)."""
    from tests.common import step_errors, sync_oracle_to
    envs, ora, rng = _pair(53, max_episode_steps=50)
    i = np.arange(N)
    late = i % 5 == 2                                                                # in all three workgroups, next to running lanes
    s = ora.get_state()
    el = s["elapsed"].copy(); el[late] = 48
    ora.set_state(elapsed=el)
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    worst = 0.0
    for t in range(3):
        a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
        a[:, 6] = np.where((i // 4) % 2 == 1, 1.0, -1.0)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal, t
        assert np.array_equal(o["truncated"].astype(bool), late if t == 1 else np.zeros(N, bool)), t      # the reset lands in the middle step
        worst = max(worst, float(e.max()))
    so = ora.get_state()
    assert (so["elapsed"][late] == 1).all() and (so["elapsed"][~late] == 4).all()
    eq, ev, ew = _state_errors(envs, ora)
    assert envs.counters()["bad_state_resets"] == 0
    envs.close()
    w = dict(obs=worst, q=eq, v=ev, w=ew)
    print("\nreset: " + " ".join(f"{k} {v:.3e}" for k, v in w.items()))
    return w


def _within(w, b):
    assert w["obs"] <= b["obs"] and w["q"] <= b["q"] and w["v"] <= b["v"] and w["w"] <= b["w"], (w, b)


def test_env_step_with_mixed_gear_rows(torch_cuda):
    _within(measure_env_step(False), BOUNDS["mixed"])


def test_env_step_leaves_the_remote_path_and_returns(torch_cuda):
    _within(measure_env_step(True), BOUNDS["cross"])


def test_auto_reset_in_the_middle_of_three_env_steps(torch_cuda):
    _within(measure_auto_reset(), BOUNDS["reset"])
