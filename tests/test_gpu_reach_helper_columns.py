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

from tests import reach_parity as rp
from tests.common import step_errors, sync_oracle_to, torch_cuda  # noqa: F401
from tests.reach_parity import ARM_HI, N

pytestmark = pytest.mark.gpu

BOUNDS = {
    "mixed": dict(obs=5.7e-11, q=9.9e-11, v=1.3e-08, w=5.1e-10),      # 5.732e-13  9.947e-13  1.380e-10  5.174e-12
    "cross": dict(obs=5.7e-11, q=9.9e-11, v=1.3e-08, w=5.1e-10),      # 5.732e-13  9.947e-13  1.380e-10  5.174e-12 (the worst lane does not cross)
    "reset": dict(obs=1.7e-06, q=6.0e-06, v=1.8e-04, w=1.1e-05),      # 1.724e-08  6.089e-08  1.805e-06  1.116e-07 (three free-running env-steps)
}


def _state_errors(envs, ora):
    eq, ev, ew, _ = rp.state_errors(envs, ora, relative_warm=True)
    return float(eq.max()), float(ev.max()), float(ew.max())


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
    a[rp.groups(N)[1], 6] = 1.0
    if cross:
        c = (i % 64 == 5) | (i % 64 == 30)
        q[c, 0] = ARM_HI - 0.02; qd[c, 0] = rng.uniform(7.5, 8.5, int(c.sum())); a[c, 0] = 1.0
    ora.set_state(qpos=q, qvel=qd)
    return a


def _substep_paths(ora, a, seed):
    """Per sub-step and workgroup, from a twin oracle stepped with frame_skip = 1 (the joint controller writes the same ctrl in every
    env-step): does some lane hold an arm row (the main wave solves), a gear row (the columns are read)?"""
    twin = rp.oracle(N, 1, seed)
    twin.set_state(**ora.get_state())
    arm, gear = np.zeros((20, 3), bool), np.zeros((20, 3), bool)
    for k in range(20):
        out, row, fing = rp.limit_rows_of(twin.get_state()["qpos"])
        assert not fing.any()                                                       # no finger row: the arm rows alone switch the path
        arm[k], gear[k] = rp.per_group(out, N), rp.per_group(row, N)
        twin.step(a)
    return arm, gear


def measure_env_step(cross):
    """Worst errors of one env-step over the 165 lanes: dict(obs, q, v, w)."""
    seed = 51
    envs, ora, rng = rp.running_pair("joint", 20, seed)
    a = _mixed_gear_state(ora, rng, cross)
    arm, gear = _substep_paths(ora, a, seed)
    print(f"\nsub-steps with an arm row, per workgroup: {rp.show(arm)}\nsub-steps with a gear row, per workgroup: {rp.show(gear)}")
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
    envs, ora, rng = rp.running_pair("joint", 20, 53, max_episode_steps=50)
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


def test_env_step_with_mixed_gear_rows(torch_cuda):
    w, b = measure_env_step(False), BOUNDS["mixed"]
    assert rp.within(w, b), (w, b)


def test_env_step_leaves_the_remote_path_and_returns(torch_cuda):
    w, b = measure_env_step(True), BOUNDS["cross"]
    assert rp.within(w, b), (w, b)


def test_auto_reset_in_the_middle_of_three_env_steps(torch_cuda):
    w, b = measure_auto_reset(), BOUNDS["reset"]
    assert rp.within(w, b), (w, b)
