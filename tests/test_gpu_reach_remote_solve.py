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
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 165
ARM_HI = 2.96706                                     # jnt_range[0][1] of the mycobot280 tables; the gear joints' range is [0, 0.7]
GROUPS = [slice(0, 64), slice(64, 128), slice(128, N)]

# Test 2, 100 x the error of the build this change started from (the main wave solves, barrier S2b), measured on an MI355X on these very
# states; the measured figures are in the comments.  qpos / qvel / observation absolute, the warm start (= qacc) relative to the lane's
# largest |qacc|, as in test_gpu_reach_four_waves.py.
MIXED_BOUNDS = {
    "joint": dict(obs=9.5e-14, q=3.6e-12, v=1.8e-09, w=8.6e-12),      # 9.518e-16  3.673e-14  1.837e-11  8.614e-14
}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _pair(controller, frame_skip, seed):
    """Engine and oracle after a reset and one ordinary step: warm start, lagged q and ctrl are those of a running episode."""
    from tests.common import make_pair, step_errors, sync_oracle_to
    kw = dict(controller_type=controller, reward_type="dense", seed=seed, max_episode_steps=10 ** 9, frame_skip=frame_skip)
    if controller == "IK" and frame_skip == 1: kw["control_steps"] = 1
    envs, ora = make_pair(N, **kw)
    envs.reset(seed=seed); ora.reset(seed=seed)
    rng = np.random.default_rng(seed)
    sync_oracle_to(envs, ora)
    _, flags_equal, _ = step_errors(envs, ora, rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32))
    assert flags_equal
    return envs, ora, rng


def _state_errors(envs, ora, relative_warm=False):
    st, so = envs.get_state(), ora.get_state()
    gq, gv, gw = (st[k].cpu().numpy().T for k in ("qpos", "qvel", "warm"))
    assert all(np.isfinite(x).all() for x in (gq, gv, gw, so["qpos"], so["qvel"], so["warm"]))
    w = np.abs(gw - so["warm"]).max(axis=1)
    if relative_warm: w = w / np.abs(so["warm"]).max(axis=1)
    return np.abs(gq - so["qpos"]).max(axis=1), np.abs(gv - so["qvel"]).max(axis=1), w, (gq, gv, gw)


# ------------------------------------------------------------------------------- 1. remote -> main-wave solve -> remote in one env-step
def measure_switch(rows):
    """One env-step from the states of test_env_step_switches_paths_and_back (built here, their path through the twenty sub-steps checked on
    a second oracle): -> (worst observation error over the 165 lanes, flags_equal).  tests/test_gpu_reach_one_wave.py runs it too."""
    from tests.common import make_oracle, step_errors, sync_oracle_to
    envs, ora, rng = _pair("joint", 20, 41)
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(N)
    cross = (i % 64 == 5) | (i % 64 == 30)
    q[:, 6] = -rng.uniform(3e-3, 5e-3, N); q[:, 8] = -rng.uniform(3e-3, 5e-3, N)
    q[i % 3 == 1, 8] = rng.uniform(0.05, 0.3, int((i % 3 == 1).sum()))             # a third of the lanes: row 6 only
    if rows == "direct":
        q[cross, 6] = rng.uniform(0.05, 0.3, int(cross.sum())); q[cross, 8] = rng.uniform(0.05, 0.3, int(cross.sum()))
    else:
        q[cross, 6] = -4e-3; q[cross, 8] = -4e-3
    q[cross, 0] = ARM_HI - 0.02; qd[cross, 0] = rng.uniform(7.5, 8.5, int(cross.sum()))
    ora.set_state(qpos=q, qvel=qd)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    a[:, 6] = -1.0; a[cross, 0] = 1.0
    # the path of every sub-step, from a twin stepped with frame_skip = 1 (the joint controller writes the same ctrl in every env-step)
    twin = make_oracle(N, controller_type="joint", reward_type="dense", seed=41, max_episode_steps=10 ** 9, frame_skip=1)
    twin.reset(seed=41); twin.set_state(**ora.get_state())
    arm_out, gear_row, most_rows = np.zeros((20, 3), bool), np.zeros((20, 3), bool), 0
    for k in range(20):
        tq = twin.get_state()["qpos"]
        out = np.abs(tq[:, :6]) > ARM_HI
        gear = (tq[:, 6] < 0) | (tq[:, 8] < 0)
        assert not (np.abs(tq[:, [7, 9]]) > 0.872664).any()                         # no finger row: the arm rows alone switch the path
        for g, sl in enumerate(GROUPS):
            arm_out[k, g] = out[sl].any(); gear_row[k, g] = gear[sl].any()
        most_rows = max(most_rows, int((out.sum(axis=1) + (tq[:, 6] < 0) + (tq[:, 8] < 0))[out.any(axis=1)].max(initial=0)))
        twin.step(a)
    print(f"\n{rows}: sub-steps with an arm row, per workgroup: " + " | ".join("".join("X" if x else "." for x in arm_out[:, g]) for g in range(3))
          + f"; most violated rows in a lane with an arm row: {most_rows}")
    assert gear_row.all()
    for g in range(3):
        k_out = np.nonzero(arm_out[:, g])[0]
        assert not arm_out[0, g] and k_out.size and k_out[0] >= 2 and k_out[-1] <= 17, (g, k_out)      # remote, main wave, remote again
    assert most_rows == (3 if rows == "general" else 1)
    sync_oracle_to(envs, ora)
    e, flags_equal, o = step_errors(envs, ora, a)
    eq, ev, ew, _ = _state_errors(envs, ora)
    print(f"{rows}: obs {e.max():.2e} qpos {eq.max():.2e} qvel {ev.max():.2e} warm {ew.max():.2e}")
    envs.close()
    return float(e.max()), flags_equal


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
def measure_mixed(controller):
    """Worst errors of one sub-step over the 165 lanes: dict(obs, q, v, w); w is relative to the lane's largest |qacc|."""
    from tests.common import step_errors, sync_oracle_to
    envs, ora, rng = _pair(controller, 1, 43)
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(N)
    below = -rng.uniform(1e-4, 5e-3, (N, 2)); inside = rng.uniform(0.05, 0.3, (N, 2))
    q[:, 6] = np.where((i % 4 == 0) | (i % 4 == 1), below[:, 0], inside[:, 0])      # both, only 6, only 8, none -- sixteen of each in a wave
    q[:, 8] = np.where((i % 4 == 0) | (i % 4 == 2), below[:, 1], inside[:, 1])
    qd[:, :12] = rng.uniform(-10.0, 10.0, (N, 12))
    ora.set_state(qpos=q, qvel=qd)
    tq = ora.get_state()["qpos"]
    assert not (np.abs(tq[:, :6]) > ARM_HI).any() and not (np.abs(tq[:, [7, 9]]) > 0.872664).any()      # gear rows only: a remote sub-step
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    assert flags_equal
    eq, ev, ew, _ = _state_errors(envs, ora, relative_warm=True)
    assert envs.counters()["bad_state_resets"] == 0
    qacc = np.abs(ora.get_state()["warm"]).max()
    envs.close()
    w = dict(obs=float(e.max()), q=float(eq.max()), v=float(ev.max()), w=float(ew.max()))
    print(f"\n{controller} mixed gear rows, all twelve dofs fast: " + " ".join(f"{k} {v:.3e}" for k, v in w.items()) + f"   max|qacc| {qacc:.3e}")
    return w


@pytest.mark.parametrize("controller", sorted(MIXED_BOUNDS))
def test_substep_with_mixed_gear_rows(torch_cuda, controller):
    w = measure_mixed(controller)
    b = MIXED_BOUNDS[controller]
    assert w["obs"] <= b["obs"] and w["q"] <= b["q"] and w["v"] <= b["v"] and w["w"] <= b["w"], (w, b)


# -------------------------------------------------------------------------------------------------- 3. a bad lane in a remote sub-step
def test_bad_lane_in_a_remote_substep(torch_cuda):
    """Lane 9 of every workgroup arrives with qvel = 1e12 on all twelve dofs: mj_checkVel resets it when the step starts, and the
    sub-step runs from qpos0 -- to the sub-step bounds against the oracle, like every ordinary lane.  Lane 50 (20 in the ragged
    workgroup) arrives with 9e9 rad/s on arm joint 1, which passes that check: the bias forces, the right-hand side and the solve of
    that lane overflow inside the RNE wave's remote solve, the main wave's checks on the new state catch it, and the lane leaves the
    sub-step as mj_resetData leaves it (the oracle then integrates one sub-step from there, the engine does with the next: the lag
    test_gpu_api_round2.py describes, so this lane is compared with the reset state, not with the oracle).  The sub-step is remote:
    gear rows in the other lanes, no other row."""
    from tests.common import step_errors, sync_oracle_to
    envs, ora, rng = _pair("joint", 1, 47)
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(N)
    at_load = np.nonzero(i % 64 == 9)[0]
    in_step = np.array([50, 114, 148])
    q[:, 6] = np.where(i % 2 == 0, -rng.uniform(1e-4, 5e-3, N), rng.uniform(0.05, 0.3, N))
    q[:, 8] = np.where(i % 3 == 0, -rng.uniform(1e-4, 5e-3, N), rng.uniform(0.05, 0.3, N))
    qd[at_load, :12] = 1e12
    qd[in_step, 1] = 9e9
    ora.set_state(qpos=q, qvel=qd)
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    eq, ev, ew, (gq, gv, gw) = _state_errors(envs, ora)
    c = envs.counters()
    envs.close()
    keep = np.ones(N, bool); keep[in_step] = False
    print(f"\nbad lanes: reset at load {at_load}, in the sub-step {in_step}; counters {c}; the other lanes and the lanes reset at load: "
          f"obs {e[keep].max():.2e} qpos {eq[keep].max():.2e} qvel {ev[keep].max():.2e} warm {ew[keep].max():.2e}; "
          f"lanes reset in the sub-step: |qpos| {np.abs(gq[in_step]).max():.1e} |qvel| {np.abs(gv[in_step]).max():.1e} |warm| {np.abs(gw[in_step]).max():.1e}")
    assert flags_equal
    assert all(int(ora.data(int(k)).get("warning_badstate", (1,), np.int32)[0]) >= 1 for k in at_load)
    assert c["bad_state_resets"] == at_load.size + in_step.size
    # test_gpu_parity's sub-step bounds, the lanes reset at load included
    assert e[keep].max() < 1e-13 and eq[keep].max() < 1e-12 and ev[keep].max() < 3e-10 and ew[keep].max() < 4e-8
    assert (gq[in_step] == 0).all() and (gv[in_step] == 0).all() and (gw[in_step] == 0).all()      # mj_resetData: qpos0, no velocity, no warm start
