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
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N = 165

# (controller, all twelve dofs fast?) -> 100 x the parent build's error, rounded down; the measured figures are in the comments
BOUNDS = {
    ("joint", False): dict(obs=3.3e-14, q=3.3e-13, v=1.6e-10, w=2.4e-11),      # 3.331e-16  3.377e-15  1.688e-12  2.439e-13
    ("joint", True):  dict(obs=3.3e-14, q=6.0e-13, v=3.0e-10, w=6.9e-12),      # 3.331e-16  6.079e-15  3.040e-12  6.983e-14
    ("IK", False):    dict(obs=3.3e-14, q=3.1e-13, v=1.5e-10, w=2.2e-11),      # 3.331e-16  3.161e-15  1.581e-12  2.296e-13
    ("IK", True):     dict(obs=3.3e-14, q=5.3e-13, v=2.6e-10, w=6.1e-12),      # 3.331e-16  5.321e-15  2.661e-12  6.124e-14
    ("mocap", False): dict(obs=2.2e-13, q=6.7e-12, v=3.3e-09, w=7.3e-12),      # 2.221e-15  6.701e-14  3.350e-11  7.324e-14
    ("mocap", True):  dict(obs=3.1e-13, q=6.5e-12, v=3.2e-09, w=4.8e-12),      # 3.119e-15  6.573e-14  3.286e-11  4.894e-14
}


@pytest.fixture(scope="module")
def torch_cuda(built):
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def _fast_wide_state(ora, rng, jnt_range, all_dofs):
    """The oracle's state after a reset and two random steps, arm angles spread over their ranges, velocities up to 10 rad/s."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    lo, hi = jnt_range[:6, 0], jnt_range[:6, 1]
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q[:, :6] = c + 0.98 * h * rng.uniform(-1.0, 1.0, (q.shape[0], 6))
    nd = 12 if all_dofs else 6
    qd[:, :nd] = rng.uniform(-10.0, 10.0, (q.shape[0], nd))
    ora.set_state(qpos=q, qvel=qd)


def measure(controller, all_dofs):
    """Worst errors of one sub-step over the 165 lanes: dict(obs, q, v, w); w is relative to the lane's largest |qacc|."""
    from tests.common import load_json, make_pair, step_errors, sync_oracle_to, table_name
    kw = dict(controller_type=controller, reward_type="dense", seed=33, max_episode_steps=10 ** 9, frame_skip=1)
    if controller == "IK": kw["control_steps"] = 1
    jnt_range = np.array(load_json(table_name(False, "legacy", controller == "mocap"))["jnt_range"], dtype=np.float64)
    envs, ora = make_pair(N, **kw)
    envs.reset(seed=33); ora.reset(seed=33)
    rng = np.random.default_rng(17 + int(all_dofs))
    for t in range(2):                                     # two ordinary steps: warm start, lagged q and ctrl are those of a running episode
        a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
        sync_oracle_to(envs, ora)
        step_errors(envs, ora, a)
    _fast_wide_state(ora, rng, jnt_range, all_dofs)
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    assert flags_equal
    st, so = envs.get_state(), ora.get_state()
    gq, gv, gw = (st[k].cpu().numpy().T for k in ("qpos", "qvel", "warm"))
    for name, arr in (("engine", (gq, gv, gw)), ("oracle", (so["qpos"], so["qvel"], so["warm"]))):
        assert all(np.isfinite(x).all() for x in arr), name
        # mj_resetData leaves qpos0 (zeros in joint coordinates) and zero velocity / warm start behind
        reset = (arr[1] == 0).all(axis=1) & (arr[2] == 0).all(axis=1)
        assert not reset.any(), (name, "lanes reset", np.nonzero(reset)[0])
    assert envs.counters()["bad_state_resets"] == 0
    qacc = np.abs(so["warm"]).max(axis=1)
    w = dict(obs=float(e.max()), q=float(np.abs(gq - so["qpos"]).max()), v=float(np.abs(gv - so["qvel"]).max()),
             w=float((np.abs(gw - so["warm"]).max(axis=1) / qacc).max()))
    envs.close()
    print(f"\n{controller} {'all twelve' if all_dofs else 'arm'} dofs fast: " + " ".join(f"{k} {v:.3e}" for k, v in w.items())
          + f"   max|qacc| {qacc.max():.3e} max|qvel| {np.abs(so['qvel']).max():.3e}")
    return w


@pytest.mark.parametrize("all_dofs", [False, True], ids=["arm", "all"])
@pytest.mark.parametrize("controller", ["joint", "IK", "mocap"])
def test_substep_on_fast_wide_states(torch_cuda, controller, all_dofs):
    w = measure(controller, all_dofs)
    b = BOUNDS[controller, all_dofs]
    assert w["obs"] <= b["obs"] and w["q"] <= b["q"] and w["v"] <= b["v"] and w["w"] <= b["w"], (w, b)
