"""GPU parity of the one-wave Reach kernels (step_reach_kernel<CTRL, false>, split policy NoSplit) against the CPU oracle, per sub-step.

launch_step picks them for every grid of more than one workgroup per CU -- on an MI355X every Reach engine above 16 384 environments -- and
robot_substep has arms of its own for them: the wave runs the composite pass itself, assembles H_eq after the bias, keeps the warm start and
the first active set in registers, takes the Euler step through euler_accel, and meets no hand-over barrier.  Every other per-sub-step test
runs at most 512 environments, hence the three-wave kernels.  Here MCG_NO_SPLIT=1 is in the environment when the engine is made (mcg_create
reads it), and each case then runs a measurement of tests/reach_measures.py that a three-wave file runs too, unchanged, at that file's
bound: bounds taken from the oracle and from a different kernel than the one under test, so nothing here is fitted to the one-wave kernels.

  * limit rows, one sub-step and one env-step: limit_run on test_gpu_reach_limit_rows.py's kinds and on the families of limit_row_states.py;
  * fast, wide states and mixed gear rows at +-10 rad/s: measure_fast_wide (test_gpu_reach_four_waves.py), measure_mixed
    (test_gpu_reach_remote_solve.py);
  * direct solve -> general iteration -> direct solve inside one env-step, the warm start carried in registers: measure_switch;
  * bad lanes (qvel = 1e12 / 9e9: values the kernels are written to handle): check_bad_lanes, test_bad_lane_in_a_remote_substep's body;
  * teacher-forced rollouts of 64 environments: joint, IK (control_steps 1 and 5, ctrl[:6] included), mocap, at the bounds of
    test_every_substep_of_a_100_step_rollout, test_ik_solves_teacher_forced and test_mocap_substeps_from_identical_state;
  * the natural route: an engine of one workgroup more than the CUs (plus a ragged one) without the variable, against an engine of 192 with
    it, bit for bit -- the switch selects the kernel large grids run -- and its ragged last workgroup against a 37-environment oracle.
"""
import numpy as np
import pytest

from tests import limit_row_states as ls
from tests.common import make_oracle, make_pair, step_errors, sync_oracle_to, torch_cuda  # noqa: F401
from tests.reach_measures import (FAST_WIDE_BOUNDS, MIXED_BOUNDS, SUBSTEP_BOUNDS, assert_substep, check_bad_lanes, limit_run, measure_fast_wide,
                                  measure_mixed, measure_switch)
from tests.reach_parity import within

pytestmark = pytest.mark.gpu

STATE_KEYS = ("qpos", "qvel", "ctrl", "warm", "qpos_lag", "goal", "elapsed", "episode")


@pytest.fixture
def one_wave(torch_cuda, monkeypatch):
    """Every engine made while this holds runs the one-wave Reach kernels."""
    monkeypatch.setenv("MCG_NO_SPLIT", "1")
    return torch_cuda


# ------------------------------------------------------------------------------------------------------------------------- limit rows
@pytest.mark.parametrize("controller", ls.CONTROLLERS)
@pytest.mark.parametrize("kind", ["gear_pair", "gear6", "with_arm", "none", "fingers", "many"])
def test_one_wave_substep_on_limit_states(one_wave, kind, controller):
    assert_substep(limit_run(controller, kind, 1, twin=True), controller)


@pytest.mark.parametrize("kind", ["gear_pair", "with_arm", "many"])
def test_one_wave_joint_env_step_on_limit_states(one_wave, kind):
    assert limit_run("joint", kind, 20)["obs"] < 1e-8                              # smoke()'s 20-sub-step bound


# ----------------------------------------------------------------------------------------------------------------- fast, wide states
@pytest.mark.parametrize("all_dofs", [False, True], ids=["arm", "all"])
@pytest.mark.parametrize("controller", ls.CONTROLLERS)
def test_one_wave_substep_on_fast_wide_states(one_wave, controller, all_dofs):
    w, b = measure_fast_wide(controller, all_dofs), FAST_WIDE_BOUNDS[controller, all_dofs]
    assert within(w, b), (w, b)


def test_one_wave_substep_with_mixed_gear_rows(one_wave):
    w, b = measure_mixed("joint"), MIXED_BOUNDS["joint"]
    assert within(w, b), (w, b)


@pytest.mark.parametrize("rows", ["direct", "general"])
def test_one_wave_env_step_switches_solves_and_back(one_wave, rows):
    worst, flags_equal = measure_switch(rows)
    assert flags_equal
    assert worst < 1e-8                                                           # smoke()'s 20-sub-step bound


def test_one_wave_bad_lanes(one_wave):
    check_bad_lanes()                                                             # test_bad_lane_in_a_remote_substep's states and assertions


# ------------------------------------------------------------------------------------------------------------ teacher-forced rollouts
def _teacher_forced(n, steps, actions, **kw):
    """`steps` engine steps of `n` environments, the state re-synchronised to the oracle's before each, the action redrawn every 20:
    worst errors of observation, qpos, qvel, warm start and ctrl[:6] after each."""
    seed = kw["seed"]
    envs, ora = make_pair(n, reward_type="dense", max_episode_steps=10 ** 9, frame_skip=1, **kw)
    envs.reset(seed=seed); ora.reset(seed=seed)
    worst = dict(obs=0.0, qpos=0.0, qvel=0.0, warm=0.0, ctrl=0.0)
    for t in range(steps):
        if t % 20 == 0: a = actions(envs.action_dim)
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        st, so = envs.get_state(), ora.get_state()
        worst["obs"] = max(worst["obs"], float(e.max()))
        for k in ("qpos", "qvel", "warm"): worst[k] = max(worst[k], float(np.abs(st[k].cpu().numpy().T - so[k]).max()))
        if so["ctrl"].shape[1] == 7: worst["ctrl"] = max(worst["ctrl"], float(np.abs(st["ctrl"].cpu().numpy().T[:, :6] - so["ctrl"][:, :6]).max()))
    envs.close()
    return worst


def test_one_wave_joint_rollout_teacher_forced(one_wave):
    rng = np.random.default_rng(2)
    w = _teacher_forced(64, 100, lambda dim: rng.uniform(-1, 1, (64, dim)).astype(np.float32), controller_type="joint", seed=11)
    print(f"\none wave, joint: 100 sub-steps x 64 envs from identical state: {w}")
    assert w["obs"] < 1e-13 and w["qpos"] < 1e-12 and w["qvel"] < 3e-10 and w["warm"] < 4e-8      # test_every_substep_of_a_100_step_rollout's


@pytest.mark.parametrize("control_steps", [1, 5])
def test_one_wave_ik_solves_teacher_forced(one_wave, control_steps):
    for fetch in (False, True):
        rng = np.random.default_rng(8)
        w = _teacher_forced(64, 100, lambda dim: rng.uniform(-1, 1, (64, dim)).astype(np.float32), controller_type="IK", fetch_env=fetch,
                            control_steps=control_steps, seed=13)
        print(f"\none wave, IK{' fetch' if fetch else ''}, control_steps={control_steps}: 100 steps x 64 envs from identical state: {w}")
        assert w["ctrl"] < 1e-11                                                  # test_ik_solves_teacher_forced's bounds
        assert w["obs"] < 1e-9 and w["qpos"] < 1e-9 and w["qvel"] < 1e-7


def test_one_wave_mocap_substeps_from_identical_state(one_wave):
    from tests.test_gpu_mocap import _actions
    rng = np.random.default_rng(7)
    w = _teacher_forced(64, 600, lambda dim: _actions(rng, 64, dim), controller_type="mocap", seed=3)
    print(f"\none wave, mocap: 600 sub-steps x 64 envs from identical state: {w}")
    assert w["obs"] < 3e-13 and w["qpos"] < 1e-10 and w["qvel"] < 4e-8          # test_mocap_substeps_from_identical_state's


# ------------------------------------------------------------------------------------------------------------------ the natural route
def test_large_grid_runs_the_kernel_the_switch_selects(torch_cuda, monkeypatch):
    """An engine of num_cu + 1 full workgroups and a ragged one of 37 lanes takes the one-wave kernels by itself.  Its first 192 lanes hold
    the `many` family (tiled), as an engine of 192 made with MCG_NO_SPLIT=1 does: the same kernel on the same wave composition, so one
    sub-step must agree bit for bit.  Its last 37 lanes -- the ragged workgroup -- hold the first 37 states of `fingers` and are compared
    with an oracle of 37 environments at the sub-step bounds; the oracle never sees the large engine."""
    torch = torch_cuda
    from mycobotgym_amd import MyCobotVecEnv
    num_cu = torch.cuda.get_device_properties(0).multi_processor_count
    n_big, n_small, n_tail = 64 * (num_cu + 1) + 37, 192, 37
    kw = ls.engine_kw("joint")
    monkeypatch.setenv("MCG_NO_SPLIT", "1")
    small = MyCobotVecEnv(n_small, has_object=False, env_id_offset=0, **kw)
    monkeypatch.delenv("MCG_NO_SPLIT")
    big = MyCobotVecEnv(n_big, has_object=False, env_id_offset=0, **kw)
    small.reset(seed=ls.SEED); big.reset(seed=ls.SEED)
    many, fingers = ls.family_state("joint", "many"), ls.family_state("joint", "fingers")
    idx = np.arange(n_small) % ls.N
    head = {k: many["state"][k][idx] for k in STATE_KEYS}
    tail = {k: fingers["state"][k][:n_tail].copy() for k in STATE_KEYS}
    col = lambda v: torch.as_tensor(np.ascontiguousarray(v.T))                    # the engine's layout: [dim, N]
    small.set_state(**{k: col(v) for k, v in head.items()})
    sb = {k: v.clone() for k, v in big.get_state().items() if k in STATE_KEYS}
    for k in STATE_KEYS:
        sb[k][..., :n_small] = col(head[k]).to(sb[k]); sb[k][..., n_big - n_tail:] = col(tail[k]).to(sb[k])
    big.set_state(**sb)
    a_big = np.random.default_rng(9).uniform(-1, 1, (n_big, 7)).astype(np.float32)
    a_big[:n_small] = many["action"][idx]; a_big[n_big - n_tail:] = fingers["action"][:n_tail]
    big.counters(clear=True)
    ob, *_ = big.step(torch.as_tensor(a_big))
    os_, *_ = small.step(torch.as_tensor(a_big[:n_small].copy()))
    gb, gs = big.get_state(), small.get_state()
    assert torch.isfinite(ob["observation"]).all() and big.counters()["bad_state_resets"] == 0
    assert torch.equal(ob["observation"][:n_small], os_["observation"])
    for k in ("qpos", "qvel", "warm"):
        assert torch.equal(gb[k][:, :n_small], gs[k]), k
    # the ragged workgroup against the oracle, and the oracle's own sensitivity on the same 37 states
    ora, twin = make_oracle(n_tail, **kw), make_oracle(n_tail, **kw)
    ora.reset(seed=ls.SEED); twin.reset(seed=ls.SEED)
    ora.set_state(**{k: v.copy() for k, v in tail.items()})
    o = ora.step(a_big[n_big - n_tail:])
    so = ora.get_state()
    t = ls.twin_state_errors(twin, tail, a_big[n_big - n_tail:], ora, o, np.random.default_rng(7))
    w = dict(obs=float(np.abs(ob["observation"][n_big - n_tail:].cpu().numpy() - o["obs"]).max()))
    for k, name in (("q", "qpos"), ("v", "qvel"), ("w", "warm")):
        w[k] = float(np.abs(gb[name][:, n_big - n_tail:].cpu().numpy().T - so[name]).max())
    print(f"\n{n_big} environments on {num_cu} CUs: first {n_small} lanes bit-identical to the {n_small}-env one-wave engine; ragged workgroup vs "
          "oracle " + " ".join(f"{k} {v:.2e}" for k, v in w.items()) + "; twin " + " ".join(f"{k} {v:.2e}" for k, v in t.items()))
    small.close(); big.close()
    for k, bound in SUBSTEP_BOUNDS["joint"].items():
        assert w[k] <= max(bound, 10.0 * t[k]), (k, w, t)
