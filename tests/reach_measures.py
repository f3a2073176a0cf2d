"""Measurements of the Reach parity tests that more than one file runs, with the bounds that travel with them.  Not collected.

Each section names the file that describes its states and the files that run it; tests/test_gpu_reach_one_wave.py runs most of them once
more on the one-wave kernels.  Built on tests/reach_parity.py (layout, recording, engine side, running pair) and tests/limit_row_states.py.
"""
from __future__ import annotations

import functools

import numpy as np

from tests import limit_row_states as ls
from tests import reach_parity as rp
from tests.common import make_oracle, step_errors, sync_oracle_to
from tests.reach_parity import ARM_HI, FINGER_HI, GEAR_HI, GEAR_LO, N, SEED, SUBSTEPS


# ------------------------------------------------- the window states: tests/test_gpu_reach_side_wave_slots.py, ..._factor_order.py
SLOT_CASES = ("none", "row6", "row8", "both_lower", "both_upper", "arm", "switch", "reset", "mixed")
SLOT_RUNS = [(c, N) for c in SLOT_CASES if c != "mixed"] + [("mixed", 65)]


@functools.lru_cache(maxsize=None)
def slot_oracle_run(case, n):
    """The case (tests/test_gpu_reach_side_wave_slots.py's docstring) on the CPU oracle alone: dict(action; pre / post / out = state
    before / after and outputs of each of the twenty single sub-steps; arm / gear [20, groups] = some lane of the workgroup holds an arm
    row / a gear row when the sub-step starts; env_pre = the state the env-steps start from; env_post / env_out = state and outputs after
    each whole env-step)."""
    rng = np.random.default_rng([SEED, 11, SLOT_CASES.index(case), n])
    ora = rp.oracle(n, 1, SEED, rp.episode_limit(case), running=rng)
    a = rp.put_gear_case("mixed" if case == "arm" else case, ora, rng, n)
    if case == "arm":
        s = ora.get_state()
        q, qd = s["qpos"].copy(), s["qvel"].copy()
        x = (np.arange(n) % 64 == 5) | (np.arange(n) % 64 == 30)
        q[x, 0] = ARM_HI + 0.03; qd[x, 0] = 0.0; a[x, 0] = 1.0
        ora.set_state(qpos=q, qvel=qd)
    groups = len(rp.groups(n))
    r = dict(action=a, arm=np.zeros((SUBSTEPS, groups), bool), gear=np.zeros((SUBSTEPS, groups), bool))
    start = ora.get_state()

    def rows(k, pre, o):
        arm, gear, fing = rp.limit_rows_of(pre["qpos"])
        assert not fing.any()                                              # no finger row: the arm rows alone switch the path
        r["arm"][k], r["gear"][k] = rp.per_group(arm, n), rp.per_group(gear, n)

    r.update(rp.record_substeps(ora, a, each=rows))
    # whole env-steps from the same state (reset: the first one ends the episode of a fifth of the lanes)
    if case == "reset":
        el = start["elapsed"].copy(); el[np.arange(n) % 5 == 2] = 49
        start = dict(start, elapsed=el)
    r.update(rp.replay_env_steps(rp.oracle(n, 20, SEED, rp.episode_limit(case)), start, a, steps=2 if case == "reset" else 1))
    return rp.freeze(r)


def slot_check_paths(case, n, r):
    """The sub-steps take the paths the case is about."""
    print(f"\n{case} ({n}): sub-steps with an arm row, per workgroup: {rp.show(r['arm'])}\n{case} ({n}): sub-steps with a gear row, per workgroup: {rp.show(r['gear'])}")
    q = np.stack([s["qpos"] for s in r["pre"]])
    row = (q[:, :, [6, 8]] < GEAR_LO) | (q[:, :, [6, 8]] > GEAR_HI)                   # [20, n, 2]
    if case not in ("arm", "switch"): assert not r["arm"].any()                       # twenty remote sub-steps in every workgroup
    if case == "none": assert not r["gear"].any()
    if case in ("row6", "row8"):
        j = 0 if case == "row6" else 1
        assert row[0, :, j].all() and not row[0, :, 1 - j].any()
    if case in ("both_lower", "both_upper"):
        assert row[0].all() and ((q[0, :, [6, 8]] > GEAR_HI).all() if case == "both_upper" else (q[0, :, [6, 8]] < GEAR_LO).all())
    if case == "arm":
        assert r["arm"][:2].all() and r["gear"][:2].all()                             # the main wave solves, with gear rows beside the arm row
    if case == "switch":
        for g in range(r["arm"].shape[1]):
            k_out = np.nonzero(r["arm"][:, g])[0]
            assert not r["arm"][0, g] and k_out.size and k_out[0] >= 2 and k_out[-1] <= 17, (g, k_out)      # remote, main wave, remote again
    trunc = np.stack([o["truncated"].astype(bool) for o in r["out"]])
    if case == "reset":
        late = np.arange(n) % 5 == 2
        assert np.array_equal(trunc[9], late) and not trunc[:9].any() and not trunc[10:].any()      # the reset lands in the tenth sub-step
        assert np.array_equal(r["env_out"][0]["truncated"].astype(bool), late) and not r["env_out"][1]["truncated"].any()
    else:
        assert not trunc.any() and not r["env_out"][0]["truncated"].any()


def slot_engine(case, n, frame_skip):
    return rp.engine(n, frame_skip, SEED, rp.episode_limit(case))


def measure_slot_substeps(case, n):
    """Worst errors over the twenty single sub-steps and the n lanes."""
    r = slot_oracle_run(case, n)
    slot_check_paths(case, n, r)
    return rp.measure_substeps(r, functools.partial(slot_engine, case, n), f"{case} ({n}) sub-steps")


def measure_slot_env_steps(case, n):
    """Worst errors after each whole env-step (the engine runs on from its own state) over the n lanes."""
    return rp.measure_env_steps(slot_oracle_run(case, n), functools.partial(slot_engine, case, n), f"{case} ({n}) env-steps")


# ------------------------------------- limit rows: tests/test_gpu_reach_limit_rows.py, ..._limit_families.py, tests/limit_row_states.py
# obs, qpos, qvel, warm start: the joint controller's from test_gpu_parity, IK's and mocap's from test_gpu_mocap (which has none for warm)
SUBSTEP_BOUNDS = {"joint": dict(obs=1e-13, q=1e-12, v=3e-10, w=4e-8), "IK": dict(obs=3e-13, q=1e-10, v=4e-8), "mocap": dict(obs=3e-13, q=1e-10, v=4e-8)}


def limit_state(ora, kind, rng, controller="joint"):
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


def limit_run(controller, kind, frame_skip, twin=False):
    """Worst errors against the oracle over the step from the `kind` state and the one after it: dict(obs, q, v, w).  `twin`: also the
    oracle's own sensitivity on the same states and actions (a second oracle started +-1e-14 away on qpos), under the keys twin_obs, twin_q,
    twin_v, twin_w; and the engine's bad-state counter over the two steps under `bad_state_resets`."""
    rng = np.random.default_rng(5)
    envs, ora, _ = rp.running_pair(controller, frame_skip, ls.SEED, rng=rng)
    worst = dict(obs=0.0, q=0.0, v=0.0, w=0.0)
    if twin:
        two = make_oracle(N, **ls.engine_kw(controller, frame_skip)); two.reset(seed=ls.SEED)
        prng = np.random.default_rng(7)
        worst.update(twin_obs=0.0, twin_q=0.0, twin_v=0.0, twin_w=0.0)
    for t in (1, 2):
        a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
        if t == 1:
            n6, n8 = limit_state(ora, kind, rng, controller)
            if kind == "none": assert n6 == 0 and n8 == 0
            elif kind not in ls.FAMILIES: assert n6 > 0 and (kind == "gear6" or n8 > 0)
            if twin: envs.counters(clear=True)
        sync_oracle_to(envs, ora)
        before = ora.get_state() if twin else None
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        if twin:
            for k, v in ls.twin_state_errors(two, before, a, ora, o, prng).items(): worst["twin_" + k] = max(worst["twin_" + k], v)
        eq, ev, ew, _ = rp.state_errors(envs, ora)
        worst.update(obs=max(worst["obs"], float(e.max())), q=max(worst["q"], float(eq.max())), v=max(worst["v"], float(ev.max())),
                     w=max(worst["w"], float(ew.max())))
    if twin: worst["bad_state_resets"] = envs.counters()["bad_state_resets"]
    envs.close()
    print(f"\n{controller} {kind} frame_skip={frame_skip}: " + " ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def assert_substep(w, controller):
    """limit_run(..., twin=True)'s figures against the sub-step bounds, each widened to 10 x the twin's figure where that is larger."""
    for k, bound in SUBSTEP_BOUNDS[controller].items():
        limit = max(bound, 10.0 * w["twin_" + k])
        assert w[k] <= limit, (controller, k, w[k], limit, w)
    assert w["bad_state_resets"] == 0


# ------------------------------------------------------------------------------ fast, wide states: tests/test_gpu_reach_four_waves.py
# (controller, all twelve dofs fast?) -> 100 x the parent build's error, rounded down; the measured figures are in the comments
FAST_WIDE_BOUNDS = {
    ("joint", False): dict(obs=3.3e-14, q=3.3e-13, v=1.6e-10, w=2.4e-11),      # 3.331e-16  3.377e-15  1.688e-12  2.439e-13
    ("joint", True):  dict(obs=3.3e-14, q=6.0e-13, v=3.0e-10, w=6.9e-12),      # 3.331e-16  6.079e-15  3.040e-12  6.983e-14
    ("IK", False):    dict(obs=3.3e-14, q=3.1e-13, v=1.5e-10, w=2.2e-11),      # 3.331e-16  3.161e-15  1.581e-12  2.296e-13
    ("IK", True):     dict(obs=3.3e-14, q=5.3e-13, v=2.6e-10, w=6.1e-12),      # 3.331e-16  5.321e-15  2.661e-12  6.124e-14
    ("mocap", False): dict(obs=2.2e-13, q=6.7e-12, v=3.3e-09, w=7.3e-12),      # 2.221e-15  6.701e-14  3.350e-11  7.324e-14
    ("mocap", True):  dict(obs=3.1e-13, q=6.5e-12, v=3.2e-09, w=4.8e-12),      # 3.119e-15  6.573e-14  3.286e-11  4.894e-14
}


def fast_wide_state(ora, rng, jnt_range, all_dofs):
    """The oracle's state after a reset and two random steps, arm angles spread over their ranges, velocities up to 10 rad/s."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    lo, hi = jnt_range[:6, 0], jnt_range[:6, 1]
    c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
    q[:, :6] = c + 0.98 * h * rng.uniform(-1.0, 1.0, (q.shape[0], 6))
    nd = 12 if all_dofs else 6
    qd[:, :nd] = rng.uniform(-10.0, 10.0, (q.shape[0], nd))
    ora.set_state(qpos=q, qvel=qd)


def measure_fast_wide(controller, all_dofs):
    """Worst errors of one sub-step over the 165 lanes: dict(obs, q, v, w); w is relative to the lane's largest |qacc|."""
    rng = np.random.default_rng(17 + int(all_dofs))
    envs, ora, _ = rp.running_pair(controller, 1, 33, rng=rng, steps=2)
    fast_wide_state(ora, rng, ls.jnt_range(controller), all_dofs)
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    assert flags_equal
    eq, ev, ew, got = rp.state_errors(envs, ora, relative_warm=True)                 # (all finite, on either side)
    so = ora.get_state()
    for name, arr in (("engine", got), ("oracle", (so["qpos"], so["qvel"], so["warm"]))):
        # mj_resetData leaves qpos0 (zeros in joint coordinates) and zero velocity / warm start behind
        reset = (arr[1] == 0).all(axis=1) & (arr[2] == 0).all(axis=1)
        assert not reset.any(), (name, "lanes reset", np.nonzero(reset)[0])
    assert envs.counters()["bad_state_resets"] == 0
    envs.close()
    w = dict(obs=float(e.max()), q=float(eq.max()), v=float(ev.max()), w=float(ew.max()))
    print(f"\n{controller} {'all twelve' if all_dofs else 'arm'} dofs fast: " + " ".join(f"{k} {v:.3e}" for k, v in w.items())
          + f"   max|qacc| {np.abs(so['warm']).max():.3e} max|qvel| {np.abs(so['qvel']).max():.3e}")
    return w


# ------------------------------------------------------------- the remote solve's meeting points: tests/test_gpu_reach_remote_solve.py
# 100 x the error of the build that file's change started from (the main wave solves, barrier S2b), measured on an MI355X on these very
# states; the measured figures are in the comments.  qpos / qvel / observation absolute, the warm start (= qacc) relative to the lane's
# largest |qacc|, as in FAST_WIDE_BOUNDS.
MIXED_BOUNDS = {
    "joint": dict(obs=9.5e-14, q=3.6e-12, v=1.8e-09, w=8.6e-12),      # 9.518e-16  3.673e-14  1.837e-11  8.614e-14
}


def measure_switch(rows):
    """One env-step from the states of test_env_step_switches_paths_and_back (built here, their path through the twenty sub-steps checked on
    a second oracle): -> (worst observation error over the 165 lanes, flags_equal)."""
    envs, ora, rng = rp.running_pair("joint", 20, 41)
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
    twin = rp.oracle(N, 1, 41)
    twin.set_state(**ora.get_state())
    groups = rp.groups(N)
    arm_out, gear_row, most_rows = np.zeros((20, len(groups)), bool), np.zeros((20, len(groups)), bool), 0
    for k in range(20):
        tq = twin.get_state()["qpos"]
        out = np.abs(tq[:, :6]) > ARM_HI
        gear = (tq[:, 6] < 0) | (tq[:, 8] < 0)
        assert not (np.abs(tq[:, [7, 9]]) > FINGER_HI).any()                        # no finger row: the arm rows alone switch the path
        for g, sl in enumerate(groups):
            arm_out[k, g] = out[sl].any(); gear_row[k, g] = gear[sl].any()
        most_rows = max(most_rows, int((out.sum(axis=1) + (tq[:, 6] < 0) + (tq[:, 8] < 0))[out.any(axis=1)].max(initial=0)))
        twin.step(a)
    print(f"\n{rows}: sub-steps with an arm row, per workgroup: {rp.show(arm_out)}; most violated rows in a lane with an arm row: {most_rows}")
    assert gear_row.all()
    for g in range(len(groups)):
        k_out = np.nonzero(arm_out[:, g])[0]
        assert not arm_out[0, g] and k_out.size and k_out[0] >= 2 and k_out[-1] <= 17, (g, k_out)      # remote, main wave, remote again
    assert most_rows == (3 if rows == "general" else 1)
    sync_oracle_to(envs, ora)
    e, flags_equal, o = step_errors(envs, ora, a)
    eq, ev, ew, _ = rp.state_errors(envs, ora)
    print(f"{rows}: obs {e.max():.2e} qpos {eq.max():.2e} qvel {ev.max():.2e} warm {ew.max():.2e}")
    envs.close()
    return float(e.max()), flags_equal


def measure_mixed(controller):
    """Worst errors of one sub-step over the 165 lanes: dict(obs, q, v, w); w is relative to the lane's largest |qacc|."""
    envs, ora, rng = rp.running_pair(controller, 1, 43)
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(N)
    below = -rng.uniform(1e-4, 5e-3, (N, 2)); inside = rng.uniform(0.05, 0.3, (N, 2))
    q[:, 6] = np.where((i % 4 == 0) | (i % 4 == 1), below[:, 0], inside[:, 0])      # both, only 6, only 8, none -- sixteen of each in a wave
    q[:, 8] = np.where((i % 4 == 0) | (i % 4 == 2), below[:, 1], inside[:, 1])
    qd[:, :12] = rng.uniform(-10.0, 10.0, (N, 12))
    ora.set_state(qpos=q, qvel=qd)
    tq = ora.get_state()["qpos"]
    assert not (np.abs(tq[:, :6]) > ARM_HI).any() and not (np.abs(tq[:, [7, 9]]) > FINGER_HI).any()      # gear rows only: a remote sub-step
    sync_oracle_to(envs, ora)
    envs.counters(clear=True)
    a = rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    assert flags_equal
    eq, ev, ew, _ = rp.state_errors(envs, ora, relative_warm=True)
    assert envs.counters()["bad_state_resets"] == 0
    qacc = np.abs(ora.get_state()["warm"]).max()
    envs.close()
    w = dict(obs=float(e.max()), q=float(eq.max()), v=float(ev.max()), w=float(ew.max()))
    print(f"\n{controller} mixed gear rows, all twelve dofs fast: " + " ".join(f"{k} {v:.3e}" for k, v in w.items()) + f"   max|qacc| {qacc:.3e}")
    return w


def check_bad_lanes():
    """The states and assertions of test_gpu_reach_remote_solve.py's test_bad_lane_in_a_remote_substep (its docstring says what they are)."""
    envs, ora, rng = rp.running_pair("joint", 1, 47)
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
    eq, ev, ew, (gq, gv, gw) = rp.state_errors(envs, ora)
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
