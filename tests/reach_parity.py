"""The harness of the Reach parity tests (tests/test_gpu_reach_*.py): what they share, once.  Not collected.

Those files hold their docstrings, case lists, bounds tables, path checks and tests; the layout of a run, the gear states most of them start
from, the recording of an oracle run, the engine side of a comparison and the "running pair" start are here.  The bounds of those files were
measured on the states this module makes: put_gear_case's body and the order of its rng draws are part of every table that names them.
Measurements that more than one file runs are in tests/reach_measures.py.
"""
from __future__ import annotations

import numpy as np

from tests.common import make_oracle, make_pair, step_errors, sync_state  # noqa: F401  (sync_state: the harness's own name for it)

N = 165                                              # two full workgroups and a ragged one of 37 lanes
SUBSTEPS = 20
SEED = 61                                            # of engine and oracle in the files that run put_gear_case's states as they are
ARM_HI = 2.96706                                     # jnt_range[0][1] of the mycobot280 tables
GEAR_LO, GEAR_HI, FINGER_HI = 0.0, 0.7, 0.872664     # the gear joints' range; the finger joints' is +-FINGER_HI


# ----------------------------------------------------------------------------------------------------------------------------- layout
def groups(n):
    """The lanes of every workgroup of an engine of n environments."""
    return [slice(g, min(g + 64, n)) for g in range(0, n, 64)]


def show(mask):
    """[sub-steps, workgroups] bool -> one X / . string per workgroup."""
    return " | ".join("".join("X" if x else "." for x in mask[:, g]) for g in range(mask.shape[1]))


def limit_rows_of(q):
    """Per lane of qpos q [n, >= 10]: (an arm row, a gear row, a finger row) is violated."""
    arm = (np.abs(q[:, :6]) > ARM_HI).any(axis=1)
    gear = (q[:, [6, 8]] < GEAR_LO).any(axis=1) | (q[:, [6, 8]] > GEAR_HI).any(axis=1)
    fing = (np.abs(q[:, [7, 9]]) > FINGER_HI).any(axis=1)
    return arm, gear, fing


def per_group(mask, n):
    """[n] bool -> per workgroup: some lane of it is set."""
    return [mask[sl].any() for sl in groups(n)]


# ----------------------------------------------------------------------------------------------------------------------------- states
def outside(rng, n, upper):
    """Gear angles 1e-3 .. 5e-3 rad beyond the lower limit (upper[i] false) or the upper one."""
    d = rng.uniform(1e-3, 5e-3, n)
    return np.where(upper, GEAR_HI + d, GEAR_LO - d)


def inside(rng, n, upper, near=False):
    """Gear angles inside the range, in its lower or upper part (the gear coupling pulls the two joints together): well inside, or
    (near) 2e-3 .. 8e-3 rad from the limit."""
    d = rng.uniform(2e-3, 8e-3, n) if near else rng.uniform(0.05, 0.3, n)
    return np.where(upper, GEAR_HI - d, GEAR_LO + d)


def put_gear_case(case, ora, rng, n):
    """Write the case's state into the oracle; returns the float32 action every sub-step takes.  The cases are those of
    tests/test_gpu_reach_after_s3.py's docstring (all but `arm`, which tests/reach_measures.py's slot_oracle_run adds on top of `mixed`)."""
    s = ora.get_state()
    q, qd = s["qpos"].copy(), s["qvel"].copy()
    i = np.arange(n)
    a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
    up = i % 2 == 1
    has6, has8 = np.zeros(n, bool), np.zeros(n, bool)
    if case == "row6": has6[:] = True
    elif case == "row8": has8[:] = True
    elif case in ("both_lower", "both_upper"):
        has6[:] = True; has8[:] = True; up = np.full(n, case == "both_upper")
    elif case in ("mixed", "switch", "reset"):
        has6 = (i % 4 == 0) | (i % 4 == 1); has8 = (i % 4 == 0) | (i % 4 == 2); up = (i // 4) % 2 == 1
    near = case in ("row6", "row8")                  # one row in every lane: the other joint just inside, or the gear coupling lifts the row at once
    q[:, 6] = np.where(has6, outside(rng, n, up), inside(rng, n, up, near))
    q[:, 8] = np.where(has8, outside(rng, n, up), inside(rng, n, up, near))
    qd[:, 6] = rng.uniform(-1.0, 1.0, n); qd[:, 8] = rng.uniform(-1.0, 1.0, n)
    a[:, 6] = np.where(up, 1.0, -1.0)                # the gripper servo pushes towards the limit the lane's rows are on
    if case == "crossing":
        # lane % 4: 0 inside the lower limit moving out, 1 outside it moving in, 2 inside the upper limit moving out, 3 outside it moving in
        c = i % 4
        start = np.select([c == 0, c == 1, c == 2], [GEAR_LO + 2e-3, GEAR_LO - 3e-3, GEAR_HI - 2e-3], GEAR_HI + 3e-3)
        speed = np.select([c == 0, c == 1, c == 2], [-1.0, 2.0, 1.0], -2.0)
        for j in (6, 8):
            q[:, j] = start + rng.uniform(-5e-4, 5e-4, n); qd[:, j] = speed * rng.uniform(0.8, 1.2, n)
        a[:, 6] = np.where(c >= 2, 1.0, -1.0)
    if case == "switch":
        x = (i % 64 == 5) | (i % 64 == 30)
        q[x, 0] = ARM_HI - 0.02; qd[x, 0] = rng.uniform(7.5, 8.5, int(x.sum())); a[x, 0] = 1.0
    if case == "reset":
        el = s["elapsed"].copy(); el[i % 5 == 2] = 40
        ora.set_state(elapsed=el)
    ora.set_state(qpos=q, qvel=qd)
    return a


def episode_limit(case):
    """max_episode_steps of oracle and engine for put_gear_case's `case`: `reset` alone ends episodes."""
    return 50 if case == "reset" else 10 ** 9


# -------------------------------------------------------------------------------------------------------------------------- recording
def oracle(n, frame_skip, seed, max_episode_steps=10 ** 9, table=None, controller="joint", running=None):
    """A CPU oracle after its reset: the counterpart of `engine`.  `running`: an rng; the oracle then takes one ordinary step with its
    first draw, so that warm start, lagged q and ctrl are those of a running episode."""
    ora = make_oracle(n, controller_type=controller, reward_type="dense", seed=seed, frame_skip=frame_skip,
                      max_episode_steps=max_episode_steps, table=table)
    ora.reset(seed=seed)
    if running is not None: ora.step(running.uniform(-1, 1, (n, ora.act_dim)).astype(np.float32))
    return ora


def record_substeps(ora, a, k=SUBSTEPS, each=None):
    """k steps of `ora` with action a: dict(pre / post = the state before / after every step, out = the step's outputs).
    `each(i, pre, out)` runs straight after step i, before the state after it is read."""
    r = dict(pre=[], out=[], post=[])
    for i in range(k):
        pre = ora.get_state()
        o = ora.step(a)
        if each is not None: each(i, pre, o)
        r["pre"].append(pre); r["out"].append(o); r["post"].append(ora.get_state())
    return r


def replay_env_steps(ora, start, a, steps=1):
    """`steps` free-running steps of the fresh oracle `ora` (frame_skip = 20: whole env-steps) from state `start`:
    dict(env_pre = the state as the oracle holds it, env_out / env_post = outputs and state after every step)."""
    ora.set_state(**start)
    r = dict(env_pre=ora.get_state(), env_out=[], env_post=[])
    for _ in range(steps):
        r["env_out"].append(ora.step(a)); r["env_post"].append(ora.get_state())
    return r


def freeze(x):
    """Write-protect every array in x (an array, or dicts / lists / tuples of them); returns x."""
    if isinstance(x, np.ndarray): x.flags.writeable = False
    else:
        for y in (x.values() if isinstance(x, dict) else x): freeze(y)
    return x


# ------------------------------------------------------------------------------------------------------------------------ engine side
def engine(n, frame_skip, seed, max_episode_steps=10 ** 9, table=None, controller="joint"):
    """A HIP engine after its reset, counters cleared."""
    from mycobotgym_amd import MyCobotVecEnv
    envs = MyCobotVecEnv(n, device="cuda:0", has_object=False, controller_type=controller, reward_type="dense", seed=seed,
                         frame_skip=frame_skip, max_episode_steps=max_episode_steps, table=table)
    envs.reset(seed=seed)
    envs.counters(clear=True)
    return envs


def step_errors_against(envs, step_result, o, so, what):
    """Worst errors of one engine step's outputs (envs.step's tuple) and the state it left against the oracle's (o, so): dict(obs, q, v, w),
    w relative to the lane's largest |qacc| (absolute where that is zero: a lane reset in the step); flags and counters must agree."""
    obs, rew, term, trunc, info = step_result
    assert np.array_equal(obs["desired_goal"].cpu().numpy(), o["desired"]), what
    assert np.array_equal(term.cpu().numpy(), o["terminated"].astype(bool)) and np.array_equal(trunc.cpu().numpy(), o["truncated"].astype(bool)), what
    assert np.array_equal(info["is_success"].cpu().numpy(), o["is_success"].astype(bool)), what
    e = max(float(np.abs(obs["observation"].cpu().numpy() - o["obs"]).max()), float(np.abs(obs["achieved_goal"].cpu().numpy() - o["achieved"]).max()),
            float(np.abs(rew.cpu().numpy() - o["reward"]).max()))
    st = envs.get_state()
    gq, gv, gw = (st[x].cpu().numpy().T for x in ("qpos", "qvel", "warm"))
    assert all(np.isfinite(x).all() for x in (gq, gv, gw)), what
    assert np.array_equal(st["elapsed"].cpu().numpy(), so["elapsed"]) and np.array_equal(st["episode"].cpu().numpy(), so["episode"]), what
    ew, den = np.abs(gw - so["warm"]).max(axis=1), np.abs(so["warm"]).max(axis=1)
    ew = np.where(den > 0, ew / np.where(den > 0, den, 1.0), ew)
    return dict(obs=e, q=float(np.abs(gq - so["qpos"]).max()), v=float(np.abs(gv - so["qvel"]).max()), w=float(ew.max()))


def worst(a, b):
    return {k: max(a[k], b[k]) for k in a}


def within(w, b):
    return w["obs"] <= b["obs"] and w["q"] <= b["q"] and w["v"] <= b["v"] and w["w"] <= b["w"]


def _measure(r, envs, pre, steps, label):
    import torch
    a = torch.as_tensor(r["action"].copy())
    w = dict(obs=0.0, q=0.0, v=0.0, w=0.0)
    for k, (o, so) in enumerate(steps):
        if pre is not None: sync_state(envs, pre[k])
        w = worst(w, step_errors_against(envs, envs.step(a), o, so, (label, k)))
    assert envs.counters()["bad_state_resets"] == 0
    envs.close()
    print(f"{label}: " + " ".join(f"{x} {v:.3e}" for x, v in w.items()))
    return w


def measure_substeps(r, make_engine, label):
    """Worst errors over the recorded single sub-steps of r (record_substeps' keys, and `action`) and all lanes: the engine
    make_engine(frame_skip = 1) takes the oracle's state before each sub-step and is compared with the oracle after it."""
    return _measure(r, make_engine(1), r["pre"], zip(r["out"], r["post"]), label)


def measure_env_steps(r, make_engine, label):
    """Worst errors after each recorded whole env-step of r (replay_env_steps' keys, and `action`) over all lanes: the engine
    make_engine(frame_skip = 20) takes the oracle's start state and runs on from its own."""
    envs = make_engine(20)
    sync_state(envs, r["env_pre"])
    return _measure(r, envs, None, zip(r["env_out"], r["env_post"]), label)


# ----------------------------------------------------------------------------------------------------------------------- running pair
def running_pair(controller, frame_skip, seed, n=N, rng=None, steps=1, **kw):
    """Engine and oracle after a reset and `steps` ordinary steps from identical state: warm start, lagged q and ctrl are those of a
    running episode.  -> (envs, ora, rng); the actions are the first draws of rng (default_rng(seed) unless one is given).  IK at
    frame_skip = 1 runs with control_steps = 1.  **kw: further arguments of tests.common.make_pair."""
    kw = {**dict(controller_type=controller, reward_type="dense", seed=seed, max_episode_steps=10 ** 9, frame_skip=frame_skip), **kw}
    if controller == "IK" and frame_skip == 1: kw["control_steps"] = 1
    envs, ora = make_pair(n, **kw)
    envs.reset(seed=seed); ora.reset(seed=seed)
    if rng is None: rng = np.random.default_rng(seed)
    for _ in range(steps):
        a = rng.uniform(-1, 1, (n, envs.action_dim)).astype(np.float32)
        sync_state(envs, ora.get_state())
        _, flags_equal, _ = step_errors(envs, ora, a)
        assert flags_equal
    return envs, ora, rng


def state_errors(envs, ora, relative_warm=False):
    """Per-lane errors of the engine's state against the oracle's: (qpos [n], qvel [n], warm [n], the engine's (qpos, qvel, warm));
    relative_warm: the warm start (= qacc) relative to the lane's largest |qacc|."""
    st, so = envs.get_state(), ora.get_state()
    gq, gv, gw = (st[k].cpu().numpy().T for k in ("qpos", "qvel", "warm"))
    assert all(np.isfinite(x).all() for x in (gq, gv, gw, so["qpos"], so["qvel"], so["warm"]))
    w = np.abs(gw - so["warm"]).max(axis=1)
    if relative_warm: w = w / np.abs(so["warm"]).max(axis=1)
    return np.abs(gq - so["qpos"]).max(axis=1), np.abs(gv - so["qvel"]).max(axis=1), w, (gq, gv, gw)
