"""The step kernels' episode tail -- goal distance, is_success, reward, terminated / truncated, the Monitor statistics, final_*, the
predicated in-kernel reset, the second observation and the stores -- against the rule restated in tests/indep_episode.py.

The goal is state that no step's physics reads, so the outcome of a step can be chosen exactly, in two passes from one pre-state S
(reset, three random steps with far goals): a probe engine steps with action a and far goals, which gives the step's achieved goal A
and observation; a test engine (same configuration and seed) steps from S with the same a and goals G placed around A by the scenario
table of tests/indep_episode.py, with chosen elapsed / episode / ep_return / ep_length.  The test engine must achieve A bit for bit;
everything the tail then does is a function of known numbers.

distance_threshold = 2^-7: a power of two makes d == threshold constructible (code 4: one coordinate differs by exactly 2^-7, the
others by nothing, so dx dx + dy dy + dz dz = 2^-14 and its square root 2^-7 are exact however the sum is contracted).

The dense reward's bound, |reward + d| <= 4 x 2^-53 d with d the extended-precision distance of the same float64 inputs: the three
differences are one rounding each from the same float64 inputs the rule reads (relative 2^-53 each, so every square, and with them
the sum of squares, is off by at most 2 x 2^-53 relative); along any path to the sum the products and additions are at most three
roundings, fused or not (3 x 2^-53 more: 5 x 2^-53); the square root halves the relative error (2.5 x 2^-53) and adds half an ulp of
its own (at most 2^-53 relative, reached only at the bottom of a binade): under 3 ulp, rounded up to 4 units of 2^-53 d.

Sizes: Reach 70 environments (one full wave and a ragged one of six lanes), PickAndPlace 40 (a workgroup of 32 and a ragged one whose
surplus lanes shadow environment 39); the ragged part runs in two layouts -- only its last lane finishes / no lane finishes -- so that
the wave-uniform `any lane done` branch is taken next to a wave that does not take it.

Measured on an MI355X: every configuration passes; worst dense-reward error 1.59 x 2^-53 d (Reach joint with block_gripper; 1.49 joint,
1.38 IK, 1.25 mocap, 1.36 PickAndPlace).  Each of these, made in a scratch build of the kernels, fails tests here and nothing else:
`<` to `<=` in `succ` (all 28 tests), `>` to `>=` in the sparse reward (the 12 sparse ones), the `done` predicate dropped from one
select of reset_env / reset_envp (qvel: all Reach tests; dr_scale: the domain-randomised PickAndPlace ones), the return not cleared on
reset (all 24 with auto-reset), final_achieved stored after the reset (the same 24).
"""
import ctypes as C

import numpy as np
import pytest

from tests.common import bits
from tests.indep_episode import (check_conditions, dense_reward_ulps, episode_rule, expected_by_table, scenario_codes, scenario_goals,
                                 scenario_priors)

pytestmark = pytest.mark.gpu

THRESHOLD = 2.0 ** -7
SEED = 21
MAX_STEPS = 50
FAR_GOAL = np.array([1.0, 1.0, 1.5])
DR = {"mass": (0.5, 2.0), "friction": (0.5, 1.5)}
STATE_FIELDS = ("qpos", "qvel", "ctrl", "warm", "qpos_lag", "episode", "dr_scale")       # + goal, elapsed, ep_return, ep_length: the rule's
SENTINEL = 0xA5

REACH = {f"reach-{c}-{r}": dict(has_object=False, controller_type=c, reward_type=r) for c in ("joint", "IK", "mocap") for r in ("sparse", "dense")}
PNP = {
    "pnp-joint-sparse": dict(has_object=True, controller_type="joint", reward_type="sparse"),
    "pnp-IK-dense-dr": dict(has_object=True, controller_type="IK", reward_type="dense", domain_randomization=DR),
    "pnp-mocap-dense": dict(has_object=True, controller_type="mocap", reward_type="dense"),
}
OTHERS = {       # name -> (kwargs, N, first block)
    "hidden-cube-reach-shaping": (dict(has_object=False, controller_type="joint", reward_type="reward_shaping"), 40, 32),
    "reach-joint-dense-block-gripper": (dict(has_object=False, controller_type="joint", reward_type="dense", block_gripper=True), 70, 64),
    "pnp-joint-dense-block-gripper": (dict(has_object=True, controller_type="joint", reward_type="dense", block_gripper=True), 40, 32),
    "pnp-IK-sparse-fetch": (dict(has_object=True, controller_type="IK", reward_type="sparse", fetch_env=True), 40, 32),
}


def host(x):
    return {k: host(v) for k, v in x.items()} if isinstance(x, dict) else x.cpu().numpy()


def engine(n, kw, auto_reset=True):
    from mycobotgym_amd import MyCobotVecEnv
    return MyCobotVecEnv(n, distance_threshold=THRESHOLD, seed=SEED, auto_reset=auto_reset, max_episode_steps=MAX_STEPS, **kw)


def step_outputs(out):
    obs, rew, term, trunc, info = out
    f = info["final_observation"]
    return host({"obs": obs["observation"], "achieved": obs["achieved_goal"], "desired": obs["desired_goal"], "reward": rew,
                 "terminated": term, "truncated": trunc, "is_success": info["is_success"], "final_obs": f["observation"],
                 "final_achieved": f["achieved_goal"], "final_desired": f["desired_goal"], "ep_return": info["episode"]["r"],
                 "ep_length": info["episode"]["l"]})


def prepare(kw, n, codes):
    """The probe pass -> everything the second pass needs: pre-state S with the scenario's goals and priors, the action, the probe's
    outputs and state after its step, the rule's inputs."""
    import torch
    probe = engine(n, kw)
    rng = np.random.default_rng(5)
    acts = [torch.as_tensor(rng.uniform(-1, 1, (n, probe.action_dim)).astype(np.float32), device=probe.device) for _ in range(5)]
    far = np.tile(FAR_GOAL, (n, 1))
    probe.reset(seed=SEED)
    probe.set_state(goal=far.T.copy())
    for a in acts[:3]:
        _, _, _, trunc, _ = probe.step(a)
        assert not bool(trunc.any())
    prior = scenario_priors(codes, MAX_STEPS)
    S = {k: v.clone() for k, v in probe.get_state().items()}
    S["episode"] = torch.as_tensor(prior["episode"], device=probe.device)          # (no step's physics reads it: the probe carries the test's)
    probe.set_state(**S)
    op = step_outputs(probe.step(acts[3]))
    assert not op["truncated"].any() and not op["is_success"].any()
    sp = host(probe.get_state())
    probe.close()
    G = scenario_goals(op["achieved"], codes, THRESHOLD, np.random.default_rng(6))
    d = check_conditions(op["achieved"], G, codes, THRESHOLD)                       # fails, does not skip
    S2 = dict(S, goal=torch.as_tensor(G.T.copy(), device=probe.device), elapsed=torch.as_tensor(prior["elapsed"], device=probe.device),
              ep_return=torch.as_tensor(prior["ep_return"], device=probe.device), ep_length=torch.as_tensor(prior["ep_length"], device=probe.device))
    return {"S": S, "S2": S2, "acts": acts, "a": acts[3], "op": op, "sp": sp, "G": G, "d": d, "prior": prior, "codes": codes}


def rule_for(P, kw, auto_reset, reward=None):
    p = P["prior"]
    return episode_rule(P["op"]["obs"], P["op"]["achieved"], P["G"], p["elapsed"], p["ep_return"], p["ep_length"], p["episode"],
                        threshold=THRESHOLD, reward_type=kw["reward_type"], max_episode_steps=MAX_STEPS, auto_reset=auto_reset, reward=reward)


def check_step_against_rule(name, P, kw, ot, raw_reward, auto_reset=True):
    """Flags, reward and statistics of the second pass against the rule -> the rule's outputs."""
    codes, prior = P["codes"], P["prior"]
    shaped = kw["reward_type"] == "reward_shaping"
    rule = rule_for(P, kw, auto_reset, reward=raw_reward if shaped else None)
    table = expected_by_table(codes)
    for k in ("is_success", "terminated", "truncated"):
        assert np.array_equal(rule[k], table[k]), k
        assert np.array_equal(ot[k].astype(bool), rule[k]), (k, np.flatnonzero(ot[k].astype(bool) != rule[k]))
    worst = float("nan")
    if kw["reward_type"] == "sparse":
        assert raw_reward.dtype == np.float64 and np.array_equal(bits(raw_reward), bits(rule["reward"].astype(np.float64)))
        assert ot["reward"].dtype == np.float32 and np.array_equal(bits(ot["reward"]), bits(rule["reward"]))       # signed zero included
        assert (bits(ot["reward"])[codes == 4] == 0x80000000).all() and (ot["reward"][codes == 3] == -1.0).all()
    elif kw["reward_type"] == "dense":
        ulps = dense_reward_ulps(raw_reward, rule["distance"])
        worst = float(ulps.max())
        assert (raw_reward < 0).all() and worst <= 4.0, (worst, int(ulps.argmax()))
        rule = rule_for(P, kw, auto_reset, reward=raw_reward)          # checked: the statistics are one addition of that very number
    assert np.array_equal(ot["ep_length"], rule["ep_length_out"])
    assert np.array_equal(bits(ot["ep_return"]), bits(prior["ep_return"] + raw_reward))                             # one float64 addition
    lanes = {int(c): int((codes == c).sum()) for c in np.unique(codes)}
    print(f"\n[episode tail] {name}: lanes per scenario {lanes}; finished {int(rule['finished'].sum())} of {len(codes)}; "
          f"worst dense-reward error {worst:.2f} x 2^-53 d")
    return rule


def oracle_reset(kw, n, P, mask):
    """The oracle from the same pre-state and episode numbers, reset(mask) -> (obs, achieved, desired) after it, its episode numbers."""
    from tests.common import make_oracle
    ora = make_oracle(n, distance_threshold=THRESHOLD, seed=SEED, max_episode_steps=MAX_STEPS, **kw)
    ora.reset(seed=SEED)
    s = host({k: v for k, v in P["S"].items() if k != "seed"})
    nu = ora.model.nu
    ora.set_state(qpos=s["qpos"].T.copy(), qvel=s["qvel"].T.copy(), ctrl=s["ctrl"].T[:, 7 - nu:].copy(), warm=s["warm"].T.copy(),
                  qpos_lag=s["qpos_lag"].T.copy(), goal=P["G"], elapsed=P["prior"]["elapsed"], episode=P["prior"]["episode"])
    out = ora.reset(mask=mask)
    return out, ora.get_state()["episode"]


def run_case(name, kw, n, block, layout):
    import torch
    codes = scenario_codes(n, block, layout)
    P = prepare(kw, n, codes)
    op, sp, G, prior = P["op"], P["sp"], P["G"], P["prior"]
    test = engine(n, kw)
    test.set_state(**P["S2"])
    for k in ("final_obs", "final_achieved", "final_desired"):
        test._buf[k].view(torch.uint8).fill_(SENTINEL)
    ot = step_outputs(test.step(P["a"]))
    raw_reward = test._buf["reward"].cpu().numpy()
    st = host(test.get_state())
    test.close()

    rule = check_step_against_rule(f"{name} / {layout}", P, kw, ot, raw_reward)
    fin = rule["finished"]
    if layout == "last":
        assert fin[block:].tolist() == [False] * (n - block - 1) + [True]
    elif layout == "none":
        assert not fin[block:].any()
    assert fin[:block].sum() == 5 * (block // 8)
    # the second pass achieved A bit for bit
    got_A = np.where(fin[:, None], ot["final_achieved"], ot["achieved"])
    assert np.array_equal(bits(got_A), bits(op["achieved"])), np.flatnonzero((bits(got_A) != bits(op["achieved"])).any(axis=1))
    # finished lanes: the finished episode's last observation and goals
    assert np.array_equal(bits(ot["final_obs"][fin]), bits(op["obs"][fin]))
    assert np.array_equal(bits(ot["final_achieved"][fin]), bits(op["achieved"][fin]))
    assert np.array_equal(bits(ot["final_desired"][fin]), bits(G[fin]))
    # never-finished lanes: nothing was written
    for k in ("final_obs", "final_achieved", "final_desired"):
        assert (np.ascontiguousarray(ot[k][~fin]).view(np.uint8) == SENTINEL).all(), k
    # lanes not finished: outputs and the WHOLE state are the probe's, but for the four fields that follow the rule
    keep = ~fin
    assert np.array_equal(bits(ot["obs"][keep]), bits(op["obs"][keep])) and np.array_equal(bits(ot["desired"][keep]), bits(G[keep]))
    for k in STATE_FIELDS:
        assert np.array_equal(bits(st[k][..., keep]), bits(sp[k][..., keep])), (k, "a reset leaked into a lane that did not finish")
    assert np.array_equal(st["seed"], sp["seed"])
    assert np.array_equal(bits(st["goal"][:, keep]), bits(G[keep].T))
    for k in ("elapsed", "ep_length"):
        assert np.array_equal(st[k], rule[k]), k
    assert np.array_equal(bits(st["ep_return"]), bits(rule["ep_return"]))
    assert not st["elapsed"][fin].any() and not st["ep_length"][fin].any() and not bits(st["ep_return"][fin]).any()
    # after the reset: the oracle's reset of exactly these lanes, from the same episode numbers
    (r_obs, r_ag, r_dg), r_episode = oracle_reset(kw, n, P, fin)
    assert np.array_equal(bits(ot["desired"][fin]), bits(r_dg[fin])) and np.array_equal(bits(st["goal"][:, fin]), bits(r_dg[fin].T))
    assert np.abs(ot["obs"][fin] - r_obs[fin]).max() < 1e-14 and np.abs(ot["achieved"][fin] - r_ag[fin]).max() < 1e-14
    assert np.array_equal(st["episode"], r_episode) and np.array_equal(st["episode"], rule["episode"])


# ------------------------------------------------------------------------------------------------------------- the kernels
@pytest.mark.parametrize("layout", ["last", "none"])
@pytest.mark.parametrize("name", list(REACH))
def test_reach_tail(built, name, layout):
    run_case(name, REACH[name], 70, 64, layout)


@pytest.mark.parametrize("layout", ["last", "none"])
def test_reach_tail_one_wave_kernel(built, layout, monkeypatch):
    """MCG_NO_SPLIT=1 at construction: the one-wave Reach kernel (as test_two_wave_and_one_wave_kernels_agree selects it)."""
    monkeypatch.setenv("MCG_NO_SPLIT", "1")
    run_case("reach-joint-sparse (one-wave kernel)", REACH["reach-joint-sparse"], 70, 64, layout)


@pytest.mark.parametrize("layout", ["last", "none"])
@pytest.mark.parametrize("name", list(PNP))
def test_pickandplace_tail(built, name, layout):
    run_case(name, PNP[name], 40, 32, layout)


@pytest.mark.parametrize("name", list(OTHERS))
def test_tail_of_the_other_configurations(built, name):
    """The hidden-cube Reach ids (the PickAndPlace kernel with obs_dim 10 and hide_object), block_gripper (the tail branches on it just
    before the observation) and fetch_env (an action of 4 entries)."""
    kw, n, block = OTHERS[name]
    run_case(name, kw, n, block, "last")


# ------------------------------------------------------------------------------------------------------------ the raw ABI
def own_outputs(envs, names=None):
    """An mcg_step_out of the caller's own buffers, every byte a sentinel -> (struct, tensors by name)."""
    import torch
    from mycobotgym_amd import _abi
    n, D = envs.num_envs, envs.obs_dim
    shapes = {"obs": (n, D, 8), "achieved_goal": (n, 3, 8), "desired_goal": (n, 3, 8), "reward": (n, 8), "terminated": (n, 1),
              "truncated": (n, 1), "is_success": (n, 1), "final_obs": (n, D, 8), "final_achieved": (n, 3, 8), "final_desired": (n, 3, 8),
              "ep_return": (n, 8), "ep_length": (n, 4)}
    t = {k: torch.full(s, SENTINEL, dtype=torch.uint8, device=envs.device) for k, s in shapes.items() if names is None or k in names}
    return _abi.McgStepOut(**{k: v.data_ptr() for k, v in t.items()}), t


def raw_step(envs, a, out):
    import torch
    from mycobotgym_amd import _abi
    with torch.cuda.device(envs.device):
        _abi.check(envs._lib.mcg_step(envs._h, C.c_void_p(a.data_ptr()), None if out is None else C.byref(out), envs._stream()), "mcg_step")
    torch.cuda.synchronize(envs.device)


def as_array(t, dtype):
    """A byte buffer of own_outputs ([..., item size] uint8, tensor or array) as an array of `dtype`."""
    a = t if isinstance(t, np.ndarray) else t.cpu().numpy()
    return np.ascontiguousarray(a).view(dtype)[..., 0]


RAW = {"reach": (REACH["reach-joint-sparse"], 70), "pnp": (PNP["pnp-IK-dense-dr"], 40)}


@pytest.mark.parametrize("which", list(RAW))
def test_null_outputs(built, which):
    """"Any pointer of mcg_step_out may be NULL" (include/mcg.h): three engines step from the same state with the same action -- all
    twelve pointers, only reward and truncated, out = NULL.  The state afterwards is the same bit for bit, resets included, and the
    two outputs of the second are the first's."""
    kw, n = RAW[which]
    codes = scenario_codes(n, n, "table")
    P = prepare(kw, n, codes)
    states, outs = [], []
    for names in (None, ("reward", "truncated"), ()):
        e = engine(n, kw)
        e.set_state(**P["S2"])
        o, t = own_outputs(e, names)
        raw_step(e, P["a"], None if names == () else o)
        states.append(host(e.get_state())); outs.append({k: v.cpu().numpy() for k, v in t.items()})
        e.close()
    for k in states[0]:
        assert np.array_equal(bits(states[0][k]), bits(states[1][k])) and np.array_equal(bits(states[0][k]), bits(states[2][k])), k
    assert set(outs[1]) == {"reward", "truncated"} and not outs[2]
    for k in outs[1]:
        assert np.array_equal(outs[0][k], outs[1][k]), k
    trunc = as_array(outs[0]["truncated"], np.uint8).astype(bool)
    assert np.array_equal(trunc, expected_by_table(codes)["truncated"])
    assert (states[0]["elapsed"][trunc] == 0).all() and (states[0]["elapsed"][~trunc] > 0).all()          # resets happened


@pytest.mark.parametrize("which", list(RAW))
def test_auto_reset_off(built, which):
    """auto_reset = 0 through the state engine itself: flags and statistics are the rule's, final_* are never written, nothing is reset
    (elapsed = prior + 1, the goal is still G, the state is the probe's), and a second step reports `truncated` again for codes 5-7."""
    kw, n = RAW[which]
    codes = scenario_codes(n, n, "table")
    P = prepare(kw, n, codes)
    e = engine(n, kw, auto_reset=False)
    e.set_state(**P["S2"])
    o, t = own_outputs(e)
    raw_step(e, P["a"], o)
    f64 = lambda k: as_array(t[k], np.float64)
    ot = {"obs": f64("obs"), "achieved": f64("achieved_goal"), "desired": f64("desired_goal"), "reward": f64("reward"),
          "terminated": as_array(t["terminated"], np.uint8), "truncated": as_array(t["truncated"], np.uint8),
          "is_success": as_array(t["is_success"], np.uint8), "ep_return": f64("ep_return"), "ep_length": as_array(t["ep_length"], np.int32)}
    raw_reward = ot["reward"]
    if kw["reward_type"] == "sparse":
        ot["reward"] = raw_reward.astype(np.float32)
    rule = check_step_against_rule(f"{which}, auto_reset off", P, kw, ot, raw_reward, auto_reset=False)
    for k in ("final_obs", "final_achieved", "final_desired"):
        assert bool((t[k] == SENTINEL).all()), k
    assert np.array_equal(bits(ot["obs"]), bits(P["op"]["obs"])) and np.array_equal(bits(ot["achieved"]), bits(P["op"]["achieved"]))
    assert np.array_equal(bits(ot["desired"]), bits(P["G"]))
    st = host(e.get_state())
    for k in STATE_FIELDS:
        assert np.array_equal(bits(st[k]), bits(P["sp"][k])), k
    assert np.array_equal(st["elapsed"], P["prior"]["elapsed"] + 1) and np.array_equal(st["elapsed"], rule["elapsed"])
    assert np.array_equal(bits(st["goal"]), bits(P["G"].T))
    assert np.array_equal(st["ep_length"], rule["ep_length"]) and np.array_equal(bits(st["ep_return"]), bits(rule["ep_return"]))
    raw_step(e, P["acts"][4], o)
    again = as_array(t["truncated"], np.uint8).astype(bool)
    assert again[codes >= 5].all() and (codes >= 5).sum() >= 3 * (n // 8)
    assert np.array_equal(host(e.get_state())["elapsed"], P["prior"]["elapsed"] + 2)
    e.close()
