"""The episode-tail rule of tests/indep_episode.py against the CPU oracle's env layer, by the two-pass scheme the GPU test uses
(tests/test_gpu_episode_tail.py): the goal is state that no step's physics reads, so a probe pass finds the step's achieved goal A and a
second pass from the same pre-state, with goals placed around A, has a known outcome.  This validates the rule, the scenario builder
and its conditions before a GPU is involved."""
import numpy as np
import pytest

from tests.common import bits, make_oracle
from tests.indep_episode import (SCENARIOS, check_conditions, dense_reward_ulps, episode_rule, expected_by_table, scenario_codes,
                                 scenario_goals, scenario_priors)

THRESHOLD = 2.0 ** -7
FAR_GOAL = np.array([1.0, 1.0, 1.5])
N = 24

CONFIGS = {
    "reach-joint-sparse": dict(has_object=False, controller_type="joint", reward_type="sparse"),
    "reach-IK-dense": dict(has_object=False, controller_type="IK", reward_type="dense"),
    "reach-mocap-sparse": dict(has_object=False, controller_type="mocap", reward_type="sparse"),
    "pnp-joint-dense": dict(has_object=True, controller_type="joint", reward_type="dense"),
    "hidden-cube-reach-shaping": dict(has_object=False, controller_type="joint", reward_type="reward_shaping"),
}


def test_exact_threshold_goal_exists_for_every_coordinate():
    """Code 4's condition on the coordinate ranges the achieved goals live in: for 1e5 float64 coordinates from each interval, one of
    the two signs gives fl((a + s thr) - a) == s thr for all of them, and a fixed sign for at least 97.7 %."""
    rng = np.random.default_rng(0)
    for lo, hi in ((-0.3, 0.3), (0.05, 0.5), (-0.12, 0.12)):
        a = rng.uniform(lo, hi, 100000)
        plus = ((a + THRESHOLD) - a == THRESHOLD) & (a - (a + THRESHOLD) == -THRESHOLD)
        minus = ((a - THRESHOLD) - a == -THRESHOLD) & (a - (a - THRESHOLD) == THRESHOLD)
        assert (plus | minus).all()
        assert plus.mean() >= 0.977 and minus.mean() >= 0.977, (lo, hi, plus.mean(), minus.mean())


def test_builder_meets_its_conditions_on_the_workspace():
    """The scenario builder on 2000 achieved goals per coordinate range: every code's condition holds, code 4 included -- its goal is
    exactly one threshold away as rational numbers too (for a coordinate smaller than the threshold neither sign may be, and another
    axis serves)."""
    rng = np.random.default_rng(1)
    for lo, hi in ((-0.3, 0.3), (0.05, 0.5), (-0.12, 0.12)):
        A = np.column_stack([rng.uniform(lo, hi, 2000), rng.uniform(-0.12, 0.12, 2000), rng.uniform(0.05, 0.5, 2000)])
        codes = np.arange(2000) % 8
        G = scenario_goals(A, codes, THRESHOLD, rng)
        d = check_conditions(A, G, codes, THRESHOLD)
        assert (d[codes == 4] == THRESHOLD).all()


def test_the_rule_on_hand_made_numbers():
    """The rule itself on numbers worked out by hand: a 3-4-5 triangle scaled to the threshold."""
    thr = 0.5
    A = np.zeros((4, 3))
    G = np.array([[0.3, 0.4, 0.0], [0.3, 0.4, 1e-9], [0.3, 0.4 - 1e-9, 0.0], [3.0, 4.0, 0.0]])        # d = thr, just above, just below, 5
    G[0] = [0.5, 0.0, 0.0]                                                                             # exactly thr (0.3, 0.4 are not binary fractions)
    kw = dict(elapsed=[0, 48, 49, 50], ep_return=[0.0, -1.0, -2.0, -3.0], ep_length=[0, 48, 49, 50], episode=[0, 1, 2, 3],
              threshold=thr, max_episode_steps=50)
    r = episode_rule(np.ones((4, 2)), A, G, reward_type="sparse", **kw)
    assert r["is_success"].tolist() == [False, False, True, False] == r["terminated"].tolist()
    assert r["truncated"].tolist() == [False, False, True, True]
    assert r["reward"].dtype == np.float32 and bits(r["reward"]).tolist() == [0x80000000, 0xBF800000, 0x80000000, 0xBF800000]
    assert r["ep_return_out"].tolist() == [0.0, -2.0, -2.0, -4.0] and r["ep_length_out"].tolist() == [1, 49, 50, 51]
    assert r["elapsed"].tolist() == [1, 49, 0, 0] and r["episode"].tolist() == [0, 1, 3, 4]
    assert r["ep_return"].tolist() == [0.0, -2.0, 0.0, 0.0] and r["ep_length"].tolist() == [1, 49, 0, 0]
    r = episode_rule(np.ones((4, 2)), A, G, reward_type="dense", auto_reset=False, **kw)
    assert r["reward"][0] == -0.5 and r["reward"][3] == -5.0 and r["elapsed"].tolist() == [1, 49, 50, 51] and r["episode"].tolist() == [0, 1, 2, 3]


@pytest.mark.parametrize("name", list(CONFIGS))
def test_oracle_follows_the_rule(name):
    kw = dict(CONFIGS[name], distance_threshold=THRESHOLD, seed=21, n_threads=4)
    reward_type, max_steps = kw["reward_type"], 50
    probe, test = make_oracle(N, **kw), make_oracle(N, **kw)
    rng = np.random.default_rng(5)
    far = np.tile(FAR_GOAL, (N, 1))
    third = None
    acts = [rng.uniform(-1, 1, (N, probe.act_dim)).astype(np.float32) for _ in range(5)]
    for o in (probe, test):                          # pre-state S: reset, three random steps with far goals
        o.reset(seed=21)
        o.set_state(goal=far)
        for a in acts[:3]:
            third = o.step(a)
            assert not third["truncated"].any()
    S = probe.get_state()
    for k, v in test.get_state().items():
        assert np.array_equal(bits(v), bits(S[k])), k
    codes = scenario_codes(N, N, "table")
    prior = scenario_priors(codes, max_steps)
    prior["ep_return"], prior["ep_length"] = third["ep_return"].copy(), third["ep_length"].copy()        # the oracle's set_state has neither
    assert (prior["ep_length"] == 3).all()

    a = acts[3]
    probe.set_state(**dict(S, goal=far, episode=prior["episode"]))
    op = probe.step(a)
    assert not op["truncated"].any() and not op["is_success"].any()
    G = scenario_goals(op["achieved"], codes, THRESHOLD, np.random.default_rng(6))
    check_conditions(op["achieved"], G, codes, THRESHOLD)
    test.set_state(**dict(S, goal=G, elapsed=prior["elapsed"], episode=prior["episode"]))
    ot = test.step(a)

    rule = episode_rule(op["obs"], op["achieved"], G, prior["elapsed"], prior["ep_return"], prior["ep_length"], prior["episode"],
                        threshold=THRESHOLD, reward_type=reward_type, max_episode_steps=max_steps,
                        reward=ot["reward"] if reward_type == "reward_shaping" else None)
    fin = rule["finished"]
    table = expected_by_table(codes)
    for k in ("is_success", "terminated", "truncated"):
        assert np.array_equal(rule[k], table[k]), k                    # the builder made what the table says
        assert np.array_equal(ot[k].astype(bool), rule[k]), k
    assert fin.sum() == 5 * (N // 8) and (~fin).sum() == 3 * (N // 8)
    # the second pass achieved A bit for bit
    got_A = np.where(fin[:, None], ot["final_achieved"], ot["achieved"])
    assert np.array_equal(bits(got_A), bits(op["achieved"]))
    if reward_type == "sparse":
        assert np.array_equal(bits(ot["reward"]), bits(rule["reward"].astype(np.float64)))          # signed zero included
        assert (bits(ot["reward"])[codes == 4] == 0x8000000000000000).all() and (ot["reward"][codes == 3] == -1.0).all()
    elif reward_type == "dense":
        ulps = dense_reward_ulps(ot["reward"], rule["distance"])
        print(f"\n[{name}] dense reward: worst |reward + d| = {ulps.max():.2f} x 2^-53 d")
        assert ulps.max() <= 4.0
    assert np.array_equal(ot["ep_length"], rule["ep_length_out"])
    assert np.array_equal(bits(ot["ep_return"]), bits(prior["ep_return"] + ot["reward"]))
    assert np.array_equal(bits(ot["final_obs"][fin]), bits(op["obs"][fin]))
    assert np.array_equal(bits(ot["final_achieved"][fin]), bits(op["achieved"][fin]))
    assert np.array_equal(bits(ot["final_desired"][fin]), bits(G[fin]))
    assert not ot["final_obs"][~fin].any() and not ot["final_desired"][~fin].any()                   # untouched where nothing ended
    assert np.array_equal(bits(ot["desired"][~fin]), bits(G[~fin])) and np.array_equal(bits(ot["obs"][~fin]), bits(op["obs"][~fin]))
    st, sp = test.get_state(), probe.get_state()
    assert np.array_equal(st["elapsed"], rule["elapsed"]) and np.array_equal(st["episode"], rule["episode"])
    for k in ("qpos", "qvel", "ctrl", "warm", "qpos_lag"):              # a lane that did not finish is the probe's, whatever its neighbours did
        assert np.array_equal(bits(st[k][~fin]), bits(sp[k][~fin])), k
    assert np.array_equal(bits(st["goal"][~fin]), bits(G[~fin]))
    # after the reset: a third oracle with the same episode numbers resets exactly the finished lanes
    third_o = make_oracle(N, **kw)
    third_o.reset(seed=21)
    third_o.set_state(**dict(S, episode=prior["episode"]))
    r_obs, r_ag, r_dg = third_o.reset(mask=fin)
    assert np.array_equal(bits(ot["desired"][fin]), bits(r_dg[fin])) and np.array_equal(bits(st["goal"][fin]), bits(r_dg[fin]))
    assert np.array_equal(bits(ot["obs"][fin]), bits(r_obs[fin])) and np.array_equal(bits(ot["achieved"][fin]), bits(r_ag[fin]))
    assert np.array_equal(st["episode"], third_o.get_state()["episode"])
    # one more step: the statistics of the restarted lanes begin again, the others carry on
    o2 = test.step(acts[4])
    assert np.array_equal(o2["ep_length"], rule["ep_length"] + 1)
    assert np.array_equal(bits(o2["ep_return"]), bits(rule["ep_return"] + o2["reward"]))
    assert np.array_equal(test.get_state()["elapsed"], np.where(o2["truncated"].astype(bool), 0, rule["elapsed"] + 1))
    late = np.array([SCENARIOS[int(c)][1] is not None for c in codes])
    assert late.sum() == 3 * (N // 8) and fin[late].all()
