"""The episode tail of an environment step, restated in plain numpy from the reference's text -- TEST INFRASTRUCTURE ONLY.

What happens to one environment after the physics of a step, given the step's observation and achieved goal:

  * goal_distance (utils.py:24-26): the Euclidean norm of achieved - desired;
  * _is_success (mycobot.py:285-287): d < distance_threshold, strictly;
  * compute_reward (mycobot.py:289-298): sparse -(d > threshold).astype(np.float32) -- so -0.0 where d <= threshold, at d == threshold
    without a success --, dense -d, reward_shaping: not a function of the goals (an input here; the stage reward has tests of its own);
  * compute_terminated / compute_truncated (mycobot.py:390-400): both are is_success;
  * TimeLimit(max_episode_steps) (mycobotgym/__init__.py:34): counts the step, then truncated |= elapsed >= max_episode_steps;
  * Monitor: the episode's return ("r") and length ("l") are running sums that include the step that ends the episode;
  * the vector auto-reset (include/mcg.h:11-15): where terminated | truncated, the step's observation and goals become
    final_observation, the environment is reset inside the same step and the counters start again at zero.  The per-environment
    episode number (the position of the reset's random stream, include/mcg.h: mcg_state.episode) goes up by one there.

Distances are evaluated in np.longdouble from the float64 inputs, so a comparison with the threshold is decided with 11 more bits than
any float64 evaluation has; `scenario_goals` builds goals whose distance is either far from the threshold in that precision
(|d / thr - 1| >= 1e-10, checked by `check_conditions`) or exactly on it in every precision (one coordinate differs by a power of
two, the other two by nothing).

Nothing here was written from the engine's kernels or from the CPU oracle's env layer.
"""
from __future__ import annotations

import numpy as np

REWARD_TYPES = ("sparse", "dense", "reward_shaping")

# scenario code -> (what the goal is, as a multiple of the threshold from the achieved goal; None = 1 m away), elapsed before the step
# relative to max_episode_steps (None = 5), and what the reference's text says must happen: (is_success, time limit reached)
FAR = None
SCENARIOS = {
    0: (FAR, None, (False, False)),               # nothing ends
    1: (0.5, None, (True, False)),                # success
    2: (1.0 - 1e-9, None, (True, False)),         # success, just inside
    3: (1.0 + 1e-9, None, (False, False)),        # no success, just outside
    4: ("exact", None, (False, False)),           # d == threshold: no success, no end, sparse reward -0.0
    5: (FAR, -1, (False, True)),                  # the time limit alone: truncated & !terminated
    6: (0.5, -1, (True, True)),                   # both
    7: (FAR, 0, (False, True)),                   # already over the limit: truncated
}
NON_ENDING = (0, 3, 4)
ELAPSED_SMALL = 5


def scenario_codes(n: int, block: int, layout: str) -> np.ndarray:
    """Codes by env % 8 in the first `block` environments (every wave is mixed).  The ragged rest takes non-ending codes (0, 3, 4 in
    turn); layout "last": its last environment alone finishes (code 6, success and time limit), layout "none": none of it does.
    layout "table": env % 8 throughout."""
    codes = np.arange(n) % 8
    if layout == "table":
        return codes
    assert layout in ("last", "none") and 0 < block < n
    for i in range(block, n):
        codes[i] = NON_ENDING[(i - block) % 3]
    if layout == "last":
        codes[n - 1] = 6
    return codes


def scenario_priors(codes: np.ndarray, max_episode_steps: int) -> dict:
    """elapsed by the table; distinct per-environment statistics and episode numbers (the reset draws of one wave are keyed by
    different episodes)."""
    n = len(codes)
    env = np.arange(n)
    elapsed = np.array([ELAPSED_SMALL if SCENARIOS[c][1] is None else max_episode_steps + SCENARIOS[c][1] for c in codes], dtype=np.int32)
    return {"elapsed": elapsed, "ep_return": -1.5 - 0.01 * env, "ep_length": elapsed.copy(), "episode": (1 + env % 5).astype(np.int32)}


def scenario_goals(achieved: np.ndarray, codes: np.ndarray, threshold: float, rng: np.random.Generator) -> np.ndarray:
    """G per environment from the achieved goal A of the step (float64 [n, 3]).  Code 4: G = A + s thr e_k for an axis k and a sign s
    for which the float64 G_k lies exactly thr from A_k -- as rational numbers, and therefore also as the float64 difference either
    way round (`_exactly`).  fl(A_k + s thr) is that number unless the sum had to be rounded, which the sign that shrinks |A_k| avoids
    for |A_k| >= thr; for a smaller |A_k| another axis serves (z is never that small).  A lane without any fails the build."""
    A = np.asarray(achieved, dtype=np.float64)
    n = len(codes)
    assert A.shape == (n, 3)
    G = np.empty_like(A)
    for i, c in enumerate(codes):
        what = SCENARIOS[int(c)][0]
        u = rng.normal(size=3)
        u /= np.linalg.norm(u)
        if what is FAR:
            G[i] = A[i] + 1.0 * u
        elif what == "exact":
            G[i] = A[i]
            k0, s0 = int(rng.integers(3)), int(rng.integers(2))
            for j in range(6):                               # the first (axis, sign), from a random start, that is exact
                k, s = (k0 + j // 2) % 3, (1.0, -1.0)[(s0 + j) % 2]
                g = A[i, k] + s * threshold
                if _exactly(threshold, A[i, k], g):
                    G[i, k] = g
                    break
            else:
                raise AssertionError(f"env {i}: no exact goal at distance {threshold} from {A[i]!r}")
        else:
            G[i] = A[i] + (what * threshold) * u
    return G


def _exactly(threshold, a, g) -> bool:
    from fractions import Fraction
    return (abs(Fraction(float(g)) - Fraction(float(a))) == Fraction(float(threshold))
            and abs(g - a) == threshold and abs(a - g) == threshold)


def extended_distance(achieved, goal) -> np.ndarray:
    d = np.asarray(achieved, dtype=np.float64).astype(np.longdouble) - np.asarray(goal, dtype=np.float64).astype(np.longdouble)
    return np.sqrt((d * d).sum(axis=-1))


def check_conditions(achieved, goal, codes, threshold) -> np.ndarray:
    """The conditions under which the table's outcome is decided by the inputs alone; raises AssertionError otherwise (a test that
    calls this fails, it does not skip).  -> the extended-precision distances."""
    assert np.finfo(np.longdouble).nmant >= 63, "np.longdouble is not an extended format here"
    A, G = np.asarray(achieved, dtype=np.float64), np.asarray(goal, dtype=np.float64)
    d = extended_distance(A, G)
    ratio = d / np.longdouble(threshold)
    for i, c in enumerate(codes):
        if int(c) == 4:
            diff = A[i] - G[i]
            assert np.count_nonzero(diff) == 1 and np.abs(diff).max() == threshold, (i, diff)
            k = int(np.flatnonzero(diff)[0])
            assert _exactly(threshold, A[i, k], G[i, k]), (i, k)
            assert d[i] == np.longdouble(threshold), (i, d[i])
        else:
            assert abs(ratio[i] - 1) >= 1e-10, (i, int(c), ratio[i])
            want = SCENARIOS[int(c)][0]
            assert (ratio[i] < 1) == (want is not FAR and want < 1), (i, int(c), ratio[i])
    return d


def episode_rule(obs, achieved, goal, elapsed, ep_return, ep_length, episode, *, threshold, reward_type, max_episode_steps,
                 auto_reset=True, reward=None) -> dict:
    """One step's tail for n environments.  obs [n, D], achieved / goal [n, 3] float64: the step's observation and goals; elapsed,
    ep_return, ep_length, episode [n]: the bookkeeping BEFORE the step.  reward [n]: the step's reward where it is an input
    (reward_shaping; or, for dense, the float64 number an implementation reported, once that has been checked against `reward` of a
    call without it: the statistics are then one addition of that very number).

    -> reward (sparse: float32, else float64), terminated, truncated, is_success, distance (np.longdouble), ep_return_out,
       ep_length_out, finished (terminated | truncated), final_obs / final_achieved / final_desired (rows valid where finished &
       auto_reset), and the bookkeeping after the step: elapsed, ep_return, ep_length, episode."""
    assert reward_type in REWARD_TYPES
    obs, A, G = (np.asarray(x, dtype=np.float64) for x in (obs, achieved, goal))
    elapsed, ep_length, episode = (np.asarray(x, dtype=np.int64) for x in (elapsed, ep_length, episode))
    ep_return = np.asarray(ep_return, dtype=np.float64)
    d = extended_distance(A, G)
    thr = np.longdouble(threshold)
    is_success = d < thr                                                         # mycobot.py:287
    if reward is not None:
        r = np.asarray(reward, dtype=np.float64)
    elif reward_type == "sparse":
        r = -(d > thr).astype(np.float32)                                        # mycobot.py:293, the reference's own expression
    elif reward_type == "dense":
        r = (-d).astype(np.float64)                                              # mycobot.py:295
    else:
        raise ValueError("reward_shaping: the step's reward is an input")
    terminated = is_success.copy()                                               # mycobot.py:392-394
    elapsed_now = elapsed + 1                                                    # TimeLimit.step
    truncated = is_success | (elapsed_now >= max_episode_steps)                  # mycobot.py:398-400 | TimeLimit
    ep_return_out = ep_return + r.astype(np.float64)                             # Monitor: one float64 addition
    ep_length_out = ep_length + 1
    finished = terminated | truncated
    restart = finished & bool(auto_reset)
    return {
        "reward": r, "terminated": terminated, "truncated": truncated, "is_success": is_success, "distance": d,
        "ep_return_out": ep_return_out, "ep_length_out": ep_length_out.astype(np.int32), "finished": finished,
        "final_obs": obs, "final_achieved": A, "final_desired": G,
        "elapsed": np.where(restart, 0, elapsed_now).astype(np.int32),
        "ep_return": np.where(restart, 0.0, ep_return_out),
        "ep_length": np.where(restart, 0, ep_length_out).astype(np.int32),
        "episode": (episode + restart).astype(np.int32),
    }


def expected_by_table(codes, max_episode_steps=None) -> dict:
    """What the scenario table itself promises per code: is_success, terminated, truncated."""
    succ = np.array([SCENARIOS[int(c)][2][0] for c in codes])
    limit = np.array([SCENARIOS[int(c)][2][1] for c in codes])
    return {"is_success": succ, "terminated": succ.copy(), "truncated": succ | limit}


def dense_reward_ulps(reward, distance) -> np.ndarray:
    """|reward + d| in units of 2^-53 d (half ulps of a float64 of d's binade at most): the dense reward's bound is 4 of them."""
    d = np.asarray(distance, dtype=np.longdouble)
    return (np.abs(np.asarray(reward, dtype=np.float64).astype(np.longdouble) + d) / (np.longdouble(2.0) ** -53 * d)).astype(np.float64)
