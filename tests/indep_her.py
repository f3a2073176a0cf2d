"""The hindsight replay buffer's rule, restated (test infrastructure; numpy and Python integers only).

Nothing here is shared with csrc/ or with mycobotgym_amd/replay.py, and the data structure is another one on purpose: the kernel keeps a
ring of records with ``t_in_ep`` / ``ep_len`` fields and back-fills lengths; this keeps, per environment, a Python list of whole
episodes, each a list of transitions stamped with the absolute time (the insertion count) they were added at.  Whether a transition
may be sampled is decided from those times alone: its episode has ended with a done flag, and the episode's first transition is still
inside the last ``capacity`` insertions.

Insertion (include/mcg.h: mcg_her_start / mcg_her_add).  A transition is (last observation, action, next observation, reward,
terminated).  done = truncated | terminated; where done, the step's obs / achieved_goal / desired_goal already belong to the next
episode, so the transition's next observation and its desired goal are the step's final_* there; the next transition starts from the
step's obs / achieved_goal either way.  Observations, actions and rewards are kept as float32 (numpy's cast: round to nearest even),
goals as float64.  ``start`` abandons the episode in flight; an episode that gets ``max_steps`` transitions and no done flag is
abandoned and counted.

Sampling (mcg_her_sample).  Philox4x32-10 (tests/indep_scene_rand.py) with counter (k, call low word, draw, 3 ^ (call high word << 8)),
key = seed; a draw yields (u0, u1), the two 64-bit halves' top 53 bits times 2^-53.  W = min(n, capacity).  Draw d = 0, 1, ... of sample
k: slot s = min(W - 1, floor(u0 W)), environment e = min(N - 1, floor(u1 N)); the slot holds absolute time n - 1 - ((pos - 1 - s) mod
capacity), pos = n mod capacity.  The first valid (s, e) is taken; after 256 invalid draws the sample gives up (index -1, zeros).
Samples k >= batch - n_virtual are relabelled: draw 256 gives the future step f = min(len - 1, t + floor(u0 (len - t))) of the
episode, the new goal is that transition's next achieved goal, the reward -(d > threshold) (sparse) or -d (dense),
d = sqrt(dx dx + dy dy + dz dz) in float64 on (next achieved goal, new goal), cast to float32.
"""
from __future__ import annotations

import math

import numpy as np

from tests.indep_scene_rand import philox4x32_10

MASK = 0xFFFFFFFF
STREAM = 3
MAX_DRAWS = 256


def pair(seed: int, call: int, k: int, draw: int):
    seed &= 2 ** 64 - 1
    call &= 2 ** 64 - 1
    r = philox4x32_10([k & MASK, call & MASK, draw, (STREAM ^ ((call >> 32) << 8)) & MASK], [seed & MASK, seed >> 32])
    return (((r[0] << 32) | r[1]) >> 11) * 2.0 ** -53, (((r[2] << 32) | r[3]) >> 11) * 2.0 ** -53


def record_dtype(D: int, A: int) -> np.dtype:
    """A record as include/mcg.h lays it out: nine float64 goals, the float32 block, two int32, the flag, zeros to a multiple of 16."""
    fields = [("achieved", "<f8", (3,)), ("next_achieved", "<f8", (3,)), ("desired", "<f8", (3,)),
              ("obs", "<f4", (D,)), ("next_obs", "<f4", (D,)), ("action", "<f4", (A,)), ("reward", "<f4"),
              ("t_in_ep", "<i4"), ("ep_len", "<i4"), ("terminated", "u1")]
    used = 72 + 4 * (2 * D + A + 1) + 4 + 4 + 1
    total = -(-used // 16) * 16
    return np.dtype(fields + [("pad", "u1", (total - used,))])


class Episode:
    def __init__(self):
        self.steps = []          # transitions: dicts with their absolute time
        self.ended = False       # a done flag closed it
        self.abandoned = False   # start() cut it, or it ran to max_steps transitions without a done flag

    @property
    def complete(self):
        return self.ended and not self.abandoned


class History:
    def __init__(self, N: int, D: int, A: int, capacity: int, max_steps: int, reward_type: str = "dense", threshold: float = 0.05):
        assert capacity >= 2 * max_steps and reward_type in ("dense", "sparse")
        self.N, self.D, self.A, self.capacity, self.max_steps = N, D, A, capacity, max_steps
        self.reward_type, self.threshold = reward_type, float(threshold)
        self.n = 0                                      # insertions so far
        self.episodes = [[Episode()] for _ in range(N)]
        self.last = [None] * N                          # (float32 observation, float64 achieved goal) the next transition starts from
        self.overlong = 0

    # ---------------------------------------------------------------------------------------------------- insertion
    def start(self, obs, achieved, mask=None):
        for e in range(self.N):
            if mask is not None and not mask[e]:
                continue
            cur = self.episodes[e][-1]
            if cur.steps:
                cur.abandoned = True
                self.episodes[e].append(Episode())
            self.last[e] = (np.asarray(obs[e], dtype=np.float64).astype(np.float32), np.array(achieved[e], dtype=np.float64))

    def add(self, actions, out: dict):
        """``out``: numpy arrays under mcg_step_out's names (obs, achieved_goal, desired_goal, reward, terminated, truncated, final_*)."""
        for e in range(self.N):
            done = bool(out["truncated"][e]) or bool(out["terminated"][e])
            pre = "final_" if done else ""
            nxt = {"obs": out["final_obs"][e] if done else out["obs"][e],
                   "achieved": out[pre + "achieved"][e] if done else out["achieved_goal"][e],
                   "desired": out[pre + "desired"][e] if done else out["desired_goal"][e]}
            cur = self.episodes[e][-1]
            cur.steps.append({"time": self.n, "obs": self.last[e][0], "achieved": self.last[e][1],
                              "next_obs": np.asarray(nxt["obs"], dtype=np.float64).astype(np.float32),
                              "next_achieved": np.array(nxt["achieved"], dtype=np.float64),
                              "desired": np.array(nxt["desired"], dtype=np.float64),
                              "action": np.asarray(actions[e], dtype=np.float32),
                              "reward": np.float32(np.float64(out["reward"][e])), "terminated": bool(out["terminated"][e])})
            if done:
                cur.ended = True
                self.episodes[e].append(Episode())
            elif len(cur.steps) == self.max_steps and not cur.abandoned:
                cur.abandoned = True
                self.overlong += 1
            self.last[e] = (np.asarray(out["obs"][e], dtype=np.float64).astype(np.float32), np.array(out["achieved_goal"][e], dtype=np.float64))
        self.n += 1

    # ------------------------------------------------------------------------------------------------- what is stored
    def oldest(self) -> int:
        return max(0, self.n - self.capacity)

    def find(self, e: int, time: int):
        """-> (episode, index of the transition added at ``time``) of environment e."""
        for ep in self.episodes[e]:
            if ep.steps and ep.steps[0]["time"] <= time <= ep.steps[-1]["time"]:
                return ep, time - ep.steps[0]["time"]
        raise KeyError((e, time))

    def valid(self, e: int, time: int) -> bool:
        if not self.oldest() <= time < self.n:
            return False
        ep, _ = self.find(e, time)
        return ep.complete and ep.steps[0]["time"] >= self.oldest()

    def valid_pairs(self):
        """The set of (slot, env) that may be sampled now."""
        return {(t % self.capacity, e) for e in range(self.N) for t in range(self.oldest(), self.n) if self.valid(e, t)}

    def ring(self) -> np.ndarray:
        """The record array [capacity, N] as the device must hold it: slot time % capacity holds the newest transition added there."""
        R = np.zeros((self.capacity, self.N), dtype=record_dtype(self.D, self.A))
        for e in range(self.N):
            for ep in self.episodes[e]:
                for i, tr in enumerate(ep.steps):
                    if tr["time"] < self.oldest():
                        continue
                    r = R[tr["time"] % self.capacity, e]
                    for k in ("achieved", "next_achieved", "desired", "obs", "next_obs", "action", "reward"):
                        r[k] = tr[k]
                    r["terminated"] = tr["terminated"]
                    r["t_in_ep"] = min(i, self.max_steps)
                    r["ep_len"] = len(ep.steps) if ep.complete else 0
        return R

    # ------------------------------------------------------------------------------------------------------ sampling
    def reward(self, achieved, goal) -> np.float32:
        dx, dy, dz = (float(achieved[k]) - float(goal[k]) for k in range(3))
        d = math.sqrt(dx * dx + dy * dy + dz * dz)
        return np.float32(-float(np.float32(d > self.threshold))) if self.reward_type == "sparse" else np.float32(-d)

    def sample(self, seed: int, call: int, batch: int, n_virtual: int) -> dict:
        """-> the batch as float32 arrays under mcg_her_batch's names, ``index`` int32 [B, 3], ``draws`` [B]: rejection draws used
        (MAX_DRAWS + 1 where the sample gave up), ``future`` [B]: the future step's index in its episode (-1: a real sample)."""
        D, A, cap, N = self.D, self.A, self.capacity, self.N
        W, pos = min(self.n, cap), self.n % cap
        o = {"obs": np.zeros((batch, D), np.float32), "achieved": np.zeros((batch, 3), np.float32), "desired": np.zeros((batch, 3), np.float32),
             "next_obs": np.zeros((batch, D), np.float32), "next_achieved": np.zeros((batch, 3), np.float32),
             "action": np.zeros((batch, A), np.float32), "reward": np.zeros(batch, np.float32), "done": np.zeros(batch, np.float32),
             "index": np.full((batch, 3), -1, np.int32), "draws": np.zeros(batch, np.int64), "future": np.full(batch, -1, np.int64),
             "step": np.full(batch, -1, np.int64), "length": np.zeros(batch, np.int64),
             "goal64": np.zeros((batch, 3)), "next_achieved64": np.zeros((batch, 3))}
        for k in range(batch):
            hit = None
            for d in range(MAX_DRAWS if W > 0 else 0):
                u0, u1 = pair(seed, call, k, d)
                s, e = min(W - 1, int(math.floor(u0 * W))), min(N - 1, int(math.floor(u1 * N)))
                time = self.n - 1 - ((pos - 1 - s) % cap)
                if self.valid(e, time):
                    hit = (s, e, time, d + 1)
                    break
            if hit is None:
                o["draws"][k] = MAX_DRAWS + 1
                continue
            s, e, time, o["draws"][k] = hit
            ep, t = self.find(e, time)
            tr = ep.steps[t]
            goal, reward, fslot = tr["desired"], tr["reward"], -1
            if k >= batch - n_virtual:
                u0, _ = pair(seed, call, k, MAX_DRAWS)
                L = len(ep.steps)
                f = min(L - 1, t + int(math.floor(u0 * (L - t))))
                goal = ep.steps[f]["next_achieved"]
                fslot = ep.steps[f]["time"] % cap
                reward = self.reward(tr["next_achieved"], goal)
                o["future"][k] = f
            o["step"][k], o["length"][k] = t, len(ep.steps)
            o["index"][k] = (s, e, fslot)
            o["obs"][k], o["next_obs"][k], o["action"][k] = tr["obs"], tr["next_obs"], tr["action"]
            o["achieved"][k], o["next_achieved"][k], o["desired"][k] = tr["achieved"], tr["next_achieved"], goal
            o["reward"][k], o["done"][k] = reward, float(tr["terminated"])
            o["goal64"][k], o["next_achieved64"][k] = goal, tr["next_achieved"]
        return o
