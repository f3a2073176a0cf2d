"""The on-policy rollout buffer's rule, restated (test infrastructure; numpy scalars and Python integers only).

Nothing here is shared with csrc/ or with mycobotgym_amd/rollout.py, and the data structure is another one on purpose: the kernels keep
time-major ``[T, N]`` records and planes; this keeps, per environment, a Python list of the transitions of the rollout in flight, each a
dict, and runs every recursion per environment over that list.

Insertion (include/mcg.h: mcg_rollout_start / mcg_rollout_add).  A transition is (the observation and goals the action was taken
from, whether that observation starts an episode, action, log-probability, value, reward).  Observations and goals are float32
(numpy's cast of the engine's float64: round to nearest even).  The reward is SB3's bootstrap as recalled (on_policy_algorithm.py,
collect_rollouts): float32(reward), plus float32(gamma) * final_value -- product rounded, then the sum rounded -- where the time limit
alone ended the episode (truncated and not terminated) and final values are given.  The next transition starts from the step's obs /
achieved_goal / desired_goal, and starts an episode iff truncated or terminated.

Advantages (mcg_rollout_gae; SB3's compute_returns_and_advantage as recalled), np.float32 scalars, one rounding per operation:
g = float32(gamma), c = float32(gamma * gae_lambda) (the product in float64), last = 0; backwards over the list, with `nxt` the
transition after (or the state to continue from, and the caller's last value, at the end of the list):
    nnt = 1 - float32(nxt starts an episode);  delta = (reward + (g * nxt value) * nnt) - value;  last = delta + (c * nnt) * last;
    advantage = last;  returns = last + value.

Minibatches (mcg_rollout_gather).  The M = T N transitions are numbered i = env * T + step.  Sample k of an epoch is transition
walk(k): a 4-round balanced Feistel network on b bits (b the smallest even number >= 2 with 2^b >= M, h = b / 2), applied until the
value is below M.  A round maps (L, R) to (R, L ^ (w0 & (2^h - 1))), w0 the first word of Philox4x32-10 with counter
(R, epoch low word, round, 4 ^ (epoch high word << 8)) and key = seed.
"""
from __future__ import annotations

import numpy as np

MASK = 0xFFFFFFFF
STREAM = 4
ROUNDS = 4
PERM_SEED = 11          # the seed the tests' buffers use; tests/test_rollout_cpu.py settles its walk lengths without a GPU
f32 = np.float32


def philox_word0(ctr, key) -> int:
    """Philox4x32-10 (Salmon et al. 2011: multipliers 0xD2511F53 / 0xCD9E8D57, Weyl key steps 0x9E3779B9 / 0xBB67AE85); -> word 0."""
    c0, c1, c2, c3 = (int(x) & MASK for x in ctr)
    k0, k1 = (int(x) & MASK for x in key)
    for _ in range(10):
        hi0, lo0 = divmod(0xD2511F53 * c0, 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c2, 1 << 32)
        c0, c1, c2, c3 = hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0
        k0, k1 = (k0 + 0x9E3779B9) & MASK, (k1 + 0xBB67AE85) & MASK
    return c0


def feistel_bits(M: int) -> int:
    b = 2
    while (1 << b) < M:
        b += 2
    return b


def walk(seed: int, epoch: int, k: int, M: int):
    """-> (transition index of sample k, passes through the network it took)."""
    seed &= 2 ** 64 - 1
    epoch &= 2 ** 64 - 1
    h = feistel_bits(M) // 2
    low = (1 << h) - 1
    key = [seed & MASK, seed >> 32]
    x, passes = k, 0
    while True:
        L, R = x >> h, x & low
        for r in range(ROUNDS):
            w0 = philox_word0([R, epoch & MASK, r, (STREAM ^ ((epoch >> 32) << 8)) & MASK], key)
            L, R = R, L ^ (w0 & low)
        x = (L << h) | R
        passes += 1
        if x < M:
            return x, passes


def record_dtype(D: int, A: int) -> np.dtype:
    """A record as include/mcg.h lays it out: float32 obs, achieved, desired, action, log_prob, zeros to a multiple of 16 bytes."""
    fields = [("obs", "<f4", (D,)), ("achieved", "<f4", (3,)), ("desired", "<f4", (3,)), ("action", "<f4", (A,)), ("log_prob", "<f4")]
    used = 4 * (D + 3 + 3 + A + 1)
    total = -(-used // 16) * 16
    return np.dtype(fields + [("pad", "u1", (total - used,))])


def to32(x):
    return np.asarray(x, dtype=np.float64).astype(np.float32)


class Rollout:
    def __init__(self, N: int, D: int, A: int, T: int, gamma: float, gae_lambda: float):
        self.N, self.D, self.A, self.T = N, D, A, T
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.steps = [[] for _ in range(N)]             # per environment: the transitions of the rollout in flight
        self.cont = [None] * N                          # per environment: what the next transition starts from (a dict)
        self.done = False                               # finish() has run

    # ---------------------------------------------------------------------------------------------------- insertion
    def start(self, obs, achieved, desired, mask=None):
        for e in range(self.N):
            if mask is not None and not mask[e]:
                continue
            self.cont[e] = {"obs": to32(obs[e]), "achieved": to32(achieved[e]), "desired": to32(desired[e]), "start": True}

    def add(self, actions, values, log_probs, out: dict, final_values=None):
        """``out``: numpy arrays under mcg_step_out's names (obs, achieved_goal, desired_goal, reward, terminated, truncated)."""
        g = f32(self.gamma)
        with np.errstate(all="ignore"):
            for e in range(self.N):
                assert len(self.steps[e]) < self.T
                term, trunc = bool(out["terminated"][e]), bool(out["truncated"][e])
                r = f32(np.float64(out["reward"][e]))
                if final_values is not None and trunc and not term:
                    boot = f32(g * f32(final_values[e]))
                    r = f32(r + boot)
                c = self.cont[e]
                self.steps[e].append({"obs": c["obs"], "achieved": c["achieved"], "desired": c["desired"], "start": c["start"],
                                      "action": np.asarray(actions[e], dtype=np.float32), "log_prob": f32(log_probs[e]),
                                      "value": f32(values[e]), "reward": r})
                self.cont[e] = {"obs": to32(out["obs"][e]), "achieved": to32(out["achieved_goal"][e]),
                                "desired": to32(out["desired_goal"][e]), "start": term or trunc}

    # --------------------------------------------------------------------------------------------------- advantages
    def finish(self, last_values):
        g, c = f32(self.gamma), f32(self.gamma * self.gae_lambda)
        one = f32(1.0)
        with np.errstate(all="ignore"):
            for e in range(self.N):
                assert len(self.steps[e]) == self.T
                last = f32(0.0)
                nxt_value, nxt_start = f32(last_values[e]), self.cont[e]["start"]
                for tr in reversed(self.steps[e]):
                    nnt = f32(one - f32(1.0 if nxt_start else 0.0))
                    boot = f32(f32(g * nxt_value) * nnt)
                    delta = f32(f32(tr["reward"] + boot) - tr["value"])
                    last = f32(delta + f32(f32(c * nnt) * last))
                    tr["advantage"], tr["returns"] = last, f32(last + tr["value"])
                    nxt_value, nxt_start = tr["value"], tr["start"]
        self.done = True

    def reset(self):
        self.steps = [[] for _ in range(self.N)]
        self.done = False

    # ------------------------------------------------------------------------------------------------ what is stored
    def records(self) -> np.ndarray:
        """The record array [T, N] as the device must hold it (rows of steps not yet added: zero)."""
        R = np.zeros((self.T, self.N), dtype=record_dtype(self.D, self.A))
        for e in range(self.N):
            for t, tr in enumerate(self.steps[e]):
                for k in ("obs", "achieved", "desired", "action", "log_prob"):
                    R[t, e][k] = tr[k]
        return R

    def planes(self) -> dict:
        names = [("reward", np.float32), ("value", np.float32), ("episode_start", np.uint8)]
        if self.done:
            names += [("advantage", np.float32), ("returns", np.float32)]
        P = {k: np.zeros((self.T, self.N), dtype=dt) for k, dt in names}
        for e in range(self.N):
            for t, tr in enumerate(self.steps[e]):
                for k, _ in names:
                    P[k][t, e] = tr["start" if k == "episode_start" else k]
        return P

    def carried(self) -> dict:
        """last_obs [N, D], last_goals [N, 6], last_start [N] as the device must hold them."""
        return {"last_obs": np.stack([c["obs"] for c in self.cont]),
                "last_goals": np.stack([np.concatenate([c["achieved"], c["desired"]]) for c in self.cont]),
                "last_start": np.array([c["start"] for c in self.cont], dtype=np.uint8)}

    # --------------------------------------------------------------------------------------------------- minibatches
    def gather(self, seed: int, epoch: int, first: int, count: int) -> dict:
        """-> samples first .. first + count - 1 of the epoch as float32 arrays under mcg_rollout_batch's names, ``index`` int32 [B],
        ``passes`` [B]: the walk length of every sample."""
        assert self.done
        D, A, T, M = self.D, self.A, self.T, self.T * self.N
        o = {"obs": np.zeros((count, D), np.float32), "achieved": np.zeros((count, 3), np.float32), "desired": np.zeros((count, 3), np.float32),
             "action": np.zeros((count, A), np.float32), "old_value": np.zeros(count, np.float32), "old_log_prob": np.zeros(count, np.float32),
             "advantage": np.zeros(count, np.float32), "returns": np.zeros(count, np.float32), "index": np.zeros(count, np.int32),
             "passes": np.zeros(count, np.int64)}
        for j in range(count):
            i, o["passes"][j] = walk(seed, epoch, first + j, M)
            tr = self.steps[i // T][i % T]
            o["index"][j] = i
            for name, key in (("obs", "obs"), ("achieved", "achieved"), ("desired", "desired"), ("action", "action"), ("old_value", "value"),
                              ("old_log_prob", "log_prob"), ("advantage", "advantage"), ("returns", "returns")):
                o[name][j] = tr[key]
        return o
