"""The picture replay buffer's rule, restated (test infrastructure; numpy and Python integers only).

Nothing here is shared with csrc/ or with mycobotgym_amd/replay_img.py, and the data structure is another one on purpose: the kernels
keep a ring of K + 1 rows in which the next picture of a slot is the following row; this keeps, per environment, a Python list of
every transition ever added, each holding its own ``bytes`` pictures, and the picture the environment continues from.  Which picture
follows a transition is read off the list, not off a row.

Insertion (include/mcg.h: mcg_replay_img_start / mcg_replay_img_add).  Transition a of environment e is (the picture e continued from,
action, float32 reward, terminated, timeout = truncated & !terminated, and where timeout the step's final picture).  ``start`` replaces
the picture an environment continues from; if its newest transition ended no episode, that transition has lost its successor
(``no_next``) and is never sampled.  The successor of transition a is the picture transition a + 1 was taken from, or, for the newest,
the picture the environment continues from: after an episode's end that is the next episode's first picture.

The final pictures live in F = ceil(K / Tm) + 1 places per environment, a timeout at time a in place (a // Tm) % F: a later timeout of
the same environment in the same place destroys it.  That is the one thing taken over from the layout, because it is what the caller
can observe: a sampled timeout whose final picture was destroyed comes out as terminal (done = 1, the ring's successor), and is counted.

Sampling (mcg_replay_img_sample).  Philox4x32-10 through tests/indep_her.py's construction on stream 5: counter (k, call low word, draw,
5 ^ (call high word << 8)), key = seed.  W = min(n, K).  Draw d = 0, 1, ... of sample k: j = min(W - 1, floor(u0 W)), a = n - W + j,
e = min(N - 1, floor(u1 N)); the first draw without ``no_next`` is taken; after 256 the sample gives up (index -1, zeros).
"""
from __future__ import annotations

import math

import numpy as np

from tests.indep_scene_rand import philox4x32_10

MASK = 0xFFFFFFFF
STREAM = 5
MAX_DRAWS = 256
TERMINATED, TIMEOUT, NO_NEXT = 1, 2, 4


def pair(seed: int, call: int, k: int, draw: int):
    seed &= 2 ** 64 - 1
    call &= 2 ** 64 - 1
    r = philox4x32_10([k & MASK, call & MASK, draw, (STREAM ^ ((call >> 32) << 8)) & MASK], [seed & MASK, seed >> 32])
    return (((r[0] << 32) | r[1]) >> 11) * 2.0 ** -53, (((r[2] << 32) | r[3]) >> 11) * 2.0 ** -53


def record_dtype(A: int) -> np.dtype:
    """A record as include/mcg.h lays it out: the action, the reward, the flags, zeros to a multiple of 16."""
    used = 4 * A + 8
    return np.dtype([("action", "<f4", (A,)), ("reward", "<f4"), ("flags", "<u4"), ("pad", "u1", (-(-used // 16) * 16 - used,))])


class ImageReplay:
    def __init__(self, N: int, C: int, S: int, A: int, K: int, Tm: int):
        self.N, self.C, self.S, self.A, self.K, self.Tm = N, C, S, A, K, Tm
        self.Pu = C * S * S
        self.P = -(-self.Pu // 16) * 16
        self.F = -(-K // Tm) + 1
        self.n = 0                                   # insertions so far
        self.steps = [[] for _ in range(N)]          # per environment: every transition, index = its absolute time
        self.cur = [bytes(self.Pu)] * N              # the picture each environment continues from

    # ---------------------------------------------------------------------------------------------------- insertion
    def start(self, img, mask=None):
        for e in range(self.N):
            if mask is not None and not mask[e]:
                continue
            self.cur[e] = np.ascontiguousarray(img[e], dtype=np.uint8).tobytes()
            if self.steps[e] and not (self.steps[e][-1]["terminated"] or self.steps[e][-1]["timeout"]):
                self.steps[e][-1]["no_next"] = True

    def add(self, actions, img, final_img, reward, terminated, truncated):
        for e in range(self.N):
            term = bool(terminated[e])
            timeout = bool(truncated[e]) and not term
            self.steps[e].append({"pic": self.cur[e], "action": np.asarray(actions[e], dtype=np.float32).copy(),
                                  "reward": np.float32(np.float64(reward[e])), "terminated": term, "timeout": timeout, "no_next": False,
                                  "final": np.ascontiguousarray(final_img[e], dtype=np.uint8).tobytes() if timeout else None})
            self.cur[e] = np.ascontiguousarray(img[e], dtype=np.uint8).tobytes()
        self.n += 1

    # ------------------------------------------------------------------------------------------------- what is stored
    def successor(self, e: int, a: int) -> bytes:
        return self.steps[e][a + 1]["pic"] if a + 1 < self.n else self.cur[e]

    def final_alive(self, e: int, a: int) -> bool:
        """The final picture of the timeout at time a has not been destroyed by a later timeout in its place."""
        place = (a // self.Tm) % self.F
        return not any(tr["timeout"] and (b // self.Tm) % self.F == place for b, tr in enumerate(self.steps[e]) if b > a)

    def flags(self, e: int, a: int) -> int:
        tr = self.steps[e][a]
        return (TERMINATED if tr["terminated"] else 0) | (TIMEOUT if tr["timeout"] else 0) | (NO_NEXT if tr["no_next"] else 0)

    def _padded(self, pic: bytes) -> np.ndarray:
        row = np.zeros(self.P, np.uint8)
        row[:self.Pu] = np.frombuffer(pic, np.uint8)
        return row

    def arrays(self) -> dict:
        """pixels [K + 1, N, P], finals [F, N, P], final_time [F, N] and records [K + 1, N] as the device must hold them: the place
        time % (K + 1) holds the newest thing put there, places never written are zeros (final_time: -1)."""
        R = self.K + 1
        px = np.zeros((R, self.N, self.P), np.uint8)
        fin = np.zeros((self.F, self.N, self.P), np.uint8)
        ftime = np.full((self.F, self.N), -1, np.int64)
        rec = np.zeros((R, self.N), record_dtype(self.A))
        for e in range(self.N):
            for a in range(max(0, self.n - R + 1), self.n + 1):          # the R newest pictures: times n - K .. n
                px[a % R, e] = self._padded(self.steps[e][a]["pic"] if a < self.n else self.cur[e])
            for a in range(max(0, self.n - R), self.n):                  # the R newest records
                tr = self.steps[e][a]
                rec[a % R, e]["action"], rec[a % R, e]["reward"], rec[a % R, e]["flags"] = tr["action"], tr["reward"], self.flags(e, a)
            for a, tr in enumerate(self.steps[e]):                       # in order of time: the newest in a place stays
                if tr["timeout"]:
                    fin[(a // self.Tm) % self.F, e] = self._padded(tr["final"])
                    ftime[(a // self.Tm) % self.F, e] = a
        return {"pixels": px, "finals": fin, "final_time": ftime, "records": rec}

    # ------------------------------------------------------------------------------------------------------ sampling
    def sample(self, seed: int, call: int, batch: int) -> dict:
        """-> the batch under mcg_replay_img_batch's names (pictures [B, C, S, S]), ``index`` int32 [B, 3], ``draws`` [B]: the draws the
        sample took (MAX_DRAWS + 1 where it gave up), ``time`` [B], ``flags`` [B] and ``lost`` (timeouts whose final was destroyed)."""
        N, K, C, S = self.N, self.K, self.C, self.S
        W = min(self.n, K)
        assert W >= 1
        o = {"pix": np.zeros((batch, C, S, S), np.uint8), "next_pix": np.zeros((batch, C, S, S), np.uint8),
             "action": np.zeros((batch, self.A), np.float32), "reward": np.zeros((batch, 1), np.float32),
             "done": np.zeros((batch, 1), np.float32), "index": np.full((batch, 3), -1, np.int32), "draws": np.zeros(batch, np.int64),
             "time": np.full(batch, -1, np.int64), "flags": np.zeros(batch, np.int64), "lost": 0, "give_ups": 0}
        for k in range(batch):
            hit = None
            for d in range(MAX_DRAWS):
                u0, u1 = pair(seed, call, k, d)
                j, e = min(W - 1, int(math.floor(u0 * W))), min(N - 1, int(math.floor(u1 * N)))
                a = self.n - W + j
                if not self.steps[e][a]["no_next"]:
                    hit = (a, e, d + 1)
                    break
            if hit is None:
                o["draws"][k] = MAX_DRAWS + 1
                o["give_ups"] += 1
                continue
            a, e, o["draws"][k] = hit
            tr = self.steps[e][a]
            from_final = tr["timeout"] and self.final_alive(e, a)
            lost = tr["timeout"] and not from_final
            o["lost"] += int(lost)
            nxt = tr["final"] if from_final else self.successor(e, a)
            o["pix"][k] = np.frombuffer(tr["pic"], np.uint8).reshape(C, S, S)
            o["next_pix"][k] = np.frombuffer(nxt, np.uint8).reshape(C, S, S)
            o["action"][k], o["reward"][k, 0] = tr["action"], tr["reward"]
            o["done"][k, 0] = 1.0 if (tr["terminated"] or lost) else 0.0
            o["index"][k] = (a % (K + 1), e, int(from_final))
            o["time"][k], o["flags"][k] = a, self.flags(e, a)
        o["pix_f32"] = o["pix"].astype(np.float32) / np.float32(255)
        o["next_pix_f32"] = o["next_pix"].astype(np.float32) / np.float32(255)
        return o
