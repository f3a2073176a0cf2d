"""Stacked gathers from the picture rollout buffer, restated (test infrastructure; numpy and Python integers only).  Nothing here is
shared with csrc/ or with the package.

The specification is wide storage, on the grounds tests/indep_frame_stack.py gives for the replay buffer: ``WideStackedRollout`` is the
existing tests/indep_rollout_img.ImageRollout with k * C channels, fed the stacks of the act-time rule
(tests/indep_frame_stack.StackRule; a masked restart is ``StackRule.reset(img, mask)``).  A sampled transition then simply carries the
stack its action was taken from.  That rule has no limit of 8 channels.

``FrameRollout`` is a third view, the rule as include/mcg.h states it for single-frame storage, in yet another data structure: an
ImageRollout of C channels for the slots and the planes, and per environment a Python list of the k - 1 (picture, flag) pairs from
before slot 0.

    Row t of environment e is the first picture of its episode iff its flag is 1: episode_start[t, e] for t < pos, last_start[e] for
    row pos, the kept pair's flag for t < 0.
    stack(t): slot k - 1 - i holds the picture of row t - i for i = 0, 1, ... up to and including the first row whose flag is 1, at
    most k - 1 steps back; the older slots are zeros.
    reset: the pairs become the last k - 1 of (the old pairs, then rows 0 .. pos - 1); then ImageRollout's reset.
"""
from __future__ import annotations

import numpy as np

from tests.indep_frame_stack import StackRule
from tests.indep_rollout_img import ImageRollout


class WideStackedRollout:
    """ImageRollout of k * C channels fed the act-time rule's stacks; its own calls take single frames.  ``depths[e][t]``: the frames
    of the running episode in the stack of slot t (what the act-time rule counted when it built that stack)."""

    def __init__(self, N: int, C: int, S: int, A: int, T: int, gamma: float, gae_lambda: float, k: int):
        self.N, self.C, self.S, self.A, self.T, self.k = N, C, S, A, T, k
        self.wide = ImageRollout(N, k * C, S, A, T, gamma, gae_lambda)
        self.rule = StackRule(N, C, S, k)
        self.depths = [[0] * (T + 1) for _ in range(N)]

    @property
    def pos(self):
        return self.wide.pos

    def _note(self, slot):
        for e in range(self.N):
            self.depths[e][slot] = int(self.rule.depth[e])

    def start(self, img, mask=None):
        self.wide.start(self.rule.reset(img, mask), mask)
        self._note(self.wide.pos)

    def add(self, actions, values, log_probs, img, reward, terminated, truncated, final_values=None):
        done = np.asarray(terminated, bool) | np.asarray(truncated, bool)
        stack, _ = self.rule.step(img, img, done)            # (the stacked final observation is not stored by a rollout buffer)
        self.wide.add(actions, values, log_probs, stack, reward, terminated, truncated, final_values=final_values)
        self._note(self.wide.pos)

    def finish(self, last_values):
        self.wide.finish(last_values)

    def reset(self):
        for e in range(self.N):
            self.depths[e][0] = self.depths[e][self.wide.pos]
        self.wide.reset()

    def planes(self):
        return self.wide.planes()

    def last_start(self):
        return self.wide.last_start()

    def frames(self) -> np.ndarray:
        """uint8 [T + 1, N, C, S, S]: the newest frame of every stored stack -- what single-frame storage must hold in its rows."""
        Pu = self.k * self.C * self.S * self.S
        px = self.wide.pixels()[:, :, :Pu].reshape(self.T + 1, self.N, self.k * self.C, self.S, self.S)
        return px[:, :, (self.k - 1) * self.C:]

    def gather(self, seed: int, epoch: int, first: int, count: int) -> dict:
        """ImageRollout.gather's batch (pictures [B, k * C, S, S]) with ``depth`` [B]."""
        o = self.wide.gather(seed, epoch, first, count)
        o["depth"] = np.array([self.depths[i // self.T][i % self.T] for i in o["index"].tolist()], np.int64)
        return o


class FrameRollout:
    """The rule for single-frame storage: the stacks are rebuilt when they are asked for."""

    def __init__(self, N: int, C: int, S: int, A: int, T: int, gamma: float, gae_lambda: float, k: int):
        self.N, self.C, self.S, self.A, self.T, self.k = N, C, S, A, T, k
        self.single = ImageRollout(N, C, S, A, T, gamma, gae_lambda)
        zero = bytes(self.single.P)
        self.before = [[(zero, 0)] * (k - 1) for _ in range(N)]          # per environment: rows -(k - 1) .. -1, the oldest first

    @property
    def pos(self):
        return self.single.pos

    def start(self, img, mask=None):
        self.single.start(img, mask)

    def add(self, actions, values, log_probs, img, reward, terminated, truncated, final_values=None):
        self.single.add(actions, values, log_probs, img, reward, terminated, truncated, final_values=final_values)

    def finish(self, last_values):
        self.single.finish(last_values)

    def row(self, e: int, t: int):
        """-> (the picture's P bytes, its flag) of row t, -(k - 1) <= t <= pos."""
        if t < 0:
            return self.before[e][self.k - 1 + t]
        pos = self.single.pos
        assert t <= pos
        flag = int(self.single.R.cont[e]["start"]) if t == pos else int(self.single.R.steps[e][t]["start"])
        return self.single.slots[e][t], flag

    def reset(self):
        if self.k > 1:
            for e in range(self.N):
                rows = self.before[e] + [self.row(e, t) for t in range(self.single.pos)]
                self.before[e] = rows[len(rows) - (self.k - 1):]
        self.single.reset()

    def stack(self, e: int, t: int) -> np.ndarray:
        """uint8 [k * C, S, S]; and the number of frames in it through ``depth``."""
        C, S, k = self.C, self.S, self.k
        out = np.zeros((k * C, S, S), np.uint8)
        for i in range(k):
            px, flag = self.row(e, t - i)
            out[(k - 1 - i) * C:(k - i) * C] = np.frombuffer(px, np.uint8)[:C * S * S].reshape(C, S, S)
            if flag:
                break
        return out

    def depth(self, e: int, t: int) -> int:
        for i in range(self.k):
            if self.row(e, t - i)[1]:
                return i + 1
        return self.k

    def pixels(self) -> np.ndarray:
        return self.single.pixels()

    def history(self) -> np.ndarray:
        """uint8 [k - 1, N, P] as the device must hold its history rows, padding included."""
        P = self.single.P
        return np.array([[np.frombuffer(self.before[e][r][0], np.uint8) for e in range(self.N)] for r in range(self.k - 1)],
                        dtype=np.uint8).reshape(self.k - 1, self.N, P)

    def history_start(self) -> np.ndarray:
        return np.array([[self.before[e][r][1] for e in range(self.N)] for r in range(self.k - 1)], dtype=np.uint8).reshape(self.k - 1, self.N)

    def planes(self):
        return self.single.planes()

    def last_start(self):
        return self.single.last_start()

    def gather(self, seed: int, epoch: int, first: int, count: int) -> dict:
        o = self.single.gather(seed, epoch, first, count)
        idx = o["index"].tolist()
        o["pix"] = np.array([self.stack(i // self.T, i % self.T) for i in idx], np.uint8).reshape(count, self.k * self.C, self.S, self.S)
        o["pix_f32"] = o["pix"].astype(np.float32) / np.float32(255)
        o["depth"] = np.array([self.depth(i // self.T, i % self.T) for i in idx], np.int64)
        return o
