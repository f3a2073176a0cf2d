"""Frame stacking for the pictures, restated (test infrastructure; numpy and Python integers only).  Nothing here is shared with csrc/
or with the package.

The act-time rule is SB3's channels-first ``StackedObservations.update``: a stack [k * C, S, S] whose slot s is channels
s * C .. s * C + C - 1, slot k - 1 the newest.  A step shifts the stack down one slot and puts the step's picture in the newest slot;
where the episode ended (done = terminated | truncated) the older slots become zeros, and the stacked final observation is the old
stack shifted down one slot with the finished episode's last picture in the newest slot.  A reset zeroes the older slots of the reset
environments and puts the reset's picture in the newest.

The stacked replay rule is deliberately another data structure than the kernels': they keep single frames in a ring of K + k rows and
rebuild a stack from the k rows that end at a sample; this feeds the stacks of the act-time rule, whole, into the existing
tests/indep_replay_img.ImageReplay with k * C channels and capacity K -- storage k times as wide, in which a sampled transition simply
carries its stack and its next stack (for a time-limit end: the stacked final observation).  Wide storage is the specification.

One thing is taken over from the kernels' layout, because the caller can observe it (as ImageReplay takes over the places of the final
pictures): the ring the caller allocates has capacity K + k - 1, so its final pictures have F = ceil((K + k - 1) / Tm) + 1 places.
A row index is compared through the absolute time: the rule's row is a % (K + 1), the kernels' a % (K + k).
"""
from __future__ import annotations

import math

import numpy as np

from tests.indep_replay_img import MAX_DRAWS, ImageReplay, pair


class StackRule:
    """SB3's StackedObservations on [N, k * C, S, S] uint8, and per environment the depth of its stack: the frames in it that belong
    to the running episode."""

    def __init__(self, N: int, C: int, S: int, k: int):
        self.N, self.C, self.S, self.k = N, C, S, k
        self.stack = np.zeros((N, k * C, S, S), np.uint8)
        self.depth = np.zeros(N, int)

    def reset(self, img, mask=None):
        for e in range(self.N):
            if mask is not None and not mask[e]:
                continue
            self.stack[e] = 0
            self.stack[e, (self.k - 1) * self.C:] = img[e]
            self.depth[e] = 1
        return self.stack.copy()

    def step(self, img, final_img, done):
        """-> (stack, final_stack), both for every environment."""
        C = self.C
        final = np.concatenate([self.stack[:, C:], np.asarray(final_img, np.uint8)], axis=1)
        new = np.concatenate([self.stack[:, C:], np.asarray(img, np.uint8)], axis=1)
        for e in range(self.N):
            if done[e]:
                new[e, :(self.k - 1) * C] = 0
                self.depth[e] = 1
            else:
                self.depth[e] = min(self.depth[e] + 1, self.k)
        self.stack = new
        return new.copy(), final


class StackedReplay:
    """ImageReplay of k * C channels fed the act-time rule's stacks; its own calls take single frames, as the device buffer's may."""

    def __init__(self, N: int, C: int, S: int, A: int, K: int, Tm: int, k: int):
        self.N, self.C, self.S, self.A, self.K, self.Tm, self.k = N, C, S, A, K, Tm, k
        self.wide = ImageReplay(N, k * C, S, A, K, Tm)
        self.wide.F = -(-(K + k - 1) // Tm) + 1          # the places of the final pictures in the ring the caller allocates
        self.rule = StackRule(N, C, S, k)
        self.depths = [[] for _ in range(N)]              # per environment and transition: the depth of the stack it was taken from

    @property
    def n(self):
        return self.wide.n

    def start(self, img, mask=None):
        self.wide.start(self.rule.reset(img, mask), mask)

    def add(self, actions, img, final_img, reward, terminated, truncated):
        for e in range(self.N):
            self.depths[e].append(int(self.rule.depth[e]))
        stack, final = self.rule.step(img, final_img, np.asarray(terminated, bool) | np.asarray(truncated, bool))
        self.wide.add(actions, stack, final, reward, terminated, truncated)

    def sample(self, seed: int, call: int, batch: int) -> dict:
        """ImageReplay.sample's batch (pictures [B, k * C, S, S]) with ``row``: the kernels' row (a % (K + k); -1 where the sample gave
        up), the absolute time taken again from the draw itself, and ``depth``: the frames of the sampled stack (0 where it gave up)."""
        o = self.wide.sample(seed, call, batch)
        n, W = self.wide.n, min(self.wide.n, self.K)
        o["row"], o["depth"] = np.full(batch, -1, np.int64), np.zeros(batch, np.int64)
        for i in range(batch):
            if o["draws"][i] > MAX_DRAWS:
                continue
            u0, _ = pair(seed, call, i, int(o["draws"][i]) - 1)
            a = n - W + min(W - 1, int(math.floor(u0 * W)))
            assert a == o["time"][i] and o["index"][i, 0] == a % (self.K + 1)
            o["row"][i] = a % (self.K + self.k)
            o["depth"][i] = self.depths[int(o["index"][i, 1])][a]
        return o
