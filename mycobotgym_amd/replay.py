"""``HerBuffer`` -- a hindsight replay buffer whose storage, insertion and sampling live on the GPU.

What the reference trains its goal-conditioned ids with is SB3's ``HerReplayBuffer`` (``n_sampled_goal=4``, strategy ``future``, one
environment; scripts/train.py:89-97).  This is the same rule on the engine's N lockstep environments: a time-major ring
``[capacity, N]`` of transitions, one launch to insert a step (``mcg_her_add``), one to draw a relabelled batch (``mcg_her_sample``).

    buf = HerBuffer(envs, capacity=1000, n_sampled_goal=4, seed=0)
    obs, _ = envs.reset(seed=0);  buf.start(obs)
    out = envs.step(a);           buf.add(a, *out)
    batch = buf.sample(65536)

This file owns the device memory (PyTorch tensors) and three host integers; the C side keeps no state.  No call synchronises but
``sample(check=True)`` and ``counters()``.  No CPU or PyTorch fallback: the kernels are the only implementation.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import torch

from . import _abi
from ._devbuf import DeviceBuffer, _ptr

_REWARDS = {"sparse": _abi.REWARD_SPARSE, "dense": _abi.REWARD_DENSE, "reward_shaping": _abi.REWARD_SHAPING}

# SB3's DictReplayBufferSamples names, and `index` [B, 3]: slot, env, slot the new goal came from (-1 in a real sample)
HerSamples = namedtuple("HerSamples", ["observations", "actions", "next_observations", "dones", "rewards", "index"])


class HerBuffer(DeviceBuffer):
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"), ("max_episode_steps", "max_episode_steps"),
                  ("reward_type", "reward_type"), ("distance_threshold", "distance_threshold"))
    _NO_IMAGES = "the -v1 image ids carry no goals in their observation: hindsight relabelling has nothing to act on"
    _HOST_STATE = ("n_written", "n_sampled", "seed")

    def __init__(self, envs=None, capacity: int = 1000, n_sampled_goal: int = 4, seed: int = 0, *, num_envs: Optional[int] = None,
                 obs_dim: Optional[int] = None, act_dim: Optional[int] = None, max_episode_steps: Optional[int] = None,
                 reward_type: Optional[str] = None, distance_threshold: Optional[float] = None, device=None, guard_rows: int = 0):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions, reward type, threshold, time limit and device from; or give them
        by keyword.  ``capacity``: slots of the ring (transitions per environment), at least twice the time limit.
        ``guard_rows``: spare slots allocated before and after the ring, which no call may touch (``guards()``; tests)."""
        num_envs, obs_dim, act_dim, max_episode_steps, reward_type, distance_threshold = self._resolve(envs, device, dict(
            num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim, max_episode_steps=max_episode_steps, reward_type=reward_type,
            distance_threshold=distance_threshold))
        if reward_type not in _REWARDS:
            raise ValueError(f"unknown reward_type {reward_type!r}")
        if n_sampled_goal < 0:
            raise ValueError("n_sampled_goal must be >= 0")
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        self.capacity, self.max_episode_steps = int(capacity), int(max_episode_steps)
        self.reward_type, self.distance_threshold = reward_type, float(distance_threshold)
        self.n_sampled_goal = int(n_sampled_goal)
        self.her_ratio = 1.0 - 1.0 / (self.n_sampled_goal + 1)              # SB3: the share of relabelled samples
        self.seed = int(seed) & (2 ** 64 - 1)
        self.n_written = 0           # insertions so far: the ring's position is n_written % capacity
        self.n_sampled = 0           # sample() calls so far: the `call` word of the sampling draws
        self.record_bytes = int(self._lib.mcg_her_record_bytes(self.obs_dim, self.act_dim))
        self._guard = int(guard_rows)
        n, D, dev = self.num_envs, self.obs_dim, self.device
        if self.record_bytes > 0 and n > 0 and self.capacity > 0:
            self._alloc = torch.zeros(self.capacity + 2 * self._guard, n, self.record_bytes, dtype=torch.uint8, device=dev)
        else:                        # the C side refuses the shape with its own message at the first call
            self._alloc = torch.zeros(1, 1, 16, dtype=torch.uint8, device=dev)
        self._t = {"records": self._alloc[self._guard:self._guard + max(self.capacity, 0)],
                   "t_run": torch.zeros(max(n, 1), dtype=torch.int32, device=dev),
                   "last_obs": torch.zeros(max(n, 1), max(D, 1), dtype=torch.float32, device=dev),
                   "last_achieved": torch.zeros(max(n, 1), 3, dtype=torch.float64, device=dev),
                   "counters": torch.zeros(2, dtype=torch.int64, device=dev)}       # uint64 counts carried in an int64 tensor
        self._cbuf = _abi.McgHerBuf(**{k: v.data_ptr() for k, v in self._t.items()}, n_envs=self.num_envs, obs_dim=self.obs_dim,
                                    act_dim=self.act_dim, capacity=self.capacity, max_episode_steps=self.max_episode_steps,
                                    reward_type=_REWARDS[reward_type], distance_threshold=self.distance_threshold)

    # ----------------------------------------------------------------------------------------------------- insertion
    def start(self, obs, mask=None):
        """An episode starts from ``obs`` (what ``reset`` returned) in the environments of ``mask`` (None: all); an episode that was in
        flight there is abandoned and never sampled."""
        o, ag, _ = self._goal_obs(obs, "obs")
        m = None if mask is None else self._dev(mask, torch.uint8, (self.num_envs,), "mask")
        first = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr())
        self._call("mcg_her_start", C.byref(first), _ptr(m))

    def add(self, actions, obs, reward, terminated, truncated, info):
        """One transition per environment: ``buf.add(a, *envs.step(a))``.  Where an episode ended, the transition's next observation and
        goal are ``info["final_observation"]`` (``obs`` already belongs to the next episode there)."""
        a = self._dev(actions, torch.float32, (self.num_envs, self.act_dim), "actions")
        out, _alive = self._step_out(obs, reward, terminated, truncated, info["final_observation"])
        self._call("mcg_her_add", self.n_written, _ptr(a), C.byref(out))
        self.n_written += 1

    # ------------------------------------------------------------------------------------------------------ sampling
    def n_virtual(self, batch_size: int) -> int:
        """Relabelled samples of a batch, SB3's split: the last ``int(batch * (1 - 1 / (n_sampled_goal + 1)))``."""
        return int(batch_size * self.her_ratio)

    def sample(self, batch_size: int, check: bool = True) -> HerSamples:
        """A ``future``-strategy batch: float32 device tensors under SB3's ``DictReplayBufferSamples`` names, and ``index``.
        ``check=True`` reads the give-up counter (the one synchronising path) and raises if a sample found no valid transition in
        256 draws -- as when no episode has finished yet; ``check=False`` never synchronises: such a sample has index -1 and zeros."""
        B, D, A, dev = int(batch_size), self.obs_dim, self.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        rows = max(B, 1)
        t = {"obs": torch.empty(rows, D, **f32), "achieved": torch.empty(rows, 3, **f32), "desired": torch.empty(rows, 3, **f32),
             "next_obs": torch.empty(rows, D, **f32), "next_achieved": torch.empty(rows, 3, **f32), "action": torch.empty(rows, A, **f32),
             "reward": torch.empty(rows, 1, **f32), "done": torch.empty(rows, 1, **f32),
             "index": torch.empty(rows, 3, dtype=torch.int32, device=dev)}
        out = _abi.McgHerBatch(**{k: v.data_ptr() for k, v in t.items()})
        before = self.counters()["sample_give_ups"] if check else 0
        self._call("mcg_her_sample", self.n_written, C.c_uint64(self.seed), C.c_uint64(self.n_sampled), B, self.n_virtual(B), C.byref(out))
        self.n_sampled += 1
        if check:
            gave_up = self.counters()["sample_give_ups"] - before
            if gave_up:
                raise RuntimeError(f"HerBuffer.sample: {gave_up} of {B} samples found no valid transition in 256 draws "
                                   f"({self.n_written} insertions; does the buffer hold a finished episode?)")
        return HerSamples(
            observations={"observation": t["obs"], "achieved_goal": t["achieved"], "desired_goal": t["desired"]},
            actions=t["action"],
            next_observations={"observation": t["next_obs"], "achieved_goal": t["next_achieved"], "desired_goal": t["desired"]},
            dones=t["done"], rewards=t["reward"], index=t["index"])

    # --------------------------------------------------------------------------------------------- counters, storage
    def counters(self) -> dict:
        """``sample_give_ups``: samples that found no valid transition; ``overlong_episodes``: episodes that ran to ``max_episode_steps``
        transitions without a done flag and were abandoned.  Synchronises."""
        c = self._t["counters"].cpu().tolist()
        return {"sample_give_ups": c[0] & (2 ** 64 - 1), "overlong_episodes": c[1] & (2 ** 64 - 1)}

    def guards(self):
        """The ``guard_rows`` slots before and after the ring."""
        return self._alloc[:self._guard], self._alloc[self._guard + self.capacity:]
