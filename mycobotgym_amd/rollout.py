"""``RolloutBuffer`` -- an on-policy rollout buffer whose storage, advantage recursion and minibatch gather live on the GPU.

What the reference trains PPO and A2C with is SB3's ``RolloutBuffer`` (``n_steps``; scripts/train.py:99-101).  This is the same rule on
the engine's N lockstep environments: time-major ``[n_steps, N]`` storage, one launch to insert a step with the time-limit bootstrap
(``mcg_rollout_add``), one for the backward recursion (``mcg_rollout_gae``), one per shuffled minibatch (``mcg_rollout_gather``).

    buf = RolloutBuffer(envs, n_steps=64, gamma=0.99, gae_lambda=0.95, seed=0)
    obs, _ = envs.reset(seed=0);  buf.start(obs)
    for _ in range(64):
        a, v, logp = policy(obs)
        obs, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, obs, r, term, trunc, info, final_values=value_fn(info["final_observation"]))
    buf.finish(last_values=value_fn(obs))
    for mb in buf.get(batch_size=4096): ...
    buf.reset()

This file owns the device memory (PyTorch tensors) and three host integers (``pos``, ``epoch``, ``seed``); the C side keeps no state
and no call synchronises.  No CPU or PyTorch fallback: the kernels are the only implementation.  Advantages are not normalised here
(PPO does that per minibatch).
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import torch

from . import _abi

# SB3's RolloutBufferSamples names, and `index` [B]: the sample's flat index in SB3's swap_and_flatten order, env * n_steps + step
RolloutSamples = namedtuple("RolloutSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns", "index"])

_PLANES = (("reward", torch.float32), ("value", torch.float32), ("episode_start", torch.uint8), ("advantage", torch.float32),
           ("returns", torch.float32))


class RolloutBuffer:
    def __init__(self, envs=None, n_steps: int = 64, gamma: float = 0.99, gae_lambda: float = 0.95, seed: int = 0, *,
                 num_envs: Optional[int] = None, obs_dim: Optional[int] = None, act_dim: Optional[int] = None, device=None,
                 guard_rows: int = 0):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions and device from; or give them by keyword.  ``guard_rows``: spare rows
        allocated before and after the records and every plane, which no call may touch (``guards()``; tests)."""
        if envs is not None:
            from .vec_env import MyCobotImgVecEnv
            if isinstance(envs, MyCobotImgVecEnv):
                raise ValueError("the -v1 image ids observe uint8 pictures: RolloutBuffer stores float32 state observations with their "
                                 "goals; picture records are not supported")
            num_envs = envs.num_envs if num_envs is None else num_envs
            obs_dim = envs.obs_dim if obs_dim is None else obs_dim
            act_dim = envs.action_dim if act_dim is None else act_dim
            device = envs.device if device is None else device
        missing = [k for k, v in (("num_envs", num_envs), ("obs_dim", obs_dim), ("act_dim", act_dim)) if v is None]
        if missing:
            raise ValueError(f"RolloutBuffer needs envs= or {', '.join(missing)}")
        self.device = torch.device("cuda:0" if device is None else device)
        if self.device.type != "cuda":
            raise _abi.McgError("RolloutBuffer lives on an AMD GPU only (device='cuda:N'); there is no CPU path")
        self._lib = _abi.load()
        self.num_envs, self.obs_dim, self.act_dim, self.n_steps = int(num_envs), int(obs_dim), int(act_dim), int(n_steps)
        self.gamma, self.gae_lambda = float(gamma), float(gae_lambda)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.pos = 0                 # steps of the rollout in flight
        self.epoch = 0               # get() calls so far: the `epoch` word of the permutation
        self.finished = False        # finish() has run on the rollout in flight
        self.record_bytes = int(self._lib.mcg_rollout_record_bytes(self.obs_dim, self.act_dim))
        self._guard = g = int(guard_rows)
        n, D, T, dev = max(self.num_envs, 1), max(self.obs_dim, 1), max(self.n_steps, 1), self.device
        # (a refused shape still gets small tensors: the C side refuses it with its own message at the first call)
        self._alloc = {"records": torch.zeros(T + 2 * g, n, max(self.record_bytes, 16), dtype=torch.uint8, device=dev)}
        self._alloc.update({k: torch.zeros(T + 2 * g, n, dtype=dt, device=dev) for k, dt in _PLANES})
        self._t = {k: v[g:g + T] for k, v in self._alloc.items()}
        self._t.update(last_obs=torch.zeros(n, D, dtype=torch.float32, device=dev),
                       last_goals=torch.zeros(n, 6, dtype=torch.float32, device=dev),
                       last_start=torch.zeros(n, dtype=torch.uint8, device=dev))
        self._cbuf = _abi.McgRolloutBuf(**{k: v.data_ptr() for k, v in self._t.items()}, n_envs=self.num_envs, obs_dim=self.obs_dim,
                                        act_dim=self.act_dim, n_steps=self.n_steps, gamma=self.gamma, gae_lambda=self.gae_lambda)

    # ------------------------------------------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _dev(self, x, dtype, shape, name):
        t = torch.as_tensor(x, device=self.device)
        if t.dtype != dtype:
            t = t.to(dtype)
        t = t.contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _per_env(self, x, name):
        """float32 [N]; a trailing axis of one (a value head's [N, 1]) is dropped."""
        t = torch.as_tensor(x, device=self.device)
        if t.dim() == 2 and t.shape[1] == 1:
            t = t[:, 0]
        return self._dev(t.detach(), torch.float32, (self.num_envs,), name)

    def _goal_obs(self, obs, name):
        n, D = self.num_envs, self.obs_dim
        return (self._dev(obs["observation"], torch.float64, (n, D), name + "['observation']"),
                self._dev(obs["achieved_goal"], torch.float64, (n, 3), name + "['achieved_goal']"),
                self._dev(obs["desired_goal"], torch.float64, (n, 3), name + "['desired_goal']"))

    # ----------------------------------------------------------------------------------------------------- insertion
    def start(self, obs, mask=None):
        """The environments of ``mask`` (None: all) continue from ``obs`` (what ``reset`` returned), as the first step of an episode."""
        o, ag, dg = self._goal_obs(obs, "obs")
        m = None if mask is None else self._dev(mask, torch.uint8, (self.num_envs,), "mask")
        first = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_rollout_start(C.byref(self._cbuf), C.byref(first), None if m is None else C.c_void_p(m.data_ptr()),
                                                   self._stream()), "mcg_rollout_start")

    def add(self, actions, values, log_probs, obs, reward, terminated, truncated, info=None, final_values=None):
        """One step per environment: ``buf.add(a, v, logp, *envs.step(a))``.  ``final_values``: the value estimate of
        ``info["final_observation"]``, float [N]; where the time limit alone ended an episode, ``gamma`` times it is added to the
        reward (SB3's bootstrap); None: no bootstrap.  ``info`` itself is not read."""
        if self.pos >= self.n_steps:
            raise ValueError(f"RolloutBuffer.add: the buffer is full ({self.n_steps} steps); finish(), get() and reset() come first")
        n = self.num_envs
        a = self._dev(torch.as_tensor(actions, device=self.device).detach(), torch.float32, (n, self.act_dim), "actions")
        v, lp = self._per_env(values, "values"), self._per_env(log_probs, "log_probs")
        fv = None if final_values is None else self._per_env(final_values, "final_values")
        o, ag, dg = self._goal_obs(obs, "obs")
        r = self._dev(reward, torch.float64, (n,), "reward")           # (the sparse reward comes back as float32: one small cast)
        term = self._dev(terminated, torch.bool, (n,), "terminated")
        trunc = self._dev(truncated, torch.bool, (n,), "truncated")
        out = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr(), reward=r.data_ptr(),
                              terminated=term.data_ptr(), truncated=trunc.data_ptr())
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_rollout_add(C.byref(self._cbuf), self.pos, C.c_void_p(a.data_ptr()), C.c_void_p(v.data_ptr()),
                                                 C.c_void_p(lp.data_ptr()), None if fv is None else C.c_void_p(fv.data_ptr()),
                                                 C.byref(out), self._stream()), "mcg_rollout_add")
        self.pos += 1
        self.finished = False

    # ------------------------------------------------------------------------------------- advantages and minibatches
    @property
    def full(self) -> bool:
        return self.pos >= self.n_steps

    def finish(self, last_values):
        """Advantages and returns of the full rollout (GAE); ``last_values``: the value estimate of the current observation, float [N]."""
        if not self.full:
            raise ValueError(f"RolloutBuffer.finish: the rollout has {self.pos} of {self.n_steps} steps")
        lv = self._per_env(last_values, "last_values")
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_rollout_gae(C.byref(self._cbuf), C.c_void_p(lv.data_ptr()), self._stream()), "mcg_rollout_gae")
        self.finished = True

    def get(self, batch_size: Optional[int] = None):
        """One epoch: the ``n_steps * N`` transitions in a fresh random order, in minibatches of ``batch_size`` (None: one batch; the
        last one may be short), each a ``RolloutSamples`` of float32 device tensors from one launch.  Every call is a new epoch."""
        if not self.full:
            raise ValueError(f"RolloutBuffer.get: the rollout has {self.pos} of {self.n_steps} steps")
        if not self.finished:
            raise ValueError("RolloutBuffer.get: finish(last_values) comes first")
        M = self.n_steps * self.num_envs
        B = M if batch_size is None else int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        epoch = self.epoch
        self.epoch += 1
        return (self.gather(epoch, first, min(B, M - first)) for first in range(0, M, B))

    def gather(self, epoch: int, first: int, count: int) -> RolloutSamples:
        """Samples ``first .. first + count - 1`` of epoch ``epoch``'s permutation (what ``get`` yields, one minibatch at a time)."""
        D, A, dev = self.obs_dim, self.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        rows = max(int(count), 1)
        t = {"obs": torch.empty(rows, D, **f32), "achieved": torch.empty(rows, 3, **f32), "desired": torch.empty(rows, 3, **f32),
             "action": torch.empty(rows, A, **f32), "old_value": torch.empty(rows, **f32), "old_log_prob": torch.empty(rows, **f32),
             "advantage": torch.empty(rows, **f32), "returns": torch.empty(rows, **f32),
             "index": torch.empty(rows, dtype=torch.int32, device=dev)}
        out = _abi.McgRolloutBatch(**{k: v.data_ptr() for k, v in t.items()})
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_rollout_gather(C.byref(self._cbuf), C.c_uint64(self.seed), C.c_uint64(int(epoch) & (2 ** 64 - 1)),
                                                    int(first), int(count), C.byref(out), self._stream()), "mcg_rollout_gather")
        return RolloutSamples(observations={"observation": t["obs"], "achieved_goal": t["achieved"], "desired_goal": t["desired"]},
                              actions=t["action"], old_values=t["old_value"], old_log_prob=t["old_log_prob"],
                              advantages=t["advantage"], returns=t["returns"], index=t["index"])

    def reset(self):
        """The next rollout starts at step 0.  The observation to continue from and its episode-start flag carry over: episodes go
        on across rollouts."""
        self.pos = 0
        self.finished = False

    # ------------------------------------------------------------------------------------------- storage, checkpoints
    def records(self) -> torch.Tensor:
        """uint8 [n_steps, N, record_bytes] (a view; ``_abi.rollout_record_dtype`` names the fields of a record)."""
        return self._t["records"]

    def planes(self) -> dict:
        """reward, value, episode_start, advantage, returns: [n_steps, N] views."""
        return {k: self._t[k] for k, _ in _PLANES}

    def guards(self) -> dict:
        """Per allocation (records and the five planes): the ``guard_rows`` rows before and after it."""
        g, T = self._guard, max(self.n_steps, 1)
        return {k: (v[:g], v[g + T:]) for k, v in self._alloc.items()}

    def state_dict(self) -> dict:
        """The nine device tensors (cloned) and the host state: valid in mid-rollout too."""
        sd = {k: v.clone() for k, v in self._t.items()}
        sd.update(pos=self.pos, epoch=self.epoch, seed=self.seed, finished=self.finished)
        return sd

    def load_state_dict(self, sd: dict):
        for k, v in self._t.items():
            src = torch.as_tensor(sd[k], device=self.device)
            if src.shape != v.shape or src.dtype != v.dtype:
                raise ValueError(f"{k}: expected {v.dtype} {tuple(v.shape)}, got {src.dtype} {tuple(src.shape)}")
            v.copy_(src)
        self.pos, self.epoch = int(sd["pos"]), int(sd["epoch"])
        self.seed = int(sd["seed"]) & (2 ** 64 - 1)
        self.finished = bool(sd["finished"])
