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
(PPO does that per minibatch).  The -v1 picture ids have ``ImageRolloutBuffer`` (rollout_img.py); what the two share is
``_OnPolicyBuffer`` below.
"""
from __future__ import annotations

import ctypes as C
from collections import namedtuple
from typing import Optional

import torch

from . import _abi
from ._devbuf import DeviceBuffer, _ptr

# SB3's RolloutBufferSamples names, and `index` [B]: the sample's flat index in SB3's swap_and_flatten order, env * n_steps + step
RolloutSamples = namedtuple("RolloutSamples", ["observations", "actions", "old_values", "old_log_prob", "advantages", "returns", "index"])

_PLANES = (("reward", torch.float32), ("value", torch.float32), ("episode_start", torch.uint8), ("advantage", torch.float32),
           ("returns", torch.float32))


class _OnPolicyBuffer(DeviceBuffer):
    """What ``RolloutBuffer`` and ``ImageRolloutBuffer`` share: the host state, the order of calls, the planes and their guards.  A
    subclass sets ``_ENTRY`` (the prefix of its C entries), fills ``self._alloc`` (name -> tensor with its guard rows) and implements
    ``start``, ``add`` and ``gather``."""
    _HOST_STATE = ("pos", "epoch", "seed", "finished")

    def _host_state(self, n_steps, gamma, gae_lambda, seed, guard_rows):
        self.n_steps, self.gamma, self.gae_lambda = int(n_steps), float(gamma), float(gae_lambda)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.pos = 0                 # steps of the rollout in flight
        self.epoch = 0               # get() calls so far: the `epoch` word of the permutation
        self.finished = False        # finish() has run on the rollout in flight
        self._guard = int(guard_rows)

    def _per_env(self, x, name):
        """float32 [N]; a trailing axis of one (a value head's [N, 1]) is dropped."""
        t = torch.as_tensor(x, device=self.device)
        if t.dim() == 2 and t.shape[1] == 1:
            t = t[:, 0]
        return self._dev(t.detach(), torch.float32, (self.num_envs,), name)

    def _policy_outputs(self, actions, values, log_probs, final_values):
        """What ``add`` takes from the policy, as the C side takes it; refuses a full buffer."""
        if self.pos >= self.n_steps:
            raise ValueError(f"{type(self).__name__}.add: the buffer is full ({self.n_steps} steps); finish(), get() and reset() come first")
        a = self._dev(torch.as_tensor(actions, device=self.device).detach(), torch.float32, (self.num_envs, self.act_dim), "actions")
        fv = None if final_values is None else self._per_env(final_values, "final_values")
        return a, self._per_env(values, "values"), self._per_env(log_probs, "log_probs"), fv

    @property
    def full(self) -> bool:
        return self.pos >= self.n_steps

    def finish(self, last_values):
        """Advantages and returns of the full rollout (GAE); ``last_values``: the value estimate of the current observation, float [N]."""
        if not self.full:
            raise ValueError(f"{type(self).__name__}.finish: the rollout has {self.pos} of {self.n_steps} steps")
        lv = self._per_env(last_values, "last_values")
        self._call(self._ENTRY + "_gae", _ptr(lv))
        self.finished = True

    def get(self, batch_size: Optional[int] = None, **how):
        """One epoch: the ``n_steps * N`` transitions in a fresh random order, in minibatches of ``batch_size`` (None: one batch; the
        last one may be short), each a ``RolloutSamples`` of device tensors from one launch.  Every call is a new epoch.  ``how``:
        ``gather``'s keywords."""
        if not self.full:
            raise ValueError(f"{type(self).__name__}.get: the rollout has {self.pos} of {self.n_steps} steps")
        if not self.finished:
            raise ValueError(f"{type(self).__name__}.get: finish(last_values) comes first")
        M = self.n_steps * self.num_envs
        B = M if batch_size is None else int(batch_size)
        if B < 1:
            raise ValueError("batch_size must be >= 1")
        epoch = self.epoch
        self.epoch += 1
        return (self.gather(epoch, first, min(B, M - first), **how) for first in range(0, M, B))

    def reset(self):
        """The next rollout starts at step 0.  The observation to continue from and its episode-start flag carry over: episodes go
        on across rollouts."""
        self.pos = 0
        self.finished = False

    def planes(self) -> dict:
        """reward, value, episode_start, advantage, returns: [n_steps, N] views."""
        return {k: self._t[k] for k, _ in _PLANES}

    def guards(self) -> dict:
        """Per allocation (the records, the five planes, and a picture buffer's pixels): the ``guard_rows`` rows before and after it."""
        g = self._guard
        return {k: (v[:g], v[v.shape[0] - g:]) for k, v in self._alloc.items()}


class RolloutBuffer(_OnPolicyBuffer):
    _ENTRY = "mcg_rollout"
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"))
    _NO_IMAGES = ("the -v1 image ids observe uint8 pictures: RolloutBuffer stores float32 state observations with their "
                  "goals; picture records are not supported")

    def __init__(self, envs=None, n_steps: int = 64, gamma: float = 0.99, gae_lambda: float = 0.95, seed: int = 0, *,
                 num_envs: Optional[int] = None, obs_dim: Optional[int] = None, act_dim: Optional[int] = None, device=None,
                 guard_rows: int = 0):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions and device from; or give them by keyword.  ``guard_rows``: spare rows
        allocated before and after the records and every plane, which no call may touch (``guards()``; tests)."""
        num_envs, obs_dim, act_dim = self._resolve(envs, device, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim))
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        self._host_state(n_steps, gamma, gae_lambda, seed, guard_rows)
        self.record_bytes = int(self._lib.mcg_rollout_record_bytes(self.obs_dim, self.act_dim))
        g = self._guard
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

    # ----------------------------------------------------------------------------------------------------- insertion
    def start(self, obs, mask=None):
        """The environments of ``mask`` (None: all) continue from ``obs`` (what ``reset`` returned), as the first step of an episode."""
        o, ag, dg = self._goal_obs(obs, "obs")
        m = None if mask is None else self._dev(mask, torch.uint8, (self.num_envs,), "mask")
        first = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        self._call("mcg_rollout_start", C.byref(first), _ptr(m))

    def add(self, actions, values, log_probs, obs, reward, terminated, truncated, info=None, final_values=None):
        """One step per environment: ``buf.add(a, v, logp, *envs.step(a))``.  ``final_values``: the value estimate of
        ``info["final_observation"]``, float [N]; where the time limit alone ended an episode, ``gamma`` times it is added to the
        reward (SB3's bootstrap); None: no bootstrap.  ``info`` itself is not read."""
        a, v, lp, fv = self._policy_outputs(actions, values, log_probs, final_values)
        out, _alive = self._step_out(obs, reward, terminated, truncated)
        self._call("mcg_rollout_add", self.pos, _ptr(a), _ptr(v), _ptr(lp), _ptr(fv), C.byref(out))
        self.pos += 1
        self.finished = False

    # ---------------------------------------------------------------------------------------------------- minibatches
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
        self._call("mcg_rollout_gather", C.c_uint64(self.seed), C.c_uint64(int(epoch) & (2 ** 64 - 1)), int(first), int(count), C.byref(out))
        return RolloutSamples(observations={"observation": t["obs"], "achieved_goal": t["achieved"], "desired_goal": t["desired"]},
                              actions=t["action"], old_values=t["old_value"], old_log_prob=t["old_log_prob"],
                              advantages=t["advantage"], returns=t["returns"], index=t["index"])
