"""``ImageReplayBuffer`` -- an off-policy replay buffer for the ``-v1`` picture ids whose storage, insertion and sampling live on the GPU.

What the reference trains SAC, TD3 and DDPG from is SB3's ``ReplayBuffer`` (scripts/train.py:62, 102-104).  This is the same rule on
the engine's N lockstep environments and on uint8 pictures (``mcg_replay_img_*``): a time-major ring ``[capacity + 1, N]`` that stores
every picture once -- the next picture of a slot is the following row -- and keeps the last picture of an episode that the time limit
ended in a side table, so a timeout is not taken for a termination.

    envs = make("MyCobotReach-Dense-joint-v1", num_envs=8192)
    buf = ImageReplayBuffer(envs, capacity=1000, seed=0)          # envs: or a FrameStack around it; then sample() hands out stacks
    img, _ = envs.reset(seed=0);  buf.start(img)
    out = envs.step(a);           buf.add(a, *out)
    batch = buf.sample(4096)          # batch.observations, batch.next_observations: float32 [B, C, S, S] in [0, 1]

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

# SB3's ReplayBufferSamples names, and `index` [B, 3]: row, env, where the next picture came from (0: the ring, 1: the final pictures)
ReplaySamples = namedtuple("ReplaySamples", ["observations", "actions", "next_observations", "dones", "rewards", "index"])


class ImageReplayBuffer(DeviceBuffer):
    _IMAGES = True
    _FROM_ENVS = (("num_envs", "num_envs"), ("channels", "channels"), ("image_size", "image_size"), ("act_dim", "action_dim"),
                  ("max_episode_steps", "max_episode_steps"))
    _NO_STATES = ("the -v0 ids observe float64 states with their goals: ImageReplayBuffer stores uint8 pictures; "
                  "HerBuffer is the buffer for them")
    _HOST_STATE = ("n_written", "n_sampled", "seed")

    def __init__(self, envs=None, capacity: int = 1000, seed: int = 0, *, num_envs: Optional[int] = None, channels: Optional[int] = None,
                 image_size: Optional[int] = None, act_dim: Optional[int] = None, max_episode_steps: Optional[int] = None, device=None,
                 guard_rows: int = 0, frame_stack: Optional[int] = None):
        """``envs``: a ``MyCobotImgVecEnv`` to take the dimensions, time limit and device from, or a ``FrameStack`` around one
        (``channels`` is then its ``frame_channels`` and ``frame_stack`` its ``frame_stack``); or give them by keyword.  ``capacity``:
        transitions kept per environment.  ``guard_rows``: spare rows allocated before and after the pixels, the final pictures, their
        stamps and the records, which no call may touch (``guards()``; tests).  ``frame_stack`` = k > 1: ``sample`` hands out stacks of
        the newest k frames, [B, k * C, S, S], rebuilt from the ring of single frames, which gets k - 1 more rows (``capacity + k`` in
        all): the history of the oldest transitions."""
        from .frame_stack import FrameStack
        if isinstance(envs, FrameStack):
            channels = envs.frame_channels if channels is None else channels
            frame_stack = envs.frame_stack if frame_stack is None else frame_stack
        self.frame_stack = k = 1 if frame_stack is None else int(frame_stack)
        if not 1 <= k <= 8:
            raise ValueError(f"frame_stack must be in [1, 8], got {k}")
        num_envs, channels, image_size, act_dim, max_episode_steps = self._resolve(envs, device, dict(
            num_envs=num_envs, channels=channels, image_size=image_size, act_dim=act_dim, max_episode_steps=max_episode_steps))
        self.num_envs, self.channels, self.image_size, self.act_dim = int(num_envs), int(channels), int(image_size), int(act_dim)
        self.capacity, self.max_episode_steps = int(capacity), int(max_episode_steps)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.n_written = 0           # insertions so far: the absolute time of the next transition
        self.n_sampled = 0           # sample() calls so far: the `call` word of the sampling draws
        self.record_bytes = int(self._lib.mcg_replay_img_record_bytes(self.act_dim))
        self.picture_bytes = max(self.channels, 1) * max(self.image_size, 1) ** 2
        self.row_bytes = (self.picture_bytes + 15) // 16 * 16
        self._guard = g = int(guard_rows)
        # (the C side's capacity: with the k - 1 rows of history that are never sampled)
        n, K, Tm, dev = max(self.num_envs, 1), max(self.capacity, 1) + k - 1, max(self.max_episode_steps, 1), self.device
        self.rows, self.final_rows = K + 1, -(-K // Tm) + 1
        # (a refused shape still gets small tensors: the C side refuses it with its own message at the first call)
        self._alloc = {"pixels": torch.zeros(self.rows + 2 * g, n, self.row_bytes, dtype=torch.uint8, device=dev),
                       "finals": torch.zeros(self.final_rows + 2 * g, n, self.row_bytes, dtype=torch.uint8, device=dev),
                       "final_time": torch.full((self.final_rows + 2 * g, n), -1, dtype=torch.int64, device=dev),
                       "records": torch.zeros(self.rows + 2 * g, n, max(self.record_bytes, 16), dtype=torch.uint8, device=dev)}
        self._t = {k: v[g:v.shape[0] - g] for k, v in self._alloc.items()}
        self._t["counters"] = torch.zeros(2, dtype=torch.int64, device=dev)          # uint64 counts carried in an int64 tensor
        self._cbuf = _abi.McgReplayImgBuf(**{k: v.data_ptr() for k, v in self._t.items()}, n_envs=self.num_envs, channels=self.channels,
                                          size=self.image_size, act_dim=self.act_dim, capacity=self.capacity + k - 1,
                                          max_episode_steps=self.max_episode_steps)

    # ----------------------------------------------------------------------------------------------------- insertion
    def _picture(self, img, name):
        """As ``DeviceBuffer._picture``; with ``frame_stack`` > 1 also a stack [N, k * C, S, S], of which the newest C channels are
        taken as a strided view: the ring stores single frames."""
        k = self.frame_stack
        if k > 1:
            img = torch.as_tensor(img, device=self.device)
            if img.dim() == 4 and img.shape[1] == k * self.channels:
                img = img[:, (k - 1) * self.channels:]
        return super()._picture(img, name)

    def start(self, img, mask=None):
        """The environments of ``mask`` (None: all) continue from ``img`` (what ``reset`` returned).  Where that cuts an episode in
        flight, its last transition has lost its next picture and is never sampled; after an episode's end nothing is lost."""
        t, es, cs = self._picture(img, "img")
        m = None if mask is None else self._dev(mask, torch.uint8, (self.num_envs,), "mask")
        self._call("mcg_replay_img_start", self.n_written, _ptr(t), es, cs, _ptr(m))

    def add(self, actions, img, reward, terminated, truncated, info):
        """One transition per environment: ``buf.add(a, *envs.step(a))``.  ``img`` is the next picture everywhere but where the time
        limit alone ended the episode: there it is ``info["final_observation"]`` (``img`` already belongs to the next episode)."""
        n = self.num_envs
        a = self._dev(torch.as_tensor(actions, device=self.device).detach(), torch.float32, (n, self.act_dim), "actions")
        t, es, cs = self._picture(img, "img")
        f, fes, fcs = self._picture(info["final_observation"], "info['final_observation']")
        r = self._dev(reward, torch.float64, (n,), "reward")              # (the sparse reward comes back as float32: one small cast)
        term, trunc = self._dev(terminated, torch.bool, (n,), "terminated"), self._dev(truncated, torch.bool, (n,), "truncated")
        self._call("mcg_replay_img_add", self.n_written, _ptr(a), _ptr(t), es, cs, _ptr(f), fes, fcs, _ptr(r), _ptr(term), _ptr(trunc))
        self.n_written += 1

    # ------------------------------------------------------------------------------------------------------ sampling
    def sample(self, batch_size: int, normalize: bool = True, check: bool = True) -> ReplaySamples:
        """A uniform batch of stored transitions: device tensors under SB3's ``ReplayBufferSamples`` names, and ``index``.  Pictures are
        float32 [B, C, S, S] ([B, k * C, S, S] with ``frame_stack`` = k: slot k - 1, the last C channels, is the newest frame, and the
        slots from before the episode's start are zeros), the byte / 255 (SB3's ``obs.float() / 255``, bit for bit);
        ``normalize=False``: uint8.  ``dones`` is 1
        where the episode terminated and 0 where the time limit ended it (SB3's ``dones * (1 - timeouts)``): there
        ``next_observations`` is the finished episode's last picture.  Where it terminated, ``next_observations`` is the next
        episode's first picture: its weight in a TD target is zero.  ``check=True`` reads the give-up counter (the one synchronising
        path) and raises if a sample found no valid transition in 256 draws; ``check=False`` never synchronises: such a sample has
        index -1 and zeros."""
        B, A, dev = int(batch_size), self.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        rows = max(B, 1)
        shape = (rows, self.frame_stack * self.channels, self.image_size, self.image_size)
        dt = torch.float32 if normalize else torch.uint8
        pix, nxt = torch.empty(shape, dtype=dt, device=dev), torch.empty(shape, dtype=dt, device=dev)
        t = {"pix_f32" if normalize else "pix": pix, "next_pix_f32" if normalize else "next_pix": nxt, "action": torch.empty(rows, A, **f32),
             "reward": torch.empty(rows, 1, **f32), "done": torch.empty(rows, 1, **f32),
             "index": torch.empty(rows, 3, dtype=torch.int32, device=dev)}
        out = _abi.McgReplayImgBatch(**{k: v.data_ptr() for k, v in t.items()})
        before = self.counters()["sample_give_ups"] if check else 0
        if self.frame_stack == 1:
            self._call("mcg_replay_img_sample", self.n_written, C.c_uint64(self.seed), C.c_uint64(self.n_sampled), B, C.byref(out))
        else:
            self._call("mcg_replay_img_sample_stacked", self.n_written, C.c_uint64(self.seed), C.c_uint64(self.n_sampled), B, self.frame_stack,
                       C.byref(out))
        self.n_sampled += 1
        if check:
            gave_up = self.counters()["sample_give_ups"] - before
            if gave_up:
                raise RuntimeError(f"ImageReplayBuffer.sample: {gave_up} of {B} samples found no valid transition in 256 draws "
                                   f"({self.n_written} insertions; did start() cut every stored episode?)")
        return ReplaySamples(observations=pix, actions=t["action"], next_observations=nxt, dones=t["done"], rewards=t["reward"],
                             index=t["index"])

    # --------------------------------------------------------------------------------------------- counters, storage
    def counters(self) -> dict:
        """``sample_give_ups``: samples that found no valid transition; ``finals_overwritten``: samples of a time-limit end whose final
        picture had been overwritten (they came out as terminal).  Synchronises."""
        c = self._t["counters"].cpu().tolist()
        return {"sample_give_ups": c[0] & (2 ** 64 - 1), "finals_overwritten": c[1] & (2 ** 64 - 1)}

    def guards(self) -> dict:
        """Per allocation (pixels, finals, final_time, records): the ``guard_rows`` rows before and after it."""
        g = self._guard
        return {k: (v[:g], v[v.shape[0] - g:]) for k, v in self._alloc.items()}

    def pixels(self) -> torch.Tensor:
        """The pictures, uint8 [rows, N, C, S, S] with rows = capacity + frame_stack (a view, without the padding of a row): row
        ``a % rows`` is what the action of transition ``a`` was taken from -- a single frame, whatever ``frame_stack`` is."""
        return self._t["pixels"][:, :, :self.picture_bytes].unflatten(2, (self.channels, self.image_size, self.image_size))

    @property
    def nbytes(self) -> int:
        """Bytes of device memory the buffer holds."""
        return sum(v.numel() * v.element_size() for v in (*self._alloc.values(), self._t["counters"]))
