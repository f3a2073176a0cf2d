"""``ImageRolloutBuffer`` -- ``RolloutBuffer``'s life cycle and rules for the ``-v1`` picture ids: an on-policy rollout buffer of uint8
pictures on the GPU (``mcg_rollout_img_*``; PPO and A2C are how the reference trains from a picture, scripts/train.py:99-101).

    envs = make("MyCobotReach-Dense-joint-v1", num_envs=8192)
    buf = ImageRolloutBuffer(envs, n_steps=32, gamma=0.99, gae_lambda=0.95, seed=0)
    img, info = envs.reset(seed=0);  buf.start(img)
    for _ in range(32):
        a, v, logp = policy(img)
        img, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, img, r, term, trunc, info, final_values=value_fn(info["final_observation"]))
    buf.finish(last_values=value_fn(img))
    for mb in buf.get(4096, normalize=True): ...     # mb.observations: float32 [B, C, S, S] in [0, 1]; normalize=False: uint8
    buf.reset()

The pixels are uint8 ``[n_steps + 1, N, P]``: row t is the picture the action of step t was taken from, ``add`` writes the picture
the step returned into the next row, and ``reset()`` copies the last row written to row 0.  Nothing else is carried, so an insertion
reads and writes every pixel once.  The planes, the advantage recursion and the permutation are ``RolloutBuffer``'s: equal
``(seed, epoch, n_steps, N)`` give equal ``index``.  No CPU or PyTorch fallback.

With ``frame_stack=k`` the buffer still stores single frames and ``get`` hands out stacks of the newest k, ``[B, k * C, S, S]``
(``mcg_rollout_img_gather_stacked``):

    fs = FrameStack(make("MyCobotReach-Dense-joint-v1", num_envs=8192), 4)
    buf = ImageRolloutBuffer(fs, n_steps=32, frame_stack=4)       # without the keyword: the stacks stored whole, as 4 * C channels
    stack, info = fs.reset(seed=0);  buf.start(stack)             # start and add take the stack or its newest frame

``pixels`` and the ``episode_start`` plane then have k - 1 more rows in front, the history: the last k - 1 pictures of the rollout
before and their flags, which ``reset()`` carries over together with the picture to continue from (``mcg_rollout_img_carry_stacked``).
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._devbuf import _ptr
from .rollout import _PLANES, RolloutSamples, _OnPolicyBuffer


class ImageRolloutBuffer(_OnPolicyBuffer):
    _ENTRY = "mcg_rollout_img"
    _IMAGES = True
    _FROM_ENVS = (("num_envs", "num_envs"), ("channels", "channels"), ("image_size", "image_size"), ("act_dim", "action_dim"))
    _NO_STATES = ("the -v0 ids observe float64 states with their goals: ImageRolloutBuffer stores uint8 pictures; "
                  "RolloutBuffer is the buffer for them")

    def __init__(self, envs=None, n_steps: int = 32, gamma: float = 0.99, gae_lambda: float = 0.95, seed: int = 0, *,
                 num_envs: Optional[int] = None, channels: Optional[int] = None, image_size: Optional[int] = None,
                 act_dim: Optional[int] = None, device=None, guard_rows: int = 0, frame_stack: Optional[int] = None):
        """``envs``: a ``MyCobotImgVecEnv`` to take the dimensions and device from; or give them by keyword.  ``guard_rows``: spare rows
        allocated before and after the pixels, the records and every plane, which no call may touch (``guards()``; tests).
        ``frame_stack`` = k > 1: single frames are stored and ``gather`` / ``get`` hand out stacks of the newest k, [B, k * C, S, S];
        of a ``FrameStack`` (whose ``frame_stack`` must be k) ``channels`` is then its ``frame_channels``.  None or 1: what is passed
        in is stored as it is -- a ``FrameStack``'s stacks as k * C channels."""
        from .frame_stack import FrameStack
        self.frame_stack = k = 1 if frame_stack is None else int(frame_stack)
        if not 1 <= k <= 8:
            raise ValueError(f"frame_stack must be in [1, 8], got {k}")
        if k > 1 and isinstance(envs, FrameStack):
            if envs.frame_stack != k:
                raise ValueError(f"frame_stack={k}, but the FrameStack stacks {envs.frame_stack} frames")
            channels = envs.frame_channels if channels is None else channels
        num_envs, channels, image_size, act_dim = self._resolve(envs, device, dict(num_envs=num_envs, channels=channels,
                                                                                   image_size=image_size, act_dim=act_dim))
        self.num_envs, self.channels, self.image_size, self.act_dim = int(num_envs), int(channels), int(image_size), int(act_dim)
        self._host_state(n_steps, gamma, gae_lambda, seed, guard_rows)
        self.record_bytes = int(self._lib.mcg_rollout_img_record_bytes(self.act_dim))
        self.picture_bytes = max(self.channels, 1) * max(self.image_size, 1) ** 2
        self.row_bytes = (self.picture_bytes + 15) // 16 * 16
        g = self._guard
        n, T, dev = max(self.num_envs, 1), max(self.n_steps, 1), self.device
        # the k - 1 rows of history in front of row 0 of the pixels and of the episode_start plane (include/mcg.h: the stacked entries)
        hist = {"pixels": k - 1, "episode_start": k - 1}
        # (a refused shape still gets small tensors: the C side refuses it with its own message at the first call)
        self._alloc = {"pixels": torch.zeros(k - 1 + T + 1 + 2 * g, n, self.row_bytes, dtype=torch.uint8, device=dev),
                       "records": torch.zeros(T + 2 * g, n, max(self.record_bytes, 16), dtype=torch.uint8, device=dev)}
        self._alloc.update({name: torch.zeros(hist.get(name, 0) + T + 2 * g, n, dtype=dt, device=dev) for name, dt in _PLANES})
        self._t = {name: v[g + hist.get(name, 0):v.shape[0] - g] for name, v in self._alloc.items()}
        self._history = {name: self._alloc[name][g:g + rows] for name, rows in hist.items()}
        self._t["last_start"] = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._cbuf = _abi.McgRolloutImgBuf(**{k: v.data_ptr() for k, v in self._t.items()}, n_envs=self.num_envs, channels=self.channels,
                                           size=self.image_size, act_dim=self.act_dim, n_steps=self.n_steps, gamma=self.gamma,
                                           gae_lambda=self.gae_lambda)

    # ----------------------------------------------------------------------------------------------------- insertion
    def _picture(self, img, name):
        """As ``DeviceBuffer._picture``; with ``frame_stack`` > 1 also a stack [N, k * C, S, S], of which the newest C channels are
        taken as a strided view: the buffer stores single frames."""
        k = self.frame_stack
        if k > 1:
            img = torch.as_tensor(img, device=self.device)
            if img.dim() == 4 and img.shape[1] == k * self.channels:
                img = img[:, (k - 1) * self.channels:]
        return super()._picture(img, name)

    def start(self, img, mask=None):
        """The environments of ``mask`` (None: all) continue from ``img`` (what ``reset`` returned), as the first step of an episode."""
        t, es, cs = self._picture(img, "img")
        m = None if mask is None else self._dev(mask, torch.uint8, (self.num_envs,), "mask")
        self._call("mcg_rollout_img_start", self.pos, _ptr(t), es, cs, _ptr(m))

    def add(self, actions, values, log_probs, img, reward, terminated, truncated, info=None, final_values=None):
        """One step per environment: ``buf.add(a, v, logp, *envs.step(a))``.  ``final_values``: the value estimate of
        ``info["final_observation"]``, float [N]; where the time limit alone ended an episode, ``gamma`` times it is added to the
        reward (SB3's bootstrap); None: no bootstrap.  ``info`` itself is not read."""
        a, v, lp, fv = self._policy_outputs(actions, values, log_probs, final_values)
        t, es, cs = self._picture(img, "img")
        n = self.num_envs
        r = self._dev(reward, torch.float64, (n,), "reward")              # (the sparse reward comes back as float32: one small cast)
        term, trunc = self._dev(terminated, torch.bool, (n,), "terminated"), self._dev(truncated, torch.bool, (n,), "truncated")
        self._call("mcg_rollout_img_add", self.pos, _ptr(a), _ptr(v), _ptr(lp), _ptr(fv), _ptr(t), es, cs, _ptr(r), _ptr(term), _ptr(trunc))
        self.pos += 1
        self.finished = False

    def reset(self):
        """The next rollout starts at step 0 and continues from the last picture written: one launch copies its row to row 0.  Its
        episode-start flag carries over as it is: episodes go on across rollouts.  With ``frame_stack`` = k > 1 the same launch moves
        the k - 1 pictures before it and their flags into the history rows."""
        if self.frame_stack == 1:
            self._call("mcg_rollout_img_carry", self.pos)
        else:
            self._call("mcg_rollout_img_carry_stacked", self.pos, self.frame_stack)
        super().reset()

    # ---------------------------------------------------------------------------------------------------- minibatches
    def gather(self, epoch: int, first: int, count: int, normalize: bool = True) -> RolloutSamples:
        """Samples ``first .. first + count - 1`` of epoch ``epoch``'s permutation (what ``get`` yields, one minibatch at a time).
        ``observations``: float32 [B, C, S, S], the byte / 255 (SB3's ``obs.float() / 255``, bit for bit); ``normalize=False``: the uint8
        picture.  With ``frame_stack`` = k: [B, k * C, S, S], slot k - 1 (the last C channels) the picture the action was taken from,
        the slots from before the episode's start zeros."""
        A, dev = self.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        rows = max(int(count), 1)
        pix = torch.empty(rows, self.frame_stack * self.channels, self.image_size, self.image_size, dtype=torch.float32 if normalize else torch.uint8, device=dev)
        t = {"pix_f32" if normalize else "pix": pix, "action": torch.empty(rows, A, **f32), "old_value": torch.empty(rows, **f32),
             "old_log_prob": torch.empty(rows, **f32), "advantage": torch.empty(rows, **f32), "returns": torch.empty(rows, **f32),
             "index": torch.empty(rows, dtype=torch.int32, device=dev)}
        out = _abi.McgRolloutImgBatch(**{k: v.data_ptr() for k, v in t.items()})
        where = (C.c_uint64(self.seed), C.c_uint64(int(epoch) & (2 ** 64 - 1)), int(first), int(count), C.byref(out))
        if self.frame_stack == 1:
            self._call("mcg_rollout_img_gather", *where)
        else:
            self._call("mcg_rollout_img_gather_stacked", self.frame_stack, *where)
        return RolloutSamples(observations=pix, actions=t["action"], old_values=t["old_value"], old_log_prob=t["old_log_prob"],
                              advantages=t["advantage"], returns=t["returns"], index=t["index"])

    # ------------------------------------------------------------------------------------------------------- storage
    def pixels(self) -> torch.Tensor:
        """The pictures, uint8 [n_steps + 1, N, C, S, S] (a view, without the padding of a row): row t is what the action of step t
        was taken from -- a single frame, whatever ``frame_stack`` is."""
        return self._t["pixels"][:, :, :self.picture_bytes].unflatten(2, (self.channels, self.image_size, self.image_size))

    def history(self) -> torch.Tensor:
        """The ``frame_stack - 1`` rows before row 0 of ``pixels()``, uint8 [k - 1, N, C, S, S] (a view): the pictures of the rollout
        before that the stacks of this one's first steps reach back to, the oldest first."""
        return self._history["pixels"][:, :, :self.picture_bytes].unflatten(2, (self.channels, self.image_size, self.image_size))

    def history_start(self) -> torch.Tensor:
        """The episode-start flags of ``history()``'s rows, uint8 [k - 1, N] (a view)."""
        return self._history["episode_start"]

    def state_dict(self) -> dict:
        """``DeviceBuffer.state_dict``; with ``frame_stack`` > 1 also the history rows and their flags."""
        sd = super().state_dict()
        if self.frame_stack > 1:
            sd.update(history=self._history["pixels"].clone(), history_start=self._history["episode_start"].clone())
        return sd

    def load_state_dict(self, sd: dict):
        if self.frame_stack > 1:
            rows = (("history", self._history["pixels"]), ("history_start", self._history["episode_start"]))
            src = {key: torch.as_tensor(sd[key], device=self.device) for key, _ in rows}
            for key, v in rows:          # both checked before either is written
                if src[key].shape != v.shape or src[key].dtype != v.dtype:
                    raise ValueError(f"{key}: expected {v.dtype} {tuple(v.shape)}, got {src[key].dtype} {tuple(src[key].shape)}")
            for key, v in rows:
                v.copy_(src[key])
        super().load_state_dict(sd)
