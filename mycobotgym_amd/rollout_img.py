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
                 act_dim: Optional[int] = None, device=None, guard_rows: int = 0):
        """``envs``: a ``MyCobotImgVecEnv`` to take the dimensions and device from; or give them by keyword.  ``guard_rows``: spare rows
        allocated before and after the pixels, the records and every plane, which no call may touch (``guards()``; tests)."""
        num_envs, channels, image_size, act_dim = self._resolve(envs, device, dict(num_envs=num_envs, channels=channels,
                                                                                   image_size=image_size, act_dim=act_dim))
        self.num_envs, self.channels, self.image_size, self.act_dim = int(num_envs), int(channels), int(image_size), int(act_dim)
        self._host_state(n_steps, gamma, gae_lambda, seed, guard_rows)
        self.record_bytes = int(self._lib.mcg_rollout_img_record_bytes(self.act_dim))
        self.picture_bytes = max(self.channels, 1) * max(self.image_size, 1) ** 2
        self.row_bytes = (self.picture_bytes + 15) // 16 * 16
        g = self._guard
        n, T, dev = max(self.num_envs, 1), max(self.n_steps, 1), self.device
        # (a refused shape still gets small tensors: the C side refuses it with its own message at the first call)
        self._alloc = {"pixels": torch.zeros(T + 1 + 2 * g, n, self.row_bytes, dtype=torch.uint8, device=dev),
                       "records": torch.zeros(T + 2 * g, n, max(self.record_bytes, 16), dtype=torch.uint8, device=dev)}
        self._alloc.update({k: torch.zeros(T + 2 * g, n, dtype=dt, device=dev) for k, dt in _PLANES})
        self._t = {k: v[g:v.shape[0] - g] for k, v in self._alloc.items()}
        self._t["last_start"] = torch.zeros(n, dtype=torch.uint8, device=dev)
        self._cbuf = _abi.McgRolloutImgBuf(**{k: v.data_ptr() for k, v in self._t.items()}, n_envs=self.num_envs, channels=self.channels,
                                           size=self.image_size, act_dim=self.act_dim, n_steps=self.n_steps, gamma=self.gamma,
                                           gae_lambda=self.gae_lambda)

    # ----------------------------------------------------------------------------------------------------- insertion
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
        episode-start flag carries over as it is: episodes go on across rollouts."""
        self._call("mcg_rollout_img_carry", self.pos)
        super().reset()

    # ---------------------------------------------------------------------------------------------------- minibatches
    def gather(self, epoch: int, first: int, count: int, normalize: bool = True) -> RolloutSamples:
        """Samples ``first .. first + count - 1`` of epoch ``epoch``'s permutation (what ``get`` yields, one minibatch at a time).
        ``observations``: float32 [B, C, S, S], the byte / 255 (SB3's ``obs.float() / 255``, bit for bit); ``normalize=False``: the uint8
        picture."""
        A, dev = self.act_dim, self.device
        f32 = dict(dtype=torch.float32, device=dev)
        rows = max(int(count), 1)
        pix = torch.empty(rows, self.channels, self.image_size, self.image_size, dtype=torch.float32 if normalize else torch.uint8, device=dev)
        t = {"pix_f32" if normalize else "pix": pix, "action": torch.empty(rows, A, **f32), "old_value": torch.empty(rows, **f32),
             "old_log_prob": torch.empty(rows, **f32), "advantage": torch.empty(rows, **f32), "returns": torch.empty(rows, **f32),
             "index": torch.empty(rows, dtype=torch.int32, device=dev)}
        out = _abi.McgRolloutImgBatch(**{k: v.data_ptr() for k, v in t.items()})
        self._call("mcg_rollout_img_gather", C.c_uint64(self.seed), C.c_uint64(int(epoch) & (2 ** 64 - 1)), int(first), int(count), C.byref(out))
        return RolloutSamples(observations=pix, actions=t["action"], old_values=t["old_value"], old_log_prob=t["old_log_prob"],
                              advantages=t["advantage"], returns=t["returns"], index=t["index"])

    # ------------------------------------------------------------------------------------------------------- storage
    def pixels(self) -> torch.Tensor:
        """The pictures, uint8 [n_steps + 1, N, C, S, S] (a view, without the padding of a row): row t is what the action of step t
        was taken from."""
        return self._t["pixels"][:, :, :self.picture_bytes].unflatten(2, (self.channels, self.image_size, self.image_size))
