"""What ``HerBuffer`` (replay.py), ``RolloutBuffer`` (rollout.py) and the two buffers of pictures (rollout_img.py, replay_img.py) share: a buffer whose memory is PyTorch tensors on one AMD GPU and
whose every operation is one call of a stateless C entry that takes the buffer's struct first and the current stream last."""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi


_STEP_OUT = ("obs", "achieved_goal", "desired_goal", "reward", "terminated", "truncated", "final_obs", "final_achieved", "final_desired")


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class DeviceBuffer:
    """A subclass sets ``_FROM_ENVS`` (constructor keyword, attribute of a ``MyCobotVecEnv`` to take it from), ``_NO_IMAGES`` (why it
    refuses the -v1 image ids and a ``FrameStack`` around them; a buffer of pictures sets ``_IMAGES = True`` and ``_NO_STATES``, why it
    refuses the -v0 ids) and
    ``_HOST_STATE`` (the host fields of ``state_dict()``), fills ``self._t`` (name -> device tensor, the pointers of the struct) and
    ``self._cbuf`` (the struct), and keeps ``num_envs``, ``obs_dim`` (with ``_goal_obs``) and ``seed``."""
    _IMAGES = False

    def _resolve(self, envs, device, given: dict):
        """Sets ``device`` and loads the library -> the values of ``_FROM_ENVS``'s keywords in its order, each as ``given`` or else
        from ``envs`` (the device likewise)."""
        if envs is not None:
            from .frame_stack import FrameStack
            from .vec_env import MyCobotImgVecEnv
            if isinstance(envs, (MyCobotImgVecEnv, FrameStack)) != self._IMAGES:      # (a FrameStack's `channels` is k * C: wide storage)
                raise ValueError(self._NO_STATES if self._IMAGES else self._NO_IMAGES)
            given = {k: getattr(envs, attr) if given[k] is None else given[k] for k, attr in self._FROM_ENVS}
            device = envs.device if device is None else device
        missing = [k for k, _ in self._FROM_ENVS if given[k] is None]
        if missing:
            raise ValueError(f"{type(self).__name__} needs envs= or {', '.join(missing)}")
        self.device = torch.device("cuda:0" if device is None else device)
        if self.device.type != "cuda":
            raise _abi.McgError(f"{type(self).__name__} lives on an AMD GPU only (device='cuda:N'); there is no CPU path")
        self._lib = _abi.load()
        return [given[k] for k, _ in self._FROM_ENVS]

    # ------------------------------------------------------------------------------------------------------ plumbing
    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def _call(self, name, *args):
        with torch.cuda.device(self.device):
            _abi.check(getattr(self._lib, name)(C.byref(self._cbuf), *args, self._stream()), name)

    def _dev(self, x, dtype, shape, name):
        t = torch.as_tensor(x, device=self.device)
        if t.dtype != dtype:
            t = t.to(dtype)
        t = t.contiguous()
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{name}: expected shape {tuple(shape)}, got {tuple(t.shape)}")
        return t

    def _picture(self, img, name):
        """uint8 [N, C, S, S] whose [S, S] planes are contiguous -> (the tensor, its environment and channel strides in bytes).  The
        environment's own layout (the [N, C, S, S] view of a [C, N, S, S] buffer) and a contiguous tensor pass without a copy.  (A
        buffer of pictures: it keeps ``channels`` and ``image_size``.)"""
        t = torch.as_tensor(img, device=self.device)
        shape = (self.num_envs, self.channels, self.image_size, self.image_size)
        if t.dtype != torch.uint8:
            raise ValueError(f"{name}: expected uint8 pictures, got {t.dtype}")
        if tuple(t.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(t.shape)}")
        if not t[0, 0].is_contiguous() or (self.channels > 1 and t.stride(1) < self.image_size ** 2):
            t = t.contiguous()
        return t, t.stride(0), t.stride(1)

    def _goal_obs(self, obs, name):
        n, D = self.num_envs, self.obs_dim
        return (self._dev(obs["observation"], torch.float64, (n, D), name + "['observation']"),
                self._dev(obs["achieved_goal"], torch.float64, (n, 3), name + "['achieved_goal']"),
                self._dev(obs["desired_goal"], torch.float64, (n, 3), name + "['desired_goal']"))

    def _step_out(self, obs, reward, terminated, truncated, final=None):
        """What ``step`` returned as the C side takes it -> (``McgStepOut``, the tensors it points into: keep them until the call).
        ``final``: ``info["final_observation"]``, where the callee reads it."""
        n = self.num_envs
        keep = [*self._goal_obs(obs, "obs"),
                self._dev(reward, torch.float64, (n,), "reward"),           # (the sparse reward comes back as float32: one small cast)
                self._dev(terminated, torch.bool, (n,), "terminated"), self._dev(truncated, torch.bool, (n,), "truncated")]
        if final is not None:
            keep += self._goal_obs(final, "info['final_observation']")
        return _abi.McgStepOut(**{k: t.data_ptr() for k, t in zip(_STEP_OUT, keep)}), keep

    # ------------------------------------------------------------------------------------------- storage, checkpoints
    def records(self) -> torch.Tensor:
        """The records, uint8 [capacity or n_steps, N, record_bytes] (a view; ``_abi.her_record_dtype``, ``_abi.rollout_record_dtype``,
        ``_abi.rollout_img_record_dtype`` or ``_abi.replay_img_record_dtype`` names the fields of a record; ``ImageReplayBuffer``:
        capacity + 1 rows)."""
        return self._t["records"]

    def state_dict(self) -> dict:
        """The device tensors (cloned) and the host state: everything a new buffer of the same shape needs to go on as this one
        would, at any point between two calls."""
        sd = {k: v.clone() for k, v in self._t.items()}
        sd.update({k: getattr(self, k) for k in self._HOST_STATE})
        return sd

    def load_state_dict(self, sd: dict):
        for k, v in self._t.items():
            src = torch.as_tensor(sd[k], device=self.device)
            if src.shape != v.shape or src.dtype != v.dtype:
                raise ValueError(f"{k}: expected {v.dtype} {tuple(v.shape)}, got {src.dtype} {tuple(src.shape)}")
            v.copy_(src)
        for k in self._HOST_STATE:
            setattr(self, k, type(getattr(self, k))(sd[k]))       # int; bool for a flag
        self.seed &= 2 ** 64 - 1
