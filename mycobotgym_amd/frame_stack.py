"""``FrameStack`` -- SB3's ``VecFrameStack`` for the ``-v1`` picture ids, on the GPU: the policy sees the newest ``k`` pictures as
``k * C`` channels, and after a reset the frames from before the episode are zeros.

One picture shows where the arm is, not how it moves; the reference's recipes for picture observations stack frames for that
(``VecFrameStack(env, n_stack=k)``, channels first: ``StackedObservations``).  The wrapper keeps the stack on the device and updates it
with one launch per step (``mcg_frame_stack_push``): the shift, the zeroing where an episode ended, the new picture, and the stacked
``final_observation`` in one pass.

    fs = FrameStack(make("MyCobotReach-Dense-joint-v1", num_envs=8192), 4)
    buf = ImageReplayBuffer(fs, capacity=1000)        # stores single frames; sample() rebuilds the stacks
    stack, _ = fs.reset(seed=0);  buf.start(stack)
    out = fs.step(a);             buf.add(a, *out)

Slot ``s`` of a stack is channels ``s * C .. s * C + C - 1``; slot ``k - 1`` is the newest.  No CPU or PyTorch fallback: the kernel is
the only implementation.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import _abi
from ._devbuf import _ptr
from .spaces import Box, batch_box
from .vec_env import MyCobotImgVecEnv


def _strides(t: torch.Tensor, name: str):
    """uint8 [N, C, S, S] whose [S, S] planes are contiguous -> (the tensor, its environment and channel strides in bytes)."""
    if t.dtype != torch.uint8:
        raise ValueError(f"{name}: expected uint8 pictures, got {t.dtype}")
    if not t[0, 0].is_contiguous() or (t.shape[1] > 1 and t.stride(1) < t.shape[2] * t.shape[3]):
        t = t.contiguous()
    return t, t.stride(0), t.stride(1)


class FrameStack:
    def __init__(self, envs: MyCobotImgVecEnv, k: int):
        """``envs``: a ``MyCobotImgVecEnv``; ``k``: frames per stack, 1 .. 8.  Everything the wrapper does not define (``num_envs``,
        ``device``, ``action_dim``, ``max_episode_steps``, ``image_size``, ``render``, ``get_state``, ...) is the wrapped env's."""
        if not isinstance(envs, MyCobotImgVecEnv):
            raise ValueError("FrameStack wraps a MyCobotImgVecEnv (the -v1 picture ids): the -v0 ids observe states, not pictures")
        k = int(k)
        if not 1 <= k <= 8:
            raise ValueError(f"frame_stack must be in [1, 8], got {k}")
        self.envs, self.frame_stack, self.frame_channels = envs, k, envs.channels
        self.channels = k * envs.channels
        s = envs.image_size
        self.single_observation_space = Box(0, 255, (self.channels, s, s), np.uint8)
        self.observation_space = batch_box(self.single_observation_space, envs.num_envs)
        self._lib = _abi.load()
        self._stack = torch.zeros(envs.num_envs, self.channels, s, s, dtype=torch.uint8, device=envs.device)
        self._final = torch.zeros_like(self._stack)
        self._all = torch.ones(envs.num_envs, dtype=torch.uint8, device=envs.device)

    def __getattr__(self, name):          # only what the wrapper itself lacks
        if name == "envs":
            raise AttributeError(name)
        return getattr(self.envs, name)

    def _push(self, img, final_img, done, mask):
        envs = self.envs
        t, es, cs = _strides(img, "img")
        f, fes, fcs = (None, 0, 0) if final_img is None else _strides(final_img, "final_observation")
        with torch.cuda.device(envs.device):
            _abi.check(self._lib.mcg_frame_stack_push(
                _ptr(self._stack), None if f is None else _ptr(self._final), envs.num_envs, self.frame_channels, envs.image_size,
                self.frame_stack, _ptr(t), es, cs, _ptr(f), fes, fcs, _ptr(done), _ptr(mask),
                C.c_void_p(torch.cuda.current_stream(envs.device).cuda_stream)), "mcg_frame_stack_push")

    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None, mask: Optional[torch.Tensor] = None):
        """-> (stack uint8 [N, k * C, S, S], info).  The environments of ``mask`` (None: all) restart: the older slots of their stacks
        are zeros, the newest is the reset's picture; the others keep their stacks."""
        img, info = self.envs.reset(seed=seed, options=options, mask=mask)
        m = self._all if mask is None else torch.as_tensor(mask, device=self.envs.device).to(torch.uint8).contiguous()
        if tuple(m.shape) != (self.envs.num_envs,):
            raise ValueError(f"mask: expected shape {(self.envs.num_envs,)}, got {tuple(m.shape)}")
        self._push(img, None, None, m)
        return self._stack.clone(), info

    def step(self, actions, copy: bool = True):
        """-> (stack, reward, terminated, truncated, info) as the wrapped env's, the picture and ``info["final_observation"]`` stacked:
        the final stack is the old stack shifted down one slot with the finished episode's last picture in the newest slot (for every
        environment, as the env hands out ``final_observation`` for every environment); the stack is the old one shifted likewise,
        its older slots zeros where ``terminated | truncated``, with the step's picture in the newest slot.  ``copy=False`` hands
        out the wrapper's own two tensors, which the next call overwrites."""
        img, reward, terminated, truncated, info = self.envs.step(actions, copy=False)
        done = (terminated | truncated).to(torch.uint8)
        self._push(img, info["final_observation"], done, None)
        info = dict(info, final_observation=self._final.clone() if copy else self._final)
        return (self._stack.clone() if copy else self._stack), reward, terminated, truncated, info

    # ------------------------------------------------------------------------------------------------------ checkpoints
    def state_dict(self) -> dict:
        """The wrapped env's state and the stack: what a fresh ``FrameStack`` of the same shape needs to go on as this one would."""
        return {"envs": self.envs.state_dict(), "stack": self._stack.clone()}

    def load_state_dict(self, sd: dict):
        src = torch.as_tensor(sd["stack"], device=self.envs.device)
        if src.shape != self._stack.shape or src.dtype != self._stack.dtype:
            raise ValueError(f"stack: expected uint8 {tuple(self._stack.shape)}, got {src.dtype} {tuple(src.shape)}")
        self.envs.load_state_dict(sd["envs"])
        self._stack.copy_(src)
