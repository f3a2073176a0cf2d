"""``PPOUpdate`` -- the update half of PPO / A2C on an ``ActorCritic``: the loss of a minibatch, its gradient and Adam, in HIP launches.

SB3's ``PPO.train`` / ``A2C.train`` on one minibatch of the rollout buffer: ``evaluate_actions``, the clipped surrogate (or A2C's
``-adv * log_prob``), the value and entropy terms, the gradient with respect to every parameter, ``clip_grad_norm_`` and
``torch.optim.Adam``'s step -- here ``mcg_policy_grad`` and ``mcg_policy_adam`` (csrc/mcg_policy_grad.hip) on the policy's blob in place,
so the next ``pol(obs)`` sees the new weights with no repack.

    pol = ActorCritic(envs, hidden=(64, 64))
    opt = PPOUpdate(pol, learning_rate=3e-4, clip_range=0.2, ent_coef=0.0, vf_coef=0.5, max_grad_norm=0.5)      # SB3's PPO defaults
    for _ in range(10):
        for mb in buf.get(4096):
            opt.step(mb)               # six launches; no PyTorch op, no synchronisation
    opt.stats                          # float32 [8] on the device: loss, policy_loss, value_loss, entropy_loss, approx_kl, clip_fraction, 0, 0

This file owns the gradient, Adam's two moments (float32 device tensors in the blob's layout), the scratch and the step count; the C
side keeps no state.  The scratch's sizing and the moments' checkpoint are _nets.py's ``Update``, shared with SAC and TD3 / DDPG: there
the moments are dicts by blob name, here ``m`` and ``v`` stay plain tensors and pass through it as one-entry dicts.  Deterministic: equal inputs give equal bits.  ``clip_range_vf`` and ``target_kl`` are not built (the second needs
a host synchronisation, which a caller can do on ``opt.stats[4]``).  A sharded job all-reduces ``opt.grad_blob`` between
``opt.compute_grad(mb)`` and ``opt.apply()``.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi
from ._devbuf import _ptr
from ._nets import Update
from .policy import blob_shapes, minibatch_rows, unpack

_LOSSES = {"ppo": _abi.LOSS_PPO, "a2c": _abi.LOSS_A2C}
_HYPER = ("learning_rate", "clip_range", "ent_coef", "vf_coef", "max_grad_norm", "normalize_advantage", "betas", "adam_eps", "loss")
STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")


def check_hyper(loss, clip_range, betas, unbuilt: dict):
    """The refusals of the constructor (no device needed)."""
    for k in unbuilt:
        if k == "clip_range_vf":
            raise ValueError("clip_range_vf is not built: the value loss is the unclipped mean((returns - value)^2)")
        if k == "target_kl":
            raise ValueError("target_kl is not built: it needs a host synchronisation per minibatch; read opt.stats[4] (approx_kl) and stop "
                             "the epoch yourself")
        raise TypeError(f"PPOUpdate: unexpected keyword {k!r}")
    if loss not in _LOSSES:
        raise ValueError(f"loss must be one of {sorted(_LOSSES)}, got {loss!r}")
    if loss == "ppo" and not float(clip_range) > 0.0:
        raise ValueError(f"clip_range must be > 0 for loss='ppo', got {clip_range!r}")
    if len(betas) != 2 or not all(0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"betas must be two numbers in [0, 1), got {betas!r}")


def check_minibatch(mb, obs_dim: int, act_dim: int, need_old: bool, who: str = "PPOUpdate") -> int:
    """A ``RolloutSamples`` of ``RolloutBuffer`` -> its rows B (no device needed); refuses the picture buffers' samples."""
    for k in ("observations", "actions", "old_log_prob", "advantages", "returns"):
        if not hasattr(mb, k):
            raise ValueError(f"{who}: the minibatch has no field {k!r}: pass what RolloutBuffer.get yields (a RolloutSamples)")
    B = minibatch_rows(mb.observations, mb.actions, obs_dim, act_dim, who)
    for k in ("advantages", "returns") + (("old_log_prob",) if need_old else ()):
        x = getattr(mb, k)
        if not torch.is_tensor(x) or x.dtype != torch.float32 or tuple(x.shape) != (B,):
            raise ValueError(f"{who}: {k}: expected a float32 tensor of shape {(B,)}, got {getattr(x, 'dtype', type(x).__name__)} "
                             f"{tuple(getattr(x, 'shape', ()))}")
    return B


class PPOUpdate(Update):
    _WORK_ENTRY, _NOUN = "mcg_policy_grad_work_floats", "minibatch"

    def __init__(self, policy, learning_rate: float = 3e-4, clip_range: float = 0.2, ent_coef: float = 0.0, vf_coef: float = 0.5,
                 max_grad_norm: float = 0.5, normalize_advantage: bool = True, betas=(0.9, 0.999), adam_eps: float = 1e-5,
                 loss: str = "ppo", **unbuilt):
        """``policy``: the ``ActorCritic`` whose blob is updated in place.  The defaults are SB3's PPO's; ``loss="a2c"`` gives A2C's
        policy term (SB3's A2C uses RMSprop by default: here the optimiser is Adam for both).  ``max_grad_norm <= 0``: no clipping.
        ``learning_rate`` and ``clip_range`` may be set between steps; schedules are the caller's."""
        check_hyper(loss, clip_range, betas, unbuilt)
        self.policy = policy
        self.learning_rate, self.clip_range, self.ent_coef, self.vf_coef = float(learning_rate), float(clip_range), float(ent_coef), float(vf_coef)
        self.max_grad_norm, self.normalize_advantage = float(max_grad_norm), bool(normalize_advantage)
        self.betas, self.adam_eps, self.loss = (float(betas[0]), float(betas[1])), float(adam_eps), loss
        self.steps = 0                   # Adam steps taken so far
        f32 = dict(dtype=torch.float32, device=policy.device)
        n = policy.blob_floats
        self.grad_blob, self.m, self.v = torch.zeros(n, **f32), torch.zeros(n, **f32), torch.zeros(n, **f32)
        self.stats, self.grad_norm = torch.zeros(8, **f32), torch.zeros(1, **f32)
        self._work = None                # sized for the largest B seen

    # --------------------------------------------------------------------------------------------------------- calls
    def compute_grad(self, mb) -> torch.Tensor:
        """The loss of ``mb`` (a ``RolloutSamples`` of ``RolloutBuffer``) and its gradient -> ``grad_blob`` (float32 [blob_floats], in
        the blob's layout; padding positions are 0); ``stats`` is written too.  Four launches."""
        pol = self.policy
        if self.loss == "ppo" and not self.clip_range > 0.0:
            raise ValueError(f"clip_range must be > 0 for loss='ppo', got {self.clip_range!r}")
        B = check_minibatch(mb, pol.obs_dim, pol.act_dim, self.loss == "ppo")
        more = dict(advantage=mb.advantages, returns=mb.returns)
        if self.loss == "ppo":
            more["old_log_prob"] = mb.old_log_prob
        batch, B, _keep = pol._minibatch(mb.observations, mb.actions, "PPOUpdate", **more)
        hyper = _abi.McgPolicyHyper(loss_kind=_LOSSES[self.loss], normalize_advantage=int(self.normalize_advantage),
                                    clip_range=self.clip_range, ent_coef=self.ent_coef, vf_coef=self.vf_coef)
        work = self._work_for(B)
        pol._call("mcg_policy_grad", C.byref(batch), C.c_int64(B), C.byref(hyper), _ptr(work), C.c_int64(work.numel()),
                  _ptr(self.grad_blob), _ptr(self.stats))
        return self.grad_blob

    def apply(self):
        """Clip ``grad_blob`` by its global norm (written to ``grad_norm``) and take one Adam step on the policy's blob.  Two launches.
        (A sharded job all-reduces ``grad_blob`` before this.)"""
        self.steps += 1
        self.policy._call("mcg_policy_adam", _ptr(self.grad_blob), _ptr(self.m), _ptr(self.v), C.c_int64(self.steps),
                          C.c_double(self.learning_rate), C.c_double(self.betas[0]), C.c_double(self.betas[1]), C.c_double(self.adam_eps),
                          C.c_double(self.max_grad_norm), _ptr(self.grad_norm))

    def step(self, mb):
        """One update on one minibatch: ``compute_grad`` then ``apply``.  No PyTorch op and no synchronisation (the scratch is
        allocated when a larger B than any before arrives)."""
        self.compute_grad(mb)
        self.apply()

    def grad(self, mb) -> dict:
        """The gradient of ``mb``'s loss under SB3's parameter names (``unpack`` of ``grad_blob``): for tests and for callers with an
        optimiser of their own."""
        pol = self.policy
        return unpack(self.compute_grad(mb), pol.obs_dim, pol.act_dim, pol.pi, pol.vf)

    # --------------------------------------------------------------------------------------------------- checkpoints
    def _nets(self):
        pol = self.policy
        return {"blob": (blob_shapes(pol.obs_dim, pol.act_dim, pol.pi, pol.vf), 0)}

    def _moments(self):
        return {"blob": self.m}, {"blob": self.v}, "{}"

    def state_dict(self) -> dict:
        """Adam's moments as blobs (``m``, ``v``) and under SB3's names (``exp_avg``, ``exp_avg_sq``), ``step`` and the
        hyper-parameters.  With the policy's and the buffer's state dicts, training continues bit for bit."""
        sd = self._moments_state()
        sd.update({k: sd[k]["blob"] for k in ("m", "v")})
        sd.update({k: getattr(self, k) for k in _HYPER})
        return sd

    def load_state_dict(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``."""
        self._load_moments({**sd, **{k: {"blob": sd[k]} for k in ("m", "v") if k in sd}})
        hyper = {k: sd[k] for k in _HYPER if k in sd}
        check_hyper(hyper.get("loss", self.loss), hyper.get("clip_range", self.clip_range), hyper.get("betas", self.betas), {})
        for k, x in hyper.items():
            setattr(self, k, (float(x[0]), float(x[1])) if k == "betas" else x)
