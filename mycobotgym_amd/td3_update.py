"""``TD3Update`` and ``DDPGUpdate`` -- the update half of TD3 and DDPG on a ``TD3Policy``: one gradient step of SB3's ``TD3.train`` in
HIP launches.

    pol = TD3Policy(envs, hidden=(256, 256))
    opt = TD3Update(pol, learning_rate=1e-3, gamma=0.99, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5)
    for _ in range(gradient_steps):
        opt.step(buf.sample(256))      # HerBuffer.sample's HerSamples; no PyTorch op, no synchronisation
    opt.stats                          # float32 [8] on the device: critic_loss, actor_loss, mean(q0), mean(q1), mean(q_pi), 0, 0, 0

One step is, in SB3's order (include/mcg.h restates it; each line reads what an earlier one wrote):

1. ``steps += 1``;
2. ``y = pol.td_target(batch, gamma, target_policy_noise, target_noise_clip)``: one launch, one ``target_calls``;
3. the critic loss sum_k mean((q_k - y)^2) (no 0.5), its gradient over the ``critic`` blob, Adam on it with ``steps``;
4. where ``steps % policy_delay == 0``: ``actor_steps += 1``; the actor loss -mean(qf0(obs, actor(obs))) through qf0 alone, as just
   updated, its gradient over the ``actor`` blob alone, Adam on it with ``actor_steps``; then ``pol.polyak(tau)`` on both pairs.

The blobs are updated in place, so the next ``pol(obs)`` sees the new actor with no repack.  This file owns the gradients, Adam's
moments (float32 device tensors in the blobs' layouts), the scratch and both step counts; the C side (``mcg_td3_critic_grad``,
``mcg_td3_actor_grad``, csrc/mcg_td3_grad.hip; Adam is ``mcg_sac_adam``) keeps no state.  Deterministic: equal inputs give equal bits.
No CPU or PyTorch fallback.  ``DDPGUpdate`` is the same class with DDPG's defaults (no delay, no smoothing), for a policy with one
critic.  Not built: gSDE, ``n_critics`` > 2, CNN critics for the -v1 picture ids, learning-rate schedules, ``optimizer_class``,
``action_noise`` objects (Ornstein-Uhlenbeck among them), a sharded all-reduce of the gradients.
"""
from __future__ import annotations

import ctypes as C

import torch

from . import _abi
from ._devbuf import _ptr
from ._nets import _finite
from ._offpolicy import OffPolicyUpdate, check_common_hyper, critic_shapes
from .td3_policy import _actor_shapes

_HYPER = ("learning_rate", "gamma", "tau", "policy_delay", "target_policy_noise", "target_noise_clip", "betas", "eps")
STATS = ("critic_loss", "actor_loss", "q0_mean", "q1_mean", "q_pi_mean")


def check_hyper(learning_rate, gamma, tau, policy_delay, target_policy_noise, target_noise_clip, betas, eps, unbuilt: dict, who="TD3Update"):
    """The refusals of the constructor (no device needed)."""
    check_common_hyper(learning_rate, gamma, tau, betas, eps, unbuilt, {
        "n_critics": "n_critics is the policy's: TD3Policy(n_critics=1 or 2); n_critics > 2 is not built",
        "action_noise": "an action_noise object (OrnsteinUhlenbeckActionNoise or any other) is not built: the collection noise is "
                        "NormalActionNoise with mean 0, given as pol(obs, noise_std=sigma)"},
        "TD3's and DDPG's actor is deterministic", who)
    if isinstance(policy_delay, bool) or not _finite(policy_delay) or int(policy_delay) != policy_delay or int(policy_delay) < 1:
        raise ValueError(f"policy_delay must be an integer >= 1, got {policy_delay!r}")
    for name, x in (("target_policy_noise", target_policy_noise), ("target_noise_clip", target_noise_clip)):
        if not _finite(x) or float(x) < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {x!r}")


class TD3Update(OffPolicyUpdate):
    _WORK_ENTRY, _N_ROWS = "mcg_td3_grad_work_floats", 1          # (y per row)

    def __init__(self, policy, learning_rate: float = 1e-3, gamma: float = 0.99, tau: float = 0.005, policy_delay: int = 2,
                 target_policy_noise: float = 0.2, target_noise_clip: float = 0.5, betas=(0.9, 0.999), eps: float = 1e-8, **unbuilt):
        """``policy``: the ``TD3Policy`` whose four blobs are updated in place.  The defaults are SB3's TD3's.  ``learning_rate`` may
        be set between steps; schedules are the caller's."""
        check_hyper(learning_rate, gamma, tau, policy_delay, target_policy_noise, target_noise_clip, betas, eps, unbuilt, type(self).__name__)
        if not (hasattr(policy, "_t") and all(k in policy._t for k in ("actor", "actor_target", "critic", "critic_target"))):
            raise ValueError(f"{type(self).__name__} needs a TD3Policy (or DDPGPolicy), got {type(policy).__name__}")
        self.policy = policy
        self.learning_rate, self.gamma, self.tau, self.policy_delay = float(learning_rate), float(gamma), float(tau), int(policy_delay)
        self.target_policy_noise, self.target_noise_clip = float(target_policy_noise), float(target_noise_clip)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0                   # gradient steps so far (SB3's n_updates): the critic optimiser's step count
        self.actor_steps = 0             # actor updates so far: the actor optimiser's step count
        self._allocate({"critic": policy.critic_floats, "actor": policy.actor_floats})

    def _nets(self):
        pol = self.policy
        return {"critic": (critic_shapes(pol.obs_dim, pol.act_dim, pol.qf, "critic", pol.n_critics), pol.act_dim),
                "actor": (_actor_shapes(pol.obs_dim, pol.act_dim, pol.pi), 0)}

    # --------------------------------------------------------------------------------------------------------- calls
    def _critic_grad(self, rows, y, B, work):
        self.policy._call("mcg_td3_critic_grad", C.byref(rows), _ptr(y), C.c_int64(B), _ptr(work), C.c_int64(work.numel()),
                          _ptr(self.grad_blob["critic"]), _ptr(self.stats))

    def _actor_grad(self, rows, B, work, out=None):
        cout = None if out is None else C.byref(_abi.McgTd3ActorGradOut(**{k: v.data_ptr() for k, v in out.items()}))
        self.policy._call("mcg_td3_actor_grad", C.byref(rows), C.c_int64(B), _ptr(work), C.c_int64(work.numel()), _ptr(self.grad_blob["actor"]),
                          _ptr(self.stats), cout)

    def _target(self, batch, y):
        self.policy.td_target(batch, gamma=self.gamma, target_policy_noise=self.target_policy_noise, target_noise_clip=self.target_noise_clip,
                              out={"target": y})

    def step(self, batch, out=None):
        """One gradient step on one replay batch (``HerBuffer.sample``'s ``HerSamples``), in the order the module's head states.  No
        PyTorch op and no synchronisation (the scratch is allocated when another B than before arrives).  ``out``: tensors for the
        actor loss's intermediates under ``mcg_td3_actor_grad_out``'s names (action [B, A], q_pi [B], dq_da [B, A]); written on the
        steps with an actor update."""
        pol = self.policy
        B, rows, _keep, work, y = self._inputs(batch)
        out = self._check_out(out, B)
        self.steps += 1
        self._target(batch, y)
        self._critic_grad(rows, y, B, work)
        self._adam("critic", self.steps)
        if self.steps % self.policy_delay == 0:
            self.actor_steps += 1
            self._actor_grad(rows, B, work, out)
            self._adam("actor", self.actor_steps)
            pol.polyak(self.tau)

    def grad(self, batch, out=None) -> dict:
        """Both losses' gradients on the blobs as they stand, with no optimiser step in between and whatever the delay, under SB3's
        state-dict names; ``stats`` is written too.  The call numbers and step counts are left as they were."""
        pol = self.policy
        B, rows, _keep, work, y = self._inputs(batch)
        out = self._check_out(out, B)
        calls = pol.target_calls
        self._target(batch, y)
        pol.target_calls = calls
        self._critic_grad(rows, y, B, work)
        self._actor_grad(rows, B, work, out)
        return self._named({k: self.grad_blob[k] for k in ("critic", "actor")})

    def _out_shapes(self, B):
        A = self.policy.act_dim
        return {"action": (B, A), "q_pi": (B,), "dq_da": (B, A)}

    # --------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """Adam's moments of both optimisers as blobs (``m``, ``v``: critic, actor) and under SB3's names (``exp_avg``,
        ``exp_avg_sq``), ``step``, ``actor_steps`` and the hyper-parameters.  With the policy's and the buffer's state dicts, training
        continues bit for bit."""
        sd = {**self._moments_state(), "actor_steps": self.actor_steps, "stats": self.stats.clone()}
        sd.update({k: getattr(self, k) for k in _HYPER})
        return sd

    def load_state_dict(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``."""
        self._load_moments(sd)
        self.actor_steps = int(sd["actor_steps"])
        if "stats" in sd:                # (actor_loss and q_pi_mean keep their last value across steps without an actor update)
            self.stats.copy_(torch.as_tensor(sd["stats"], device=self.policy.device))
        hyper = {k: sd.get(k, getattr(self, k)) for k in _HYPER}
        check_hyper(unbuilt={}, **hyper)
        for k, x in hyper.items():
            setattr(self, k, (float(x[0]), float(x[1])) if k == "betas" else (int(x) if k == "policy_delay" else float(x)))


class DDPGUpdate(TD3Update):
    """``TD3Update`` with DDPG's defaults: the actor and the targets every step, and no target smoothing."""

    def __init__(self, policy, learning_rate: float = 1e-3, gamma: float = 0.99, tau: float = 0.005, policy_delay: int = 1,
                 target_policy_noise: float = 0.0, target_noise_clip: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, **unbuilt):
        super().__init__(policy, learning_rate, gamma, tau, policy_delay, target_policy_noise, target_noise_clip, betas, eps, **unbuilt)
