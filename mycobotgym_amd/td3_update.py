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
import math

import torch

from . import _abi
from ._devbuf import _ptr
from .sac_policy import check_out
from .sac_update import _finite, check_batch
from .td3_policy import pack_actor, pack_critic, unpack_actor, unpack_critic

_HYPER = ("learning_rate", "gamma", "tau", "policy_delay", "target_policy_noise", "target_noise_clip", "betas", "eps")
STATS = ("critic_loss", "actor_loss", "q0_mean", "q1_mean", "q_pi_mean")


def check_hyper(learning_rate, gamma, tau, policy_delay, target_policy_noise, target_noise_clip, betas, eps, unbuilt: dict, who="TD3Update"):
    """The refusals of the constructor (no device needed)."""
    for k in unbuilt:
        if k in ("use_sde", "sde_sample_freq", "use_sde_at_warmup"):
            if unbuilt[k] in (False, None, -1):
                continue
            raise ValueError(f"gSDE ({k}) is not built: TD3's and DDPG's actor is deterministic")
        if k == "n_critics":
            raise ValueError("n_critics is the policy's: TD3Policy(n_critics=1 or 2); n_critics > 2 is not built")
        if k in ("optimizer_class", "optimizer_kwargs"):
            raise ValueError(f"{k} is not built: the optimiser is torch.optim.Adam's rule without amsgrad or weight decay")
        if k == "action_noise":
            raise ValueError("an action_noise object (OrnsteinUhlenbeckActionNoise or any other) is not built: the collection noise is "
                             "NormalActionNoise with mean 0, given as pol(obs, noise_std=sigma)")
        raise TypeError(f"{who}: unexpected keyword {k!r}")
    if callable(learning_rate):
        raise ValueError("a learning-rate schedule is not built: learning_rate takes a float only (it may be set between steps)")
    if not _finite(learning_rate) or not float(learning_rate) > 0.0:
        raise ValueError(f"learning_rate must be a finite float > 0, got {learning_rate!r}")
    if not _finite(gamma) or not 0.0 <= float(gamma) <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
    if not _finite(tau) or not 0.0 < float(tau) <= 1.0:
        raise ValueError(f"tau must be in (0, 1], got {tau!r}")
    if isinstance(policy_delay, bool) or not _finite(policy_delay) or int(policy_delay) != policy_delay or int(policy_delay) < 1:
        raise ValueError(f"policy_delay must be an integer >= 1, got {policy_delay!r}")
    for name, x in (("target_policy_noise", target_policy_noise), ("target_noise_clip", target_noise_clip)):
        if not _finite(x) or float(x) < 0.0:
            raise ValueError(f"{name} must be finite and >= 0, got {x!r}")
    if len(betas) != 2 or not all(_finite(b) and 0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"betas must be two numbers in [0, 1), got {betas!r}")
    if not _finite(eps) or float(eps) < 0.0:
        raise ValueError(f"eps must be finite and >= 0, got {eps!r}")


class TD3Update:
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
        f32 = dict(dtype=torch.float32, device=policy.device)
        n = {"critic": policy.critic_floats, "actor": policy.actor_floats}
        self.grad_blob = {k: torch.zeros(n[k], **f32) for k in n}
        self.m, self.v = {k: torch.zeros(n[k], **f32) for k in n}, {k: torch.zeros(n[k], **f32) for k in n}
        self.stats = torch.zeros(8, **f32)
        self._work, self._rows = None, {}      # the scratch, sized for the largest B seen; y per B

    # --------------------------------------------------------------------------------------------------------- calls
    def _buffers(self, B: int):
        pol = self.policy
        need = int(pol._lib.mcg_td3_grad_work_floats(C.byref(pol._cbuf), C.c_int64(B)))
        if need == 0:
            raise ValueError(f"{type(self).__name__}: a batch of {B} rows is not supported (1 <= B < 2^27)")
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=pol.device)
        if B not in self._rows:
            self._rows = {B: torch.empty(B, dtype=torch.float32, device=pol.device)}
        return self._work, self._rows[B]

    def _critic_grad(self, rows, y, B, work):
        self.policy._call("mcg_td3_critic_grad", C.byref(rows), _ptr(y), C.c_int64(B), _ptr(work), C.c_int64(work.numel()),
                          _ptr(self.grad_blob["critic"]), _ptr(self.stats))

    def _actor_grad(self, rows, B, work, out=None):
        cout = None if out is None else C.byref(_abi.McgTd3ActorGradOut(**{k: v.data_ptr() for k, v in out.items()}))
        self.policy._call("mcg_td3_actor_grad", C.byref(rows), C.c_int64(B), _ptr(work), C.c_int64(work.numel()), _ptr(self.grad_blob["actor"]),
                          _ptr(self.stats), cout)

    def _adam(self, k, step):
        pol = self.policy
        with torch.cuda.device(pol.device):
            _abi.check(pol._lib.mcg_sac_adam(_ptr(pol._t[k]), _ptr(self.grad_blob[k]), _ptr(self.m[k]), _ptr(self.v[k]),
                                             C.c_int64(self.grad_blob[k].numel()), C.c_int64(step), C.c_double(self.learning_rate),
                                             C.c_double(self.betas[0]), C.c_double(self.betas[1]), C.c_double(self.eps), pol._stream()), "mcg_sac_adam")

    def _inputs(self, batch):
        pol = self.policy
        if not float(self.learning_rate) > 0.0 or not math.isfinite(self.learning_rate):
            raise ValueError(f"learning_rate must be a finite float > 0, got {self.learning_rate!r}")
        B = check_batch(batch, pol.obs_dim, pol.act_dim, pol.device, type(self).__name__)
        keep = [batch.observations[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [batch.actions.contiguous()]
        rows = _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)})
        return (B, rows, keep) + self._buffers(B)

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
        D, A = pol.obs_dim, pol.act_dim
        g = unpack_critic(self.grad_blob["critic"], D, A, pol.qf, "critic", pol.n_critics)
        g.update(unpack_actor(self.grad_blob["actor"], D, A, pol.pi, "actor"))
        return g

    def _check_out(self, out, B):
        if out is None:
            return None
        A = self.policy.act_dim
        shapes = {"action": (B, A), "q_pi": (B,), "dq_da": (B, A)}
        if not isinstance(out, dict) or not out:
            raise ValueError(f"{type(self).__name__}: out: a dict with any of {sorted(shapes)}")
        return check_out(out, shapes, next(iter(out)), type(self).__name__, self.policy.device)

    # --------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """Adam's moments of both optimisers as blobs (``m``, ``v``: critic, actor) and under SB3's names (``exp_avg``,
        ``exp_avg_sq``), ``step``, ``actor_steps`` and the hyper-parameters.  With the policy's and the buffer's state dicts, training
        continues bit for bit."""
        pol = self.policy
        D, A = pol.obs_dim, pol.act_dim

        def named(t):
            sd = unpack_critic(t["critic"], D, A, pol.qf, "critic", pol.n_critics)
            sd.update(unpack_actor(t["actor"], D, A, pol.pi, "actor"))
            return sd
        sd = {"m": {k: t.clone() for k, t in self.m.items()}, "v": {k: t.clone() for k, t in self.v.items()}, "exp_avg": named(self.m),
              "exp_avg_sq": named(self.v), "step": self.steps, "actor_steps": self.actor_steps, "stats": self.stats.clone()}
        sd.update({k: getattr(self, k) for k in _HYPER})
        return sd

    def load_state_dict(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``."""
        pol = self.policy
        D, A, dev = pol.obs_dim, pol.act_dim, pol.device
        for blob, mine, names in (("m", self.m, "exp_avg"), ("v", self.v, "exp_avg_sq")):
            if blob in sd:
                src = {k: torch.as_tensor(sd[blob][k], device=dev) for k in mine}
            elif names in sd:
                src = {"critic": pack_critic(sd[names], D, A, pol.qf, "critic", pol.n_critics, device=dev),
                       "actor": pack_actor(sd[names], D, A, pol.pi, "actor", device=dev)}
            else:
                raise ValueError(f"the state dict has neither {blob!r} nor {names!r}")
            for k, t in mine.items():
                if src[k].dtype != torch.float32 or tuple(src[k].shape) != tuple(t.shape):
                    raise ValueError(f"{blob}[{k!r}]: expected float32 {tuple(t.shape)}, got {src[k].dtype} {tuple(src[k].shape)}")
            for k, t in mine.items():
                t.copy_(src[k])
        self.steps, self.actor_steps = int(sd["step"]), int(sd["actor_steps"])
        if "stats" in sd:                # (actor_loss and q_pi_mean keep their last value across steps without an actor update)
            self.stats.copy_(torch.as_tensor(sd["stats"], device=dev))
        hyper = {k: sd.get(k, getattr(self, k)) for k in _HYPER}
        check_hyper(unbuilt={}, **hyper)
        for k, x in hyper.items():
            setattr(self, k, (float(x[0]), float(x[1])) if k == "betas" else (int(x) if k == "policy_delay" else float(x)))


class DDPGUpdate(TD3Update):
    """``TD3Update`` with DDPG's defaults: the actor and the targets every step, and no target smoothing."""

    def __init__(self, policy, learning_rate: float = 1e-3, gamma: float = 0.99, tau: float = 0.005, policy_delay: int = 1,
                 target_policy_noise: float = 0.0, target_noise_clip: float = 0.0, betas=(0.9, 0.999), eps: float = 1e-8, **unbuilt):
        super().__init__(policy, learning_rate, gamma, tau, policy_delay, target_policy_noise, target_noise_clip, betas, eps, **unbuilt)
