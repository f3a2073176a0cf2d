"""``SACUpdate`` -- the update half of SAC on an ``SACPolicy``: one gradient step of SB3's ``SAC.train`` in HIP launches.

    pol = SACPolicy(envs, hidden=(256, 256))
    opt = SACUpdate(pol, learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto")      # SB3's SAC defaults
    for _ in range(gradient_steps):
        opt.step(buf.sample(256))      # HerBuffer.sample's HerSamples; no PyTorch op, no synchronisation
    opt.stats                          # float32 [8] on the device: critic_loss, actor_loss, ent_coef_loss, ent_coef, mean(q0), mean(q1), mean(logp), 0

One step is, in SB3's order (include/mcg.h restates it; each line reads what an earlier one wrote):

1. alpha = exp(log_ent_coef) as it stands before this step's alpha update (``ent_coef="auto"``), or the constant ``ent_coef``;
2. ``y = pol.td_target(batch, gamma)``: the existing launch, one ``target_calls``;
3. the critic loss 0.5 (mean((q0 - y)^2) + mean((q1 - y)^2)), its gradient over the ``critic`` blob, Adam on it (no clipping);
4. the actor loss mean(alpha logp - min(q0, q1)(obs, a)) with a fresh draw, through the critic as just updated, its gradient over
   the ``actor`` blob alone, Adam on it;
5. ``"auto"``: the loss -mean(log_ent_coef (logp + target_entropy)) with step 4's logp, Adam on the one float;
6. ``pol.polyak(tau)`` after every ``target_update_interval``-th step (counted over this object's life, checkpoints included).

The three blobs and ``log_ent_coef`` are updated in place, so the next ``pol(obs)`` sees the new actor with no repack.  This file owns
the gradients, Adam's moments (float32 device tensors in the blobs' layouts), the scratch, the step count and the call number of the
actor-loss noise (Philox domain 9); the C side (``mcg_sac_critic_grad``, ``mcg_sac_actor_grad``, ``mcg_sac_alpha_step``,
``mcg_sac_adam``; csrc/mcg_sac_grad.hip) keeps no state.  Deterministic: equal inputs give equal bits.  No CPU or PyTorch fallback.
Not built: gSDE, ``n_critics != 2``, CNN critics for the -v1 picture ids, learning-rate schedules.  TD3 and DDPG are ``TD3Update`` / ``DDPGUpdate`` (td3_update.py).
"""
from __future__ import annotations

import ctypes as C
import math

from . import _abi
from ._devbuf import _ptr
from ._nets import _finite
from ._offpolicy import OffPolicyUpdate, check_batch, check_common_hyper, critic_shapes      # noqa: F401 (check_batch: imported from here, as ever)
from .sac_policy import _actor_shapes

_HYPER = ("learning_rate", "gamma", "tau", "ent_coef", "target_entropy", "target_update_interval", "betas", "eps")
STATS = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef", "q0_mean", "q1_mean", "log_prob_mean")


def check_hyper(learning_rate, gamma, tau, ent_coef, target_entropy, target_update_interval, betas, eps, unbuilt: dict):
    """The refusals of the constructor (no device needed) -> (auto?, the constant alpha or None, the initial alpha of "auto_x" or None)."""
    check_common_hyper(learning_rate, gamma, tau, betas, eps, unbuilt, {
        "max_grad_norm": "max_grad_norm is not built: SB3's SAC clips no gradients",
        "n_critics": "n_critics != 2 is not built: the kernels differentiate the twin critics qf0 and qf1",
        "action_noise": "action_noise is not built: SAC explores through its own entropy term"},
        "the noise is the squashed Gaussian's, drawn per call", "SACUpdate")
    if isinstance(target_update_interval, bool) or int(target_update_interval) != target_update_interval or int(target_update_interval) < 1:
        raise ValueError(f"target_update_interval must be an integer >= 1, got {target_update_interval!r}")
    if not (target_entropy == "auto" or _finite(target_entropy)):
        raise ValueError(f"target_entropy must be 'auto' (-act_dim) or a finite float, got {target_entropy!r}")
    if isinstance(ent_coef, str):
        if ent_coef == "auto":
            return True, None, None
        if ent_coef.startswith("auto_"):
            try:
                init = float(ent_coef[5:])
            except ValueError:
                init = -1.0
            if not (math.isfinite(init) and init > 0.0):
                raise ValueError(f"ent_coef: the initial value of 'auto_<x>' must be a finite float > 0, got {ent_coef!r}")
            return True, None, init
        raise ValueError(f"ent_coef must be 'auto', 'auto_<x>' or a float, got {ent_coef!r}")
    if not _finite(ent_coef) or float(ent_coef) < 0.0:
        raise ValueError(f"ent_coef must be 'auto' or a finite float >= 0 (negative or non-finite values are refused), got {ent_coef!r}")
    return False, float(ent_coef), None


class SACUpdate(OffPolicyUpdate):
    _WORK_ENTRY, _N_ROWS = "mcg_sac_grad_work_floats", 2          # (y and logp per row)

    def __init__(self, policy, learning_rate: float = 3e-4, gamma: float = 0.99, tau: float = 0.005, ent_coef="auto", target_entropy="auto",
                 target_update_interval: int = 1, betas=(0.9, 0.999), eps: float = 1e-8, **unbuilt):
        """``policy``: the ``SACPolicy`` whose blobs and ``log_ent_coef`` are updated in place.  The defaults are SB3's SAC's.
        ``ent_coef``: ``"auto"`` learns ``log_ent_coef`` from the value the policy holds; ``"auto_0.1"`` first sets it to ln 0.1, as
        SB3 does; a float keeps alpha constant, and ``log_ent_coef`` is then neither read nor stepped.  ``learning_rate`` may be set
        between steps; schedules are the caller's."""
        self.auto, self._alpha, init = check_hyper(learning_rate, gamma, tau, ent_coef, target_entropy, target_update_interval, betas, eps, unbuilt)
        if not (hasattr(policy, "_t") and all(k in policy._t for k in ("actor", "critic", "critic_target", "log_ent_coef"))):
            raise ValueError(f"SACUpdate needs an SACPolicy, got {type(policy).__name__}")
        self.policy = policy
        self.learning_rate, self.gamma, self.tau = float(learning_rate), float(gamma), float(tau)
        self.ent_coef, self.target_update_interval = ent_coef, int(target_update_interval)
        self.target_entropy = -float(policy.act_dim) if target_entropy == "auto" else float(target_entropy)
        self.betas, self.eps = (float(betas[0]), float(betas[1])), float(eps)
        self.steps = 0                   # gradient steps taken so far: Adam's step count of the three optimisers
        self.actor_calls = 0             # actor-loss draws so far: the `call` word of their noise
        self._allocate({"critic": policy.critic_floats, "actor": policy.actor_floats, "log_ent_coef": 1})
        if init is not None:
            policy.log_ent_coef.fill_(math.log(init))

    def _nets(self):
        pol = self.policy
        return {"critic": (critic_shapes(pol.obs_dim, pol.act_dim, pol.qf, "critic"), pol.act_dim),
                "actor": (_actor_shapes(pol.obs_dim, pol.act_dim, pol.pi), 0)}

    # --------------------------------------------------------------------------------------------------------- calls
    def _critic_grad(self, rows, y, B, work):
        self.policy._call("mcg_sac_critic_grad", C.byref(rows), _ptr(y), C.c_int64(B), _ptr(work), C.c_int64(work.numel()),
                          _ptr(self.grad_blob["critic"]), _ptr(self.stats))

    def _actor_grad(self, rows, logp, B, work, out=None):
        pol = self.policy
        lec = _ptr(pol.log_ent_coef) if self.auto else None
        cout = None if out is None else C.byref(_abi.McgSacActorGradOut(**{k: v.data_ptr() for k, v in out.items()}))
        pol._call("mcg_sac_actor_grad", C.byref(rows), C.c_int64(B), C.c_uint64(pol.seed), C.c_uint64(self.actor_calls),
                  C.c_float(0.0 if self.auto else self._alpha), lec, _ptr(work), C.c_int64(work.numel()), _ptr(self.grad_blob["actor"]),
                  _ptr(logp), _ptr(self.stats), cout)

    def _alpha_step(self, logp, B, lr):
        k = "log_ent_coef"
        self._bare("mcg_sac_alpha_step", _ptr(self.policy.log_ent_coef), _ptr(logp), C.c_int64(B), C.c_float(self.target_entropy), _ptr(self.m[k]),
                   _ptr(self.v[k]), C.c_int64(max(self.steps, 1)), C.c_double(lr), C.c_double(self.betas[0]), C.c_double(self.betas[1]),
                   C.c_double(self.eps), _ptr(self.grad_blob[k]), _ptr(self.stats))

    def step(self, batch, out=None):
        """One gradient step on one replay batch (``HerBuffer.sample``'s ``HerSamples``), in the order the module's head states.  No
        PyTorch op and no synchronisation (the scratch is allocated when another B than before arrives).  ``out``: tensors for the
        actor loss's intermediates under ``mcg_sac_actor_grad_out``'s names (action, noise [B, A], q_pi [2, B], dq_da [B, A])."""
        pol = self.policy
        B, rows, _keep, work, y, logp = self._inputs(batch)
        out = self._check_out(out, B)
        pol.td_target(batch, gamma=self.gamma, ent_coef=None if self.auto else self._alpha, out={"target": y})
        self.steps += 1
        self._critic_grad(rows, y, B, work)
        self._adam("critic")
        self._actor_grad(rows, logp, B, work, out)
        self.actor_calls += 1
        self._adam("actor")
        if self.auto:
            self._alpha_step(logp, B, self.learning_rate)
        if self.steps % self.target_update_interval == 0:
            pol.polyak(self.tau)

    def grad(self, batch, out=None) -> dict:
        """The three losses' gradients on the blobs as they stand, with no optimiser step in between, under SB3's state-dict names
        (plus ``log_ent_coef`` with ``"auto"``); ``stats`` is written too.  The call numbers are left as they were: a ``step`` on the
        same batch afterwards draws the same noise.  For tests and for callers with optimisers of their own."""
        pol = self.policy
        B, rows, _keep, work, y, logp = self._inputs(batch)
        out = self._check_out(out, B)
        calls = pol.target_calls
        pol.td_target(batch, gamma=self.gamma, ent_coef=None if self.auto else self._alpha, out={"target": y})
        pol.target_calls = calls
        self._critic_grad(rows, y, B, work)
        self._actor_grad(rows, logp, B, work, out)
        g = self._named({k: self.grad_blob[k] for k in ("critic", "actor")})
        if self.auto:
            self._alpha_step(logp, B, 0.0)
            g["log_ent_coef"] = self.grad_blob["log_ent_coef"].clone()
        return g

    def _out_shapes(self, B):
        A = self.policy.act_dim
        return {"action": (B, A), "noise": (B, A), "q_pi": (2, B), "dq_da": (B, A)}

    # --------------------------------------------------------------------------------------------------- checkpoints
    def state_dict(self) -> dict:
        """Adam's moments of the three optimisers as blobs (``m``, ``v``: critic, actor, log_ent_coef) and under SB3's names
        (``exp_avg``, ``exp_avg_sq``), ``step``, ``actor_calls`` and the hyper-parameters.  With the policy's and the buffer's state
        dicts, training continues bit for bit."""
        sd = {**self._moments_state(), "actor_calls": self.actor_calls}
        sd.update({k: getattr(self, k) for k in _HYPER})
        return sd

    def load_state_dict(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``."""
        self._load_moments(sd)
        self.actor_calls = int(sd["actor_calls"])
        hyper = {k: sd.get(k, getattr(self, k)) for k in _HYPER}
        self.auto, self._alpha, _ = check_hyper(unbuilt={}, **hyper)
        for k, x in hyper.items():
            setattr(self, k, (float(x[0]), float(x[1])) if k == "betas" else x)
