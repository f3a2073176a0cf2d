"""``SACPolicy`` -- the gradient-free half of SAC on the device: the collection action, the twin critics, the TD target of a replay
batch as one launch, and the Polyak step.

What the reference's ``scripts/train.py`` trains by default is SB3's SAC with ``MultiInputPolicy``; for the -v0 ids (a ``Dict`` space of
``Box``es) that is ``SACPolicy`` with a ``CombinedExtractor``: a squashed-Gaussian actor with a state-dependent ``log_std``, two
critics on ``cat(features, action)`` and a target copy of them.  This file owns the weights (three float32 device blobs: ``actor``,
``critic``, ``critic_target``), ``log_ent_coef``, the seed and two call numbers; the C side (``mcg_sac_*``, csrc/mcg_sac.hip) keeps no
state and no call synchronises.

    pol = SACPolicy(envs, hidden=(256, 256), activation="relu", seed=0)
    obs, _ = envs.reset(seed=0);  buf.start(obs)
    a = pol(obs)                                   # one launch
    out = envs.step(a);  buf.add(a, *out)          # HerBuffer
    batch = buf.sample(4096)
    y = pol.td_target(batch, gamma=0.99)           # one launch: actor, both target critics, min, entropy term, bootstrap
    q0, q1 = pol.q_values(batch.observations, batch.actions)
    pol.polyak(tau=0.005)

No CPU or PyTorch fallback: the kernels are the only implementation.  The gradient step is ``SACUpdate`` (sac_update.py), which
updates the three blobs and ``log_ent_coef`` in place; a caller with optimisers of its own (any ``nn.Module`` with SB3's parameter
names) can still repack the blobs with ``load_state_dict`` after an update.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence

import torch

from . import _abi, _offpolicy
from ._nets import _ACTIVATIONS, _arr, _hidden_of, check_out, names_of, pack_net, unpack_net
from ._offpolicy import OffPolicyNets, _per_row, batch_rows, critic_shapes      # noqa: F401 (_per_row and batch_rows: imported from here, as ever)

_WIDTHS = ("1 to 3 hidden layers, each width a multiple of 16 in [16, 256] (SB3's TD3 / DDPG default net_arch [400, 300] is this case: "
           "300 is no multiple of 16 and 400 is above 256)")


# ----------------------------------------------------------------------------------------------------------- the blobs
# csrc/mcg_sac.hip's head states the layouts.  actor: latent_pi's layers, the head mu, the head log_std (A rows padded to 16 each).
# critic and critic_target: qf0 then qf1, each as _nets.py's pack_net restates a critic; packing and unpacking are its functions.
def _actor_shapes(obs_dim, act_dim, pi):
    """(module, out, in, first layer?) in the actor blob's order."""
    rows, k = [], obs_dim + 6
    for L, w in enumerate(pi):
        rows.append((f"actor.latent_pi.{2 * L}", w, k, L == 0))
        k = w
    return rows + [("actor.mu", act_dim, k, False), ("actor.log_std", act_dim, k, False)]


def state_names(n_pi: int, n_qf: int):
    """The weights' keys of a state dict: actor, critic, critic_target, in the blobs' order."""
    return names_of(_actor_shapes(1, 1, [16] * n_pi) + critic_shapes(1, 1, [16] * n_qf, "critic") + critic_shapes(1, 1, [16] * n_qf, "critic_target"))


def pack_actor(sd: dict, obs_dim: int, act_dim: int, pi: Sequence[int], device=None) -> torch.Tensor:
    """The ``actor.*`` entries of a state dict under SB3's names -> the actor blob (float32), with plain torch ops."""
    return pack_net(sd, _actor_shapes(obs_dim, act_dim, pi), device=device)


def pack_critic(sd: dict, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", device=None) -> torch.Tensor:
    """The ``critic.*`` (or ``critic_target.*``) entries -> that blob."""
    return _offpolicy.pack_critic(sd, obs_dim, act_dim, qf, prefix, 2, device)


def unpack_actor(blob: torch.Tensor, obs_dim: int, act_dim: int, pi: Sequence[int]) -> dict:
    """The inverse of ``pack_actor``, bit for bit."""
    return unpack_net(blob, _actor_shapes(obs_dim, act_dim, pi))


def unpack_critic(blob: torch.Tensor, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic") -> dict:
    """The inverse of ``pack_critic``, bit for bit."""
    return _offpolicy.unpack_critic(blob, obs_dim, act_dim, qf, prefix, 2)


def _refuse_foreign(keys):
    """Names an unsupported SB3 configuration by the keys its state dict carries."""
    keys = list(keys)
    if any("cnn" in k.lower() for k in keys):
        raise ValueError("a CNN features extractor is not supported: SACPolicy serves the -v0 state ids (a Dict of Boxes)")
    if any("features_extractor." in k for k in keys):
        raise ValueError("a features extractor with parameters is not supported: the features are the concatenated observation keys")
    if any(k.startswith(("critic.qf2.", "critic_target.qf2.")) for k in keys) or not any(k.startswith("critic.qf1.") for k in keys):
        raise ValueError("n_critics != 2 is not supported: the kernels evaluate the twin critics qf0 and qf1")
    if any(k.startswith("actor.") and ("sde" in k or k == "actor.log_std") for k in keys):
        raise ValueError("gSDE (use_sde=True) is not supported: log_std is the state-dependent head actor.log_std.{weight,bias}")


class SACPolicy(OffPolicyNets):
    _NO_IMAGES = ("the -v1 image ids (and a FrameStack around them) observe uint8 pictures, which SB3 gives a CNN extractor: SACPolicy is "
                  "the MLP policy of the -v0 state ids; CNN critics are not supported")
    _WIDTHS = _WIDTHS
    _refuse_foreign = staticmethod(_refuse_foreign)
    n_critics = 2

    def __init__(self, envs=None, hidden=(256, 256), activation: str = "relu", seed: int = 0, *, n_critics: int = 2, use_sde: bool = False,
                 num_envs: Optional[int] = None, obs_dim: Optional[int] = None, act_dim: Optional[int] = None, device=None,
                 env_id_offset: Optional[int] = None):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions, the device and ``env_id_offset`` from; or give them by keyword.
        ``hidden``: the widths of the actor's trunk and of each critic (SB3's ``net_arch``, default [256, 256]), or
        ``dict(pi=[...], qf=[...])``: 1 to 3 layers, multiples of 16 up to 256.  The weights start as PyTorch initialises an
        ``nn.Linear`` (uniform within 1 / sqrt(fan_in), weights and biases: SB3's SAC does not re-initialise them), from ``seed``;
        ``critic_target`` starts as a copy of ``critic`` and ``log_ent_coef`` as ln 1 = 0."""
        if use_sde:
            raise ValueError("gSDE (use_sde=True) is not supported: the noise is the squashed Gaussian's, drawn per call")
        if int(n_critics) != 2:
            raise ValueError(f"n_critics != 2 is not supported (got {n_critics}): the kernels evaluate the twin critics qf0 and qf1")
        self._setup(envs, hidden, activation, seed, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim), device, env_id_offset,
                    ("actor", "critic", "critic_target"))
        self._t["log_ent_coef"] = torch.zeros(1, dtype=torch.float32, device=self.device)
        self._cbuf = _abi.McgSac(actor=self._t["actor"].data_ptr(), critic=self._t["critic"].data_ptr(),
                                 critic_target=self._t["critic_target"].data_ptr(), n_envs=self.num_envs, obs_dim=self.obs_dim,
                                 act_dim=self.act_dim, n_pi=len(self.pi), pi_width=_arr(self.pi), n_qf=len(self.qf), qf_width=_arr(self.qf),
                                 activation=_ACTIVATIONS[activation], actor_floats=self.actor_floats, critic_floats=self.critic_floats)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _nets(self):
        D, A = self.obs_dim, self.act_dim
        return (("actor", _actor_shapes(D, A, self.pi), 0), ("critic", critic_shapes(D, A, self.qf, "critic"), A),
                ("critic_target", critic_shapes(D, A, self.qf, "critic_target"), A))

    def _blob_floats(self):
        return self._floats_of("mcg_sac_blob_floats")

    def _fit(self):
        return f"actor {self.pi} / critics {self.qf}"

    @property
    def log_ent_coef(self) -> torch.Tensor:
        """float32 [1] on the device: SB3's ``ent_coef="auto"`` parameter; ``td_target`` reads it there."""
        return self._t["log_ent_coef"]

    @classmethod
    def from_module(cls, module, envs=None, activation: Optional[str] = None, seed: int = 0, **dims):
        """From any ``nn.Module`` whose ``state_dict()`` carries SB3's names (an SB3 ``SACPolicy`` / ``MultiInputPolicy``'s does).  The
        widths come from the weights' shapes; the activation from ``module.activation_fn`` where it has one (SB3), else ``activation``
        (default relu).  gSDE, ``n_critics != 2``, a CNN extractor and a features extractor with parameters are refused."""
        if getattr(module, "use_sde", False) or getattr(getattr(module, "actor", None), "use_sde", False):
            raise ValueError("gSDE (use_sde=True) is not supported: the noise is the squashed Gaussian's, drawn per call")
        n_critics = getattr(getattr(module, "critic", None), "n_critics", 2)
        if int(n_critics) != 2:
            raise ValueError(f"n_critics != 2 is not supported (got {n_critics}): the kernels evaluate the twin critics qf0 and qf1")
        sd = {k: v for k, v in module.state_dict().items()}
        _refuse_foreign(sd)
        pi, qf = _hidden_of(sd, "actor.latent_pi"), _hidden_of(sd, "critic.qf0")[:-1]
        if not pi or not qf:
            raise ValueError("the module's state dict has no actor.latent_pi / critic.qf0 layers")
        pol = cls(envs, hidden=dict(pi=pi, qf=qf), activation=cls._activation_of(module, activation, "relu"), seed=seed, **dims)
        pol.load_state_dict(sd)
        return pol

    # ---------------------------------------------------------------------------------------------------- collection
    def _act_shapes(self) -> dict:
        N, A = self.num_envs, self.act_dim
        return {"action": (N, A), "log_prob": (N,), "mean": (N, A), "log_std": (N, A), "noise": (N, A)}

    def _new(self, *names):
        f32 = dict(dtype=torch.float32, device=self.device)
        shape = self._act_shapes()
        return {k: torch.empty(shape[k], **f32) for k in names}

    def forward(self, obs, deterministic: bool = False, out: Optional[dict] = None) -> torch.Tensor:
        """``obs``: what ``envs.reset`` / ``envs.step`` returned (float64 device tensors, read in place) -> action float32 [N, A] in
        [-1, 1]; one launch.  ``deterministic``: tanh of the mean, and no call number is used up.  ``out``: the tensors to write into,
        under ``mcg_sac_act_out``'s names (action, and any of log_prob, mean, log_std, noise)."""
        out = self._new("action") if out is None else check_out(out, self._act_shapes(), "action", "forward", self.device)
        o, ag, dg = self._goal_obs(obs, "obs")
        cobs = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        cout = _abi.McgSacActOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_sac_act", C.byref(cobs), C.c_uint64(self.seed), C.c_uint64(self.calls), C.c_int64(self.env_id_offset),
                   int(bool(deterministic)), C.byref(cout))
        if not deterministic:
            self.calls += 1
        return out["action"]

    __call__ = forward

    # --------------------------------------------------------------------------------------------------- on a batch
    def q_values(self, observations, actions, target: bool = False, out: Optional[torch.Tensor] = None):
        """Both critics on a batch: ``observations`` the dict of float32 device tensors [B, .] that ``HerBuffer.sample`` yields,
        ``actions`` float32 [B, A] -> (q0 [B], q1 [B]), two rows of one float32 [2, B] tensor (``out``); one launch.
        ``target``: the target critics."""
        return self._q_values("mcg_sac_q", _abi.SAC_CRITIC_TARGET if target else _abi.SAC_CRITIC, observations, actions, out)

    def td_target(self, batch, gamma: float = 0.99, ent_coef: Optional[float] = None, out: Optional[dict] = None) -> torch.Tensor:
        """SB3's target line on a replay batch (``HerBuffer.sample``'s ``HerSamples``, or anything with its ``next_observations``,
        ``rewards`` and ``dones``) -> target float32 [B]; one launch, and one call number of the batch noise.  ``ent_coef``: alpha
        given on the host; None: ``exp(log_ent_coef)``, read on the device.  ``out``: the tensors to write into, under
        ``mcg_sac_target_out``'s names (target, and any of next_action [B, A], next_log_prob [B], next_q [2, B], noise [B, A])."""
        B, cb, _keep, out = self._her_batch(batch, out, "td_target")
        cout = _abi.McgSacTargetOut(**{k: v.data_ptr() for k, v in out.items()})
        lec = None if ent_coef is not None else C.c_void_p(self._t["log_ent_coef"].data_ptr())
        self._call("mcg_sac_target", C.byref(cb), C.c_int64(B), C.c_uint64(self.seed), C.c_uint64(self.target_calls), C.c_float(gamma),
                   C.c_float(0.0 if ent_coef is None else ent_coef), lec, C.byref(cout))
        self.target_calls += 1
        return out["target"]

    def _target_shapes(self, B: int) -> dict:
        return {"target": (B,), "next_log_prob": (B,), "next_q": (2, B), "next_action": (B, self.act_dim), "noise": (B, self.act_dim)}

    def polyak(self, tau: float = 0.005):
        """``critic_target <- (1 - tau) critic_target + tau critic`` over the blob (SB3's ``polyak_update``); one launch."""
        self._call("mcg_sac_polyak", C.c_double(tau))
