"""``TD3Policy`` and ``DDPGPolicy`` -- the gradient-free half of TD3 and DDPG on the device: the collection action, the critics, the
smoothed TD target of a replay batch as one launch, and the Polyak step of both target pairs.

The reference's ``scripts/train.py`` offers ``--algo TD3`` and ``--algo DDPG`` with ``MultiInputPolicy``; for the -v0 ids (a ``Dict``
space of ``Box``es) that is SB3's ``TD3Policy`` with a ``CombinedExtractor``: a deterministic actor ``actor.mu`` (Linear, activation,
.., Linear(A), Tanh) with a target copy, and ``n_critics`` critics on ``cat(features, action)`` with a target copy -- two for TD3, one
for DDPG.  This file owns the weights (four float32 device blobs: ``actor``, ``actor_target``, ``critic``, ``critic_target``), the
seed and two call numbers; the C side (``mcg_td3_*``, csrc/mcg_td3.hip) keeps no state and no call synchronises.

    pol = TD3Policy(envs, hidden=(256, 256), activation="relu", seed=0)        # DDPGPolicy: the same with n_critics=1
    obs, _ = envs.reset(seed=0);  buf.start(obs)
    a = pol(obs, noise_std=0.1)                    # one launch: clamp(actor(obs) + noise_std eps, -1, 1)
    out = envs.step(a);  buf.add(a, *out)          # HerBuffer
    batch = buf.sample(4096)
    y = pol.td_target(batch, gamma=0.99, target_policy_noise=0.2, target_noise_clip=0.5)
    q0, q1 = pol.q_values(batch.observations, batch.actions)
    pol.polyak(tau=0.005)

No CPU or PyTorch fallback: the kernels are the only implementation.  The gradient step is ``TD3Update`` / ``DDPGUpdate``
(td3_update.py).  Not built: widths above 256 or no multiple of 16 (SB3's own default ``net_arch=[400, 300]`` for TD3 / DDPG is such a
shape and is refused by name), ``n_critics`` > 2, gSDE, CNN critics for the -v1 picture ids, Ornstein-Uhlenbeck or any other
``action_noise`` object (the collection noise is ``NormalActionNoise`` with mean 0, given as ``noise_std``).
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import _abi
from ._nets import _ACTIVATIONS, _arr, _hidden_of, check_out, names_of, pack_net, unpack_net
from ._offpolicy import OffPolicyNets, critic_shapes, pack_critic, unpack_critic      # noqa: F401 (pack_critic and unpack_critic: imported from here, as ever)

_WIDTHS = ("1 to 3 hidden layers, each width a multiple of 16 in [16, 256]; SB3's default net_arch [400, 300] for TD3 / DDPG is refused: "
           "300 is no multiple of 16 and 400 is above 256 -- pass net_arch=[256, 256] to SB3 and hidden=(256, 256) here")


# ----------------------------------------------------------------------------------------------------------- the blobs
# csrc/mcg_td3.hip's head states the layouts.  actor and actor_target: the trunk's layers, then the head (A rows padded to 16).
# critic and critic_target: qf0, then qf1 with two critics, each as _nets.py's pack_net restates a critic.
def _actor_shapes(obs_dim, act_dim, pi, prefix="actor"):
    """(module, out, in, first layer?) in the actor blob's order."""
    rows, k = [], obs_dim + 6
    for L, w in enumerate(pi):
        rows.append((f"{prefix}.mu.{2 * L}", w, k, L == 0))
        k = w
    return rows + [(f"{prefix}.mu.{2 * len(pi)}", act_dim, k, False)]


def state_names(n_pi: int, n_qf: int, n_critics: int = 2):
    """The weights' keys of a state dict: actor, actor_target, critic, critic_target, in the blobs' order."""
    return names_of(_actor_shapes(1, 1, [16] * n_pi) + _actor_shapes(1, 1, [16] * n_pi, "actor_target")
                    + critic_shapes(1, 1, [16] * n_qf, "critic", n_critics) + critic_shapes(1, 1, [16] * n_qf, "critic_target", n_critics))


def pack_actor(sd: dict, obs_dim: int, act_dim: int, pi: Sequence[int], prefix: str = "actor", device=None) -> torch.Tensor:
    """The ``actor.mu.*`` (or ``actor_target.mu.*``) entries of a state dict under SB3's names -> that blob (float32)."""
    return pack_net(sd, _actor_shapes(obs_dim, act_dim, pi, prefix), device=device)


def unpack_actor(blob: torch.Tensor, obs_dim: int, act_dim: int, pi: Sequence[int], prefix: str = "actor") -> dict:
    """The inverse of ``pack_actor``, bit for bit."""
    return unpack_net(blob, _actor_shapes(obs_dim, act_dim, pi, prefix))


def _refuse_foreign(keys):
    """Names an unsupported SB3 configuration by the keys its state dict carries."""
    keys = list(keys)
    if any("cnn" in k.lower() for k in keys):
        raise ValueError("a CNN features extractor is not supported: TD3Policy serves the -v0 state ids (a Dict of Boxes)")
    if any("features_extractor." in k for k in keys):
        raise ValueError("a features extractor with parameters is not supported: the features are the concatenated observation keys")
    if any(k.startswith(("critic.qf2.", "critic_target.qf2.")) for k in keys):
        raise ValueError("n_critics > 2 is not supported: the kernels evaluate qf0, or qf0 and qf1")
    if any(k.startswith("actor.") and ("sde" in k or "log_std" in k) for k in keys):
        raise ValueError("gSDE (use_sde=True) is not supported: TD3's and DDPG's actor is deterministic")


def _refuse_widths(widths):
    if list(widths) == [400, 300]:
        raise ValueError("net_arch [400, 300] (SB3's default for TD3 / DDPG) is not supported: " + _WIDTHS)


class TD3Policy(OffPolicyNets):
    _NO_IMAGES = ("the -v1 image ids (and a FrameStack around them) observe uint8 pictures, which SB3 gives a CNN extractor: TD3Policy is "
                  "the MLP policy of the -v0 state ids; CNN critics are not supported")
    _N_CRITICS = 2
    _WIDTHS = _WIDTHS
    _refuse_foreign, _refuse_widths = staticmethod(_refuse_foreign), staticmethod(_refuse_widths)

    def __init__(self, envs=None, hidden=(256, 256), activation: str = "relu", seed: int = 0, n_critics: Optional[int] = None, *,
                 use_sde: bool = False, num_envs: Optional[int] = None, obs_dim: Optional[int] = None, act_dim: Optional[int] = None,
                 device=None, env_id_offset: Optional[int] = None):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions, the device and ``env_id_offset`` from; or give them by keyword.
        ``hidden``: the widths of the actor's trunk and of each critic (SB3's ``net_arch``), or ``dict(pi=[...], qf=[...])``: 1 to 3
        layers, multiples of 16 up to 256.  ``n_critics``: 2 (TD3's default) or 1 (DDPG's).  The weights start as PyTorch initialises
        an ``nn.Linear``, from ``seed``; both targets start as copies."""
        if use_sde:
            raise ValueError("gSDE (use_sde=True) is not supported: TD3's and DDPG's actor is deterministic")
        n_critics = self._N_CRITICS if n_critics is None else n_critics
        if isinstance(n_critics, bool) or int(n_critics) != n_critics or int(n_critics) not in (1, 2):
            raise ValueError(f"n_critics must be 1 or 2 (got {n_critics}): n_critics > 2 is not supported, the kernels evaluate qf0, or qf0 and qf1")
        self.n_critics = int(n_critics)
        self._setup(envs, hidden, activation, seed, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim), device, env_id_offset,
                    ("actor", "actor_target", "critic", "critic_target"))
        self._cbuf = _abi.McgTd3(**{k: t.data_ptr() for k, t in self._t.items()}, n_envs=self.num_envs, obs_dim=self.obs_dim,
                                 act_dim=self.act_dim, n_pi=len(self.pi), pi_width=_arr(self.pi), n_qf=len(self.qf), qf_width=_arr(self.qf),
                                 activation=_ACTIVATIONS[activation], n_critics=self.n_critics, actor_floats=self.actor_floats,
                                 critic_floats=self.critic_floats)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _nets(self):
        D, A, nc = self.obs_dim, self.act_dim, self.n_critics
        return (("actor", _actor_shapes(D, A, self.pi), 0), ("actor_target", _actor_shapes(D, A, self.pi, "actor_target"), 0),
                ("critic", critic_shapes(D, A, self.qf, "critic", nc), A), ("critic_target", critic_shapes(D, A, self.qf, "critic_target", nc), A))

    def _blob_floats(self):
        return self._floats_of("mcg_td3_blob_floats", self.n_critics)

    def _fit(self):
        return f"actor {self.pi} / {self.n_critics} critic(s) {self.qf}"

    @classmethod
    def from_module(cls, module, envs=None, activation: Optional[str] = None, seed: int = 0, **dims):
        """From any ``nn.Module`` whose ``state_dict()`` carries SB3's names (an SB3 ``TD3Policy`` / ``MultiInputPolicy``'s does).  The
        widths come from the weights' shapes, ``n_critics`` from the presence of ``critic.qf1.*``, the activation from
        ``module.activation_fn`` where it has one (SB3), else ``activation`` (default relu)."""
        if getattr(module, "use_sde", False) or getattr(getattr(module, "actor", None), "use_sde", False):
            raise ValueError("gSDE (use_sde=True) is not supported: TD3's and DDPG's actor is deterministic")
        sd = {k: v for k, v in module.state_dict().items()}
        _refuse_foreign(sd)
        pi, qf = _hidden_of(sd, "actor.mu")[:-1], _hidden_of(sd, "critic.qf0")[:-1]
        if not pi or not qf:
            raise ValueError("the module's state dict has no actor.mu / critic.qf0 layers")
        n_critics = 2 if any(k.startswith("critic.qf1.") for k in sd) else 1
        pol = cls(envs, hidden=dict(pi=pi, qf=qf), activation=cls._activation_of(module, activation, "relu"), seed=seed, n_critics=n_critics, **dims)
        pol.load_state_dict(sd)
        return pol

    # ---------------------------------------------------------------------------------------------------- collection
    def _act_shapes(self) -> dict:
        N, A = self.num_envs, self.act_dim
        return {"action": (N, A), "mean": (N, A), "noise": (N, A)}

    def forward(self, obs, noise_std: float = 0.0, out: Optional[dict] = None) -> torch.Tensor:
        """``obs``: what ``envs.reset`` / ``envs.step`` returned (float64 device tensors, read in place) -> action float32 [N, A],
        ``clamp(actor(obs) + noise_std eps, -1, 1)``; one launch, and one call number whatever ``noise_std``.  ``noise_std``: a
        float >= 0, ``NormalActionNoise``'s sigma with mean 0 (an ``action_noise`` object is not supported).  ``out``: the tensors to
        write into, under ``mcg_td3_act_out``'s names (action, and any of mean, noise)."""
        if not isinstance(noise_std, (int, float)) or isinstance(noise_std, bool):
            raise ValueError(f"noise_std must be a float (NormalActionNoise's sigma, mean 0): an action_noise object such as "
                             f"OrnsteinUhlenbeckActionNoise is not supported, got {type(noise_std).__name__}")
        if not (math.isfinite(noise_std) and noise_std >= 0.0):
            raise ValueError(f"noise_std must be finite and >= 0, got {noise_std!r}")
        f32 = dict(dtype=torch.float32, device=self.device)
        shapes = self._act_shapes()
        out = {"action": torch.empty(shapes["action"], **f32)} if out is None else check_out(out, shapes, "action", "forward", self.device)
        o, ag, dg = self._goal_obs(obs, "obs")
        cobs = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        cout = _abi.McgTd3ActOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_td3_act", C.byref(cobs), C.c_uint64(self.seed), C.c_uint64(self.calls), C.c_int64(self.env_id_offset),
                   C.c_float(noise_std), C.byref(cout))
        self.calls += 1
        return out["action"]

    __call__ = forward

    # --------------------------------------------------------------------------------------------------- on a batch
    def q_values(self, observations, actions, target: bool = False, out: Optional[torch.Tensor] = None):
        """The critic(s) on a batch: ``observations`` the dict of float32 device tensors [B, .] that ``HerBuffer.sample`` yields,
        ``actions`` float32 [B, A] -> a tuple of ``n_critics`` rows [B] of one float32 [n_critics, B] tensor (``out``); one launch.
        ``target``: the target critics."""
        return self._q_values("mcg_td3_q", _abi.TD3_CRITIC_TARGET if target else _abi.TD3_CRITIC, observations, actions, out)

    def td_target(self, batch, gamma: float = 0.99, target_policy_noise: float = 0.2, target_noise_clip: float = 0.5,
                  out: Optional[dict] = None) -> torch.Tensor:
        """SB3's smoothed target on a replay batch (``HerBuffer.sample``'s ``HerSamples``, or anything with its ``next_observations``,
        ``rewards`` and ``dones``) -> target float32 [B]; one launch, and one call number of the smoothing noise whatever the sigma.
        ``out``: the tensors to write into, under ``mcg_td3_target_out``'s names (target, and any of next_action [B, A], next_q
        [n_critics, B], noise [B, A])."""
        B, cb, _keep, out = self._her_batch(batch, out, "td_target")
        cout = _abi.McgTd3TargetOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_td3_target", C.byref(cb), C.c_int64(B), C.c_uint64(self.seed), C.c_uint64(self.target_calls), C.c_float(gamma),
                   C.c_float(target_policy_noise), C.c_float(target_noise_clip), C.byref(cout))
        self.target_calls += 1
        return out["target"]

    def _target_shapes(self, B: int) -> dict:
        return {"target": (B,), "next_q": (self.n_critics, B), "next_action": (B, self.act_dim), "noise": (B, self.act_dim)}

    def polyak(self, tau: float = 0.005):
        """``critic_target`` and ``actor_target`` step towards ``critic`` and ``actor`` by ``tau`` (SB3's ``polyak_update``, twice);
        two launches."""
        self._call("mcg_td3_polyak", C.c_double(tau))


class DDPGPolicy(TD3Policy):
    """``TD3Policy`` with DDPG's default of one critic."""
    _N_CRITICS = 1
