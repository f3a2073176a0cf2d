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
import math
from typing import Optional, Sequence

import torch

from . import _abi
from ._devbuf import DeviceBuffer
from .policy import _ACTIVATIONS, _pack_layer, _unpack_layer

_WIDTHS = ("1 to 3 hidden layers, each width a multiple of 16 in [16, 256] (SB3's TD3 / DDPG default net_arch [400, 300] is this case: "
           "300 is no multiple of 16 and 400 is above 256)")
_HOST = ("seed", "calls", "target_calls")


# ----------------------------------------------------------------------------------------------------------- the blobs
# csrc/mcg_sac.hip's head states the layouts; restated.  actor: latent_pi's layers, the head mu, the head log_std (A rows padded to
# 16 each).  critic and critic_target: qf0 then qf1; a first layer is its tiles over the D + 6 feature columns (first-layer order),
# its tiles over the action padded to 16 columns (later-layer order), then its bias; the later layers; a head of 1 row padded to 16.
def _actor_shapes(obs_dim, act_dim, pi):
    """(module, out, in, first layer?) in the actor blob's order."""
    rows, k = [], obs_dim + 6
    for L, w in enumerate(pi):
        rows.append((f"actor.latent_pi.{2 * L}", w, k, L == 0))
        k = w
    return rows + [("actor.mu", act_dim, k, False), ("actor.log_std", act_dim, k, False)]


def _critic_shapes(obs_dim, act_dim, qf, prefix):
    """Likewise for ``prefix`` = critic or critic_target; a first layer's `in` counts the action's columns."""
    rows = []
    for q in range(2):
        k = obs_dim + 6 + act_dim
        for L, w in enumerate(qf):
            rows.append((f"{prefix}.qf{q}.{2 * L}", w, k, L == 0))
            k = w
        rows.append((f"{prefix}.qf{q}.{2 * len(qf)}", 1, k, False))
    return rows


def state_names(n_pi: int, n_qf: int):
    """The weights' keys of a state dict: actor, critic, critic_target, in the blobs' order."""
    names = []
    for m, *_ in (_actor_shapes(1, 1, [16] * n_pi) + _critic_shapes(1, 1, [16] * n_qf, "critic")
                  + _critic_shapes(1, 1, [16] * n_qf, "critic_target")):
        names += [m + ".weight", m + ".bias"]
    return names


def _param(sd, m, out, k, device):
    W = torch.as_tensor(sd[m + ".weight"]).detach().to(device=device, dtype=torch.float32)
    b = torch.as_tensor(sd[m + ".bias"]).detach().to(device=device, dtype=torch.float32)
    if tuple(W.shape) != (out, k) or tuple(b.shape) != (out,):
        raise ValueError(f"{m}: expected weight {(out, k)} and bias {(out,)}, got {tuple(W.shape)} and {tuple(b.shape)}")
    return W, b


def pack_actor(sd: dict, obs_dim: int, act_dim: int, pi: Sequence[int], device=None) -> torch.Tensor:
    """The ``actor.*`` entries of a state dict under SB3's names -> the actor blob (float32), with plain torch ops."""
    parts = []
    for m, out, k, first in _actor_shapes(obs_dim, act_dim, pi):
        parts += _pack_layer(*_param(sd, m, out, k, device), first)
    return torch.cat(parts).contiguous()


def pack_critic(sd: dict, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", device=None) -> torch.Tensor:
    """The ``critic.*`` (or ``critic_target.*``) entries -> that blob."""
    parts, F = [], obs_dim + 6
    for m, out, k, first in _critic_shapes(obs_dim, act_dim, qf, prefix):
        W, b = _param(sd, m, out, k, device)
        if first:
            Wa = torch.zeros(out, 16, dtype=torch.float32, device=W.device)
            Wa[:, :act_dim] = W[:, F:]
            parts += [_pack_layer(W[:, :F], b, True)[0], *_pack_layer(Wa, b, False)]
        else:
            parts += _pack_layer(W, b, False)
    return torch.cat(parts).contiguous()


def unpack_actor(blob: torch.Tensor, obs_dim: int, act_dim: int, pi: Sequence[int]) -> dict:
    """The inverse of ``pack_actor``, bit for bit."""
    sd, at = {}, 0
    for m, out, k, first in _actor_shapes(obs_dim, act_dim, pi):
        sd[m + ".weight"], sd[m + ".bias"], used = _unpack_layer(blob[at:], out, k, first)
        at += used
    return sd


def unpack_critic(blob: torch.Tensor, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic") -> dict:
    """The inverse of ``pack_critic``, bit for bit."""
    sd, at, F = {}, 0, obs_dim + 6
    for m, out, k, first in _critic_shapes(obs_dim, act_dim, qf, prefix):
        if first:
            feat = out * (-(-F // 4) * 4)                                       # the feature tiles; then the action tiles and the bias
            Wf = _unpack_layer(torch.cat([blob[at:at + feat], blob.new_zeros(out)]), out, F, True)[0]
            Wa, b, used = _unpack_layer(blob[at + feat:], out, 16, False)
            sd[m + ".weight"], sd[m + ".bias"] = torch.cat([Wf, Wa[:, :act_dim]], dim=1), b
            at += feat + used
        else:
            sd[m + ".weight"], sd[m + ".bias"], used = _unpack_layer(blob[at:], out, k, False)
            at += used
    return sd


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


def _hidden_of(sd: dict, stem: str):
    """The widths of the Linear layers ``stem``.0, .2, .. (a critic's last one is its head)."""
    widths, L = [], 0
    while f"{stem}.{2 * L}.weight" in sd:
        widths.append(int(sd[f"{stem}.{2 * L}.weight"].shape[0]))
        L += 1
    return tuple(widths)


def batch_rows(observations, actions, obs_dim: int, act_dim: int, who: str, device=None) -> int:
    """Checks float32 rows as ``HerBuffer.sample`` yields them (a dict of observation / achieved_goal / desired_goal, and ``actions``
    or None) -> their number B.  Needs no device."""
    if not isinstance(observations, dict):
        raise ValueError(f"{who}: observations must be the dict of float32 tensors that HerBuffer.sample yields (observation, achieved_goal, "
                         "desired_goal); the picture buffers' samples (-v1 ids) are not supported: the networks are the MLPs of the -v0 state ids")
    missing = [k for k in ("observation", "achieved_goal", "desired_goal") if k not in observations]
    if missing:
        raise ValueError(f"{who}: observations lacks {missing}")
    B = int(observations["observation"].shape[0]) if torch.is_tensor(observations["observation"]) and observations["observation"].dim() else 0
    if B < 1:
        raise ValueError(f"{who}: the batch is empty (B must be >= 1)")
    rows = [("observations['observation']", observations["observation"], obs_dim), ("observations['achieved_goal']", observations["achieved_goal"], 3),
            ("observations['desired_goal']", observations["desired_goal"], 3)]
    if actions is not None:
        rows.append(("actions", actions, act_dim))
    for name, t, cols in rows:
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name}: expected float32, got {getattr(t, 'dtype', type(t).__name__)} (the float64 observations of "
                             "envs.step go through HerBuffer, or SACPolicy.__call__)")
        if tuple(t.shape) != (B, cols):
            raise ValueError(f"{who}: {name}: expected shape {(B, cols)}, got {tuple(t.shape)}")
        if device is not None and t.device != device:
            raise ValueError(f"{who}: {name} lives on {t.device}, the policy on {device}")
    return B


def _per_row(t, B, name, who, device):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name}: expected float32, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(t.shape) not in ((B,), (B, 1)):
        raise ValueError(f"{who}: {name}: expected shape {(B, 1)} or {(B,)}, got {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{who}: {name} lives on {t.device}, the policy on {device}")
    return t.contiguous()


def check_out(out, shapes: dict, required: str, who: str, device=None) -> dict:
    """A caller's ``out`` dict against the shapes the kernel writes: the kernel gets bare pointers, so a tensor of another dtype, shape,
    layout or device would be written out of bounds.  Needs no device."""
    if not isinstance(out, dict) or required not in out:
        raise ValueError(f"{who}: out: '{required}' is required")
    unknown = sorted(set(out) - set(shapes))
    if unknown:
        raise ValueError(f"{who}: out: unknown {unknown}; the outputs are {sorted(shapes)}")
    for k, t in out.items():
        if not torch.is_tensor(t) or t.dtype != torch.float32 or tuple(t.shape) != shapes[k] or not t.is_contiguous():
            raise ValueError(f"{who}: out[{k!r}]: expected a contiguous float32 tensor {shapes[k]}, got "
                             f"{getattr(t, 'dtype', type(t).__name__)} {tuple(getattr(t, 'shape', ()))}")
        if device is not None and t.device != device:
            raise ValueError(f"{who}: out[{k!r}] lives on {t.device}, the policy on {device}")
    return out


def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0] * 3)[:3])


class SACPolicy(DeviceBuffer):
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"))
    _NO_IMAGES = ("the -v1 image ids (and a FrameStack around them) observe uint8 pictures, which SB3 gives a CNN extractor: SACPolicy is "
                  "the MLP policy of the -v0 state ids; CNN critics are not supported")

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
        num_envs, obs_dim, act_dim = self._resolve(envs, device, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim))
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        if env_id_offset is None:
            env_id_offset = int(envs._cfg.env_id_offset) if envs is not None and hasattr(envs, "_cfg") else 0
        self.env_id_offset = int(env_id_offset)
        if isinstance(hidden, dict):
            if set(hidden) != {"pi", "qf"}:
                raise ValueError("hidden: a dict must have exactly the keys 'pi' and 'qf'")
            self.pi, self.qf = tuple(int(w) for w in hidden["pi"]), tuple(int(w) for w in hidden["qf"])
        else:
            self.pi = self.qf = tuple(int(w) for w in hidden)
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}, got {activation!r}")
        self.activation = activation
        self.seed = int(seed) & (2 ** 64 - 1)
        self.calls = 0                   # sampling calls of __call__ so far: the `call` word of the collection noise
        self.target_calls = 0            # td_target calls so far: the `call` word of the batch noise
        fa, fc = C.c_int64(0), C.c_int64(0)
        if len(self.pi) <= 3 and len(self.qf) <= 3:
            self._lib.mcg_sac_blob_floats(self.obs_dim, self.act_dim, len(self.pi), _arr(self.pi), len(self.qf), _arr(self.qf), C.byref(fa),
                                          C.byref(fc))
        self.actor_floats, self.critic_floats = int(fa.value), int(fc.value)
        if self.actor_floats == 0:
            raise ValueError(f"unsupported shape: obs_dim {self.obs_dim}, act_dim {self.act_dim} (1..16), actor {self.pi}, critics {self.qf}: "
                             + _WIDTHS)
        f32 = dict(dtype=torch.float32, device=self.device)
        self._t = {"actor": torch.zeros(self.actor_floats, **f32), "critic": torch.zeros(self.critic_floats, **f32),
                   "critic_target": torch.zeros(self.critic_floats, **f32), "log_ent_coef": torch.zeros(1, **f32)}
        self._cbuf = _abi.McgSac(actor=self._t["actor"].data_ptr(), critic=self._t["critic"].data_ptr(),
                                 critic_target=self._t["critic_target"].data_ptr(), n_envs=self.num_envs, obs_dim=self.obs_dim,
                                 act_dim=self.act_dim, n_pi=len(self.pi), pi_width=_arr(self.pi), n_qf=len(self.qf), qf_width=_arr(self.qf),
                                 activation=_ACTIVATIONS[activation], actor_floats=self.actor_floats, critic_floats=self.critic_floats)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _initial_weights(self) -> dict:
        gen = torch.Generator().manual_seed(self.seed % (2 ** 63))
        sd = {}
        for m, out, k, _first in _actor_shapes(self.obs_dim, self.act_dim, self.pi) + _critic_shapes(self.obs_dim, self.act_dim, self.qf, "critic"):
            bound = 1.0 / math.sqrt(k)
            sd[m + ".weight"] = (torch.rand(out, k, generator=gen) * 2.0 - 1.0) * bound
            sd[m + ".bias"] = (torch.rand(out, generator=gen) * 2.0 - 1.0) * bound
        sd.update({k.replace("critic.", "critic_target.", 1): v for k, v in sd.items() if k.startswith("critic.")})
        return sd

    def _load_weights(self, sd: dict):
        D, A, dev = self.obs_dim, self.act_dim, self.device
        for name, blob in (("actor", pack_actor(sd, D, A, self.pi, device=dev)), ("critic", pack_critic(sd, D, A, self.qf, "critic", device=dev)),
                           ("critic_target", pack_critic(sd, D, A, self.qf, "critic_target", device=dev))):
            assert blob.numel() == self._t[name].numel(), (name, blob.numel(), self._t[name].numel())
            self._t[name].copy_(blob)    # in place: the struct keeps pointing at it

    @property
    def log_ent_coef(self) -> torch.Tensor:
        """float32 [1] on the device: SB3's ``ent_coef="auto"`` parameter; ``td_target`` reads it there."""
        return self._t["log_ent_coef"]

    def state_dict(self) -> dict:
        """The weights under SB3's ``SACPolicy`` names (device tensors, unpacked from the blobs), ``log_ent_coef``, and ``seed``,
        ``calls``, ``target_calls``."""
        D, A = self.obs_dim, self.act_dim
        sd = unpack_actor(self._t["actor"], D, A, self.pi)
        sd.update(unpack_critic(self._t["critic"], D, A, self.qf, "critic"))
        sd.update(unpack_critic(self._t["critic_target"], D, A, self.qf, "critic_target"))
        sd["log_ent_coef"] = self._t["log_ent_coef"].clone()
        sd.update({k: getattr(self, k) for k in _HOST})
        return sd

    def load_state_dict(self, sd: dict):
        """Weights under SB3's names (an SB3 ``SACPolicy``'s ``state_dict()`` as it stands, or this class's); repacks the three blobs.
        ``log_ent_coef``, ``seed``, ``calls`` and ``target_calls`` are taken where given."""
        sd = dict(sd)
        host = {k: sd.pop(k) for k in _HOST if k in sd}
        lec = sd.pop("log_ent_coef", None)
        _refuse_foreign(sd)
        want = set(state_names(len(self.pi), len(self.qf)))
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise ValueError(f"state dict does not fit actor {self.pi} / critics {self.qf}: missing {missing}, unexpected {extra}")
        self._load_weights(sd)
        if lec is not None:
            self._t["log_ent_coef"].copy_(torch.as_tensor(lec).detach().to(device=self.device, dtype=torch.float32).reshape(1))
        for k, v in host.items():
            setattr(self, k, int(v) & (2 ** 64 - 1) if k == "seed" else int(v))

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
        fn = getattr(module, "activation_fn", None)
        if activation is None and fn is not None:
            name = getattr(fn, "__name__", type(fn).__name__).lower()
            if name not in _ACTIVATIONS:
                raise ValueError(f"activation_fn {name!r} is not supported: relu or tanh")
            activation = name
        pi, qf = _hidden_of(sd, "actor.latent_pi"), _hidden_of(sd, "critic.qf0")[:-1]
        if not pi or not qf:
            raise ValueError("the module's state dict has no actor.latent_pi / critic.qf0 layers")
        pol = cls(envs, hidden=dict(pi=pi, qf=qf), activation=activation or "relu", seed=seed, **dims)
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
        B = batch_rows(observations, actions, self.obs_dim, self.act_dim, "q_values", self.device)
        keep = [observations[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [actions.contiguous()]
        rows = _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)})
        q = torch.empty(2, B, dtype=torch.float32, device=self.device) if out is None else out
        if q.dtype != torch.float32 or tuple(q.shape) != (2, B) or not q.is_contiguous() or q.device != self.device:
            raise ValueError(f"q_values: out: expected a contiguous float32 tensor {(2, B)} on {self.device}")
        self._call("mcg_sac_q", _abi.SAC_CRITIC_TARGET if target else _abi.SAC_CRITIC, C.byref(rows), C.c_int64(B), C.c_void_p(q.data_ptr()))
        return q[0], q[1]

    def td_target(self, batch, gamma: float = 0.99, ent_coef: Optional[float] = None, out: Optional[dict] = None) -> torch.Tensor:
        """SB3's target line on a replay batch (``HerBuffer.sample``'s ``HerSamples``, or anything with its ``next_observations``,
        ``rewards`` and ``dones``) -> target float32 [B]; one launch, and one call number of the batch noise.  ``ent_coef``: alpha
        given on the host; None: ``exp(log_ent_coef)``, read on the device.  ``out``: the tensors to write into, under
        ``mcg_sac_target_out``'s names (target, and any of next_action [B, A], next_log_prob [B], next_q [2, B], noise [B, A])."""
        who = "td_target"
        nxt = batch.next_observations
        B = batch_rows(nxt, None, self.obs_dim, self.act_dim, who, self.device)
        reward, done = _per_row(batch.rewards, B, "rewards", who, self.device), _per_row(batch.dones, B, "dones", who, self.device)
        keep = [nxt[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")]
        cb = _abi.McgHerBatch(next_obs=keep[0].data_ptr(), next_achieved=keep[1].data_ptr(), desired=keep[2].data_ptr(),
                              reward=reward.data_ptr(), done=done.data_ptr())
        out = self.new_target_out(B, "target") if out is None else check_out(out, self._target_shapes(B), "target", who, self.device)
        cout = _abi.McgSacTargetOut(**{k: v.data_ptr() for k, v in out.items()})
        lec = None if ent_coef is not None else C.c_void_p(self._t["log_ent_coef"].data_ptr())
        self._call("mcg_sac_target", C.byref(cb), C.c_int64(B), C.c_uint64(self.seed), C.c_uint64(self.target_calls), C.c_float(gamma),
                   C.c_float(0.0 if ent_coef is None else ent_coef), lec, C.byref(cout))
        self.target_calls += 1
        return out["target"]

    def new_target_out(self, B: int, *names) -> dict:
        """Fresh tensors for ``td_target``'s ``out`` under ``names``."""
        f32 = dict(dtype=torch.float32, device=self.device)
        shape = self._target_shapes(B)
        return {k: torch.empty(shape[k], **f32) for k in names}

    def _target_shapes(self, B: int) -> dict:
        return {"target": (B,), "next_log_prob": (B,), "next_q": (2, B), "next_action": (B, self.act_dim), "noise": (B, self.act_dim)}

    def polyak(self, tau: float = 0.005):
        """``critic_target <- (1 - tau) critic_target + tau critic`` over the blob (SB3's ``polyak_update``); one launch."""
        self._call("mcg_sac_polyak", C.c_double(tau))
