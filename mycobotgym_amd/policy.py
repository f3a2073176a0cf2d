"""``ActorCritic`` -- the policy line of on-policy collection as one HIP launch: action, value and log-prob from the engine's observation.

What the reference trains PPO and A2C with is SB3's ``MultiInputPolicy`` (scripts/train.py:99-101).  For the -v0 ids (a ``Dict`` space
of ``Box``es) that is SB3 >= 1.8's ``ActorCriticPolicy`` with a ``CombinedExtractor``: the flattened keys concatenated in sorted order
(``achieved_goal``, ``desired_goal``, ``observation``), two MLP trunks without shared layers, a linear head each and a diagonal
Gaussian with a state-independent ``log_std``.  This file owns the weights (one float32 device blob), the seed and the call number;
the C side (``mcg_policy_forward``, csrc/mcg_policy.hip) keeps no state and no call synchronises.

    pol = ActorCritic(envs, hidden=(64, 64), activation="tanh", seed=0)
    pol.load_state_dict(sb3_policy.state_dict())         # or ActorCritic.from_module(sb3_policy, envs)
    obs, _ = envs.reset(seed=0);  buf.start(obs)
    for _ in range(64):
        a, v, logp = pol(obs)                                         # one launch
        obs, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, obs, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
    buf.finish(last_values=pol.values(obs))

No CPU or PyTorch fallback: the kernel is the only implementation of the forward.  ``evaluate_actions`` is the same forward on a
minibatch of the rollout buffer; the loss, its gradient and Adam on the blob are ``PPOUpdate`` (policy_update.py).  A caller with an
optimiser of its own (any ``nn.Module`` with SB3's parameter names) repacks the blob with ``load_state_dict`` after an update.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Sequence

import torch

from . import _abi
from ._devbuf import DeviceBuffer

_ACTIVATIONS = {"tanh": _abi.POLICY_TANH, "relu": _abi.POLICY_RELU}
_HEADS = ("action_net.weight", "action_net.bias", "value_net.weight", "value_net.bias", "log_std")


# ------------------------------------------------------------------------------------------------------------ the blob
# csrc/mcg_policy.hip's head states the layout; restated: the policy net's layers, its head (A rows padded to 16), the value net's
# layers, its head (1 row padded to 16), log_std padded to 16.  A layer is its tiles -- tile (T, kb), float 16 g + i = W[16 T + i][k(kb, g)]
# -- then its bias.  First layer: k(kb, g) = 4 kb + g over the D + 6 columns padded with zeros to a multiple of 4.  Later layers:
# k(4 t + r, g) = 16 t + 4 g + r.
def _layer_names(net: str, n: int):
    return [f"mlp_extractor.{net}.{2 * L}" for L in range(n)]


def state_names(n_pi: int, n_vf: int):
    """The keys of a state dict, in the blob's order."""
    names = []
    for trunk, head in ((_layer_names("policy_net", n_pi), "action_net"), (_layer_names("value_net", n_vf), "value_net")):
        for m in trunk + [head]:
            names += [m + ".weight", m + ".bias"]
    return names + ["log_std"]


def _pack_layer(W: torch.Tensor, b: torch.Tensor, first: bool):
    out, k = W.shape
    out_p = -(-out // 16) * 16
    k_p = -(-k // 4) * 4 if first else k                  # (a later layer's input is a trunk width: a multiple of 16)
    Wp = torch.zeros(out_p, k_p, dtype=torch.float32, device=W.device)
    Wp[:out, :k] = W
    bp = torch.zeros(out_p, dtype=torch.float32, device=W.device)
    bp[:out] = b
    if first:
        tiles = Wp.view(out_p // 16, 16, k_p // 4, 4).permute(0, 2, 3, 1)                    # [T, kb, g, i] of W[16 T + i][4 kb + g]
    else:
        tiles = Wp.view(out_p // 16, 16, k_p // 16, 4, 4).permute(0, 2, 4, 3, 1)             # [T, t, r, g, i] of W[16 T + i][16 t + 4 g + r]
    return [tiles.reshape(-1), bp]


def _unpack_layer(flat: torch.Tensor, out: int, k: int, first: bool):
    out_p = -(-out // 16) * 16
    k_p = -(-k // 4) * 4 if first else k
    w, b = flat[:out_p * k_p], flat[out_p * k_p:out_p * k_p + out_p]
    if first:
        Wp = w.view(out_p // 16, k_p // 4, 4, 16).permute(0, 3, 1, 2)
    else:
        Wp = w.view(out_p // 16, k_p // 16, 4, 4, 16).permute(0, 4, 1, 3, 2)
    return Wp.reshape(out_p, k_p)[:out, :k].clone(), b[:out].clone(), out_p * k_p + out_p


def _shapes(obs_dim, act_dim, pi, vf):
    """(weight key, out, in, first layer?) in the blob's order."""
    rows = []
    for net, widths, head, head_out in (("policy_net", pi, "action_net", act_dim), ("value_net", vf, "value_net", 1)):
        k = obs_dim + 6
        for L, w in enumerate(widths):
            rows.append((f"mlp_extractor.{net}.{2 * L}", w, k, L == 0))
            k = w
        rows.append((head, head_out, k, False))
    return rows


def pack(sd: dict, obs_dim: int, act_dim: int, pi: Sequence[int], vf: Sequence[int], device=None) -> torch.Tensor:
    """A state dict under SB3's names -> the blob (float32 [blob_floats]), with plain torch ops."""
    parts = []
    for m, out, k, first in _shapes(obs_dim, act_dim, pi, vf):
        W = torch.as_tensor(sd[m + ".weight"]).detach().to(device=device, dtype=torch.float32)
        b = torch.as_tensor(sd[m + ".bias"]).detach().to(device=device, dtype=torch.float32)
        if tuple(W.shape) != (out, k) or tuple(b.shape) != (out,):
            raise ValueError(f"{m}: expected weight {(out, k)} and bias {(out,)}, got {tuple(W.shape)} and {tuple(b.shape)}")
        parts += _pack_layer(W, b, first)
    ls = torch.as_tensor(sd["log_std"]).detach().to(device=device, dtype=torch.float32)
    if tuple(ls.shape) != (act_dim,):
        raise ValueError(f"log_std: expected shape {(act_dim,)}, got {tuple(ls.shape)} (a state-dependent or gSDE log_std is not supported)")
    pad = torch.zeros(16, dtype=torch.float32, device=ls.device)
    pad[:act_dim] = ls
    return torch.cat(parts + [pad]).contiguous()


def unpack(blob: torch.Tensor, obs_dim: int, act_dim: int, pi: Sequence[int], vf: Sequence[int]) -> dict:
    """The inverse of ``pack``: the blob -> the state dict, bit for bit."""
    sd, at = {}, 0
    for m, out, k, first in _shapes(obs_dim, act_dim, pi, vf):
        sd[m + ".weight"], sd[m + ".bias"], used = _unpack_layer(blob[at:], out, k, first)
        at += used
    sd["log_std"] = blob[at:at + act_dim].clone()
    return sd


def _refuse_foreign(keys):
    """Names an unsupported SB3 configuration by the keys its state dict carries."""
    keys = list(keys)
    if any(".shared_net." in k for k in keys):
        raise ValueError("shared layers (mlp_extractor.shared_net) are not supported: SB3 >= 1.8 builds separate policy and value trunks")
    if any("cnn" in k.lower() for k in keys):
        raise ValueError("a CNN features extractor is not supported: ActorCritic serves the -v0 state ids (a Dict of Boxes)")
    if any(k.startswith(("features_extractor.", "pi_features_extractor.", "vf_features_extractor.")) for k in keys):
        raise ValueError("a features extractor with parameters is not supported: the features are the concatenated observation keys")


def _hidden_of(sd: dict, net: str):
    widths, L = [], 0
    while f"mlp_extractor.{net}.{2 * L}.weight" in sd:
        widths.append(int(sd[f"mlp_extractor.{net}.{2 * L}.weight"].shape[0]))
        L += 1
    return tuple(widths)


def minibatch_rows(observations, actions, obs_dim: int, act_dim: int, who: str) -> int:
    """Checks a minibatch as ``RolloutBuffer.get`` yields it (``RolloutSamples.observations``: the dict of float32 tensors, and
    ``actions``) -> its rows B.  Needs no device."""
    if not isinstance(observations, dict):
        raise ValueError(f"{who}: observations must be the dict of float32 tensors that RolloutBuffer yields (observation, achieved_goal, "
                         "desired_goal); the picture buffers' samples (-v1 ids) are not supported: the policy is the MLP of the -v0 state ids")
    missing = [k for k in ("observation", "achieved_goal", "desired_goal") if k not in observations]
    if missing:
        raise ValueError(f"{who}: observations lacks {missing}")
    if not torch.is_tensor(actions) or actions.dim() != 2 or actions.shape[1] != act_dim:
        raise ValueError(f"{who}: actions: expected a float32 tensor [B, {act_dim}], got {tuple(getattr(actions, 'shape', ()))}")
    B = int(actions.shape[0])
    if B < 1:
        raise ValueError(f"{who}: the minibatch is empty (B must be >= 1)")
    for name, t, cols in (("observations['observation']", observations["observation"], obs_dim),
                          ("observations['achieved_goal']", observations["achieved_goal"], 3),
                          ("observations['desired_goal']", observations["desired_goal"], 3), ("actions", actions, act_dim)):
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name}: expected float32, got {getattr(t, 'dtype', type(t).__name__)} (the float64 observations of "
                             "envs.step go through RolloutBuffer, or ActorCritic.__call__)")
        if tuple(t.shape) != (B, cols):
            raise ValueError(f"{who}: {name}: expected shape {(B, cols)}, got {tuple(t.shape)}")
    return B


class ActorCritic(DeviceBuffer):
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"))
    _NO_IMAGES = ("the -v1 image ids observe uint8 pictures, which SB3 gives a CNN extractor: ActorCritic is the MLP policy of the -v0 "
                  "state ids; CNN policies are not supported")

    def __init__(self, envs=None, hidden=(64, 64), activation: str = "tanh", seed: int = 0, *, num_envs: Optional[int] = None,
                 obs_dim: Optional[int] = None, act_dim: Optional[int] = None, device=None, env_id_offset: Optional[int] = None):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions, the device and ``env_id_offset`` from; or give them by keyword.
        ``hidden``: the widths of both trunks, or ``dict(pi=[...], vf=[...])`` (SB3's ``net_arch``): 1 to 3 layers, multiples of 16 up
        to 256.  The weights start as SB3 initialises them (orthogonal: gain sqrt 2 in the trunks, 0.01 for the action head, 1 for the
        value head; zero biases and ``log_std``), from ``seed``."""
        num_envs, obs_dim, act_dim = self._resolve(envs, device, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim))
        self.num_envs, self.obs_dim, self.act_dim = int(num_envs), int(obs_dim), int(act_dim)
        if env_id_offset is None:
            env_id_offset = int(envs._cfg.env_id_offset) if envs is not None and hasattr(envs, "_cfg") else 0
        self.env_id_offset = int(env_id_offset)
        if isinstance(hidden, dict):
            if set(hidden) != {"pi", "vf"}:
                raise ValueError("hidden: a dict must have exactly the keys 'pi' and 'vf' (shared layers are not supported)")
            self.pi, self.vf = tuple(int(w) for w in hidden["pi"]), tuple(int(w) for w in hidden["vf"])
        else:
            self.pi = self.vf = tuple(int(w) for w in hidden)
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}, got {activation!r}")
        self.activation = activation
        self.seed = int(seed) & (2 ** 64 - 1)
        self.calls = 0                   # sampling calls so far: the `call` word of the noise
        arr = lambda w: (C.c_int32 * 3)(*(list(w) + [0] * 3)[:3])
        self.blob_floats = int(self._lib.mcg_policy_blob_floats(self.obs_dim, self.act_dim, len(self.pi), arr(self.pi), len(self.vf),
                                                                arr(self.vf))) if len(self.pi) <= 3 and len(self.vf) <= 3 else 0
        if self.blob_floats == 0:
            raise ValueError(f"unsupported shape: obs_dim {self.obs_dim}, act_dim {self.act_dim} (1..16), trunks {self.pi} / {self.vf}: "
                             "1 to 3 hidden layers, each width a multiple of 16, at most 256")
        self._blob = torch.zeros(self.blob_floats, dtype=torch.float32, device=self.device)
        self._cbuf = _abi.McgPolicy(blob=self._blob.data_ptr(), n_envs=self.num_envs, obs_dim=self.obs_dim, act_dim=self.act_dim,
                                    n_pi=len(self.pi), n_vf=len(self.vf), pi_width=arr(self.pi), vf_width=arr(self.vf),
                                    activation=_ACTIVATIONS[activation], blob_floats=self.blob_floats)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _initial_weights(self) -> dict:
        gen = torch.Generator().manual_seed(self.seed % (2 ** 63))
        sd = {}
        for m, out, k, _first in _shapes(self.obs_dim, self.act_dim, self.pi, self.vf):
            gain = 0.01 if m == "action_net" else 1.0 if m == "value_net" else math.sqrt(2.0)
            q, r = torch.linalg.qr(torch.randn(max(out, k), min(out, k), generator=gen, dtype=torch.float64))
            q = q * torch.sign(torch.diagonal(r))
            sd[m + ".weight"] = (gain * (q if out >= k else q.T)).float()
            sd[m + ".bias"] = torch.zeros(out)
        sd["log_std"] = torch.zeros(self.act_dim)
        return sd

    def _load_weights(self, sd: dict):
        blob = pack(sd, self.obs_dim, self.act_dim, self.pi, self.vf, device=self.device)
        assert blob.numel() == self.blob_floats, (blob.numel(), self.blob_floats)
        self._blob.copy_(blob)           # in place: the struct keeps pointing at it

    def state_dict(self) -> dict:
        """The weights under SB3's ``ActorCriticPolicy`` names (device tensors, unpacked from the blob), plus ``seed`` and ``calls``."""
        sd = unpack(self._blob, self.obs_dim, self.act_dim, self.pi, self.vf)
        sd.update(seed=self.seed, calls=self.calls)
        return sd

    def load_state_dict(self, sd: dict):
        """Weights under SB3's names (an SB3 policy's ``state_dict()`` as it stands, or this class's); repacks the device blob.
        ``seed`` and ``calls`` are taken where given."""
        sd = dict(sd)
        host = {k: sd.pop(k) for k in ("seed", "calls") if k in sd}
        _refuse_foreign(sd)
        want = set(state_names(len(self.pi), len(self.vf)))
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise ValueError(f"state dict does not fit trunks {self.pi} / {self.vf}: missing {missing}, unexpected {extra}")
        self._load_weights(sd)
        if "seed" in host:
            self.seed = int(host["seed"]) & (2 ** 64 - 1)
        if "calls" in host:
            self.calls = int(host["calls"])

    @classmethod
    def from_module(cls, module, envs=None, activation: Optional[str] = None, seed: int = 0, **dims):
        """From any ``nn.Module`` whose ``state_dict()`` carries SB3's names (an SB3 ``ActorCriticPolicy`` / ``MultiInputPolicy``'s does).
        The trunks' widths come from the weights' shapes; the activation from ``module.activation_fn`` where it has one (SB3), else
        ``activation`` (default tanh).  gSDE, ``squash_output``, a CNN extractor and shared layers are refused."""
        if getattr(module, "use_sde", False):
            raise ValueError("gSDE (use_sde=True) is not supported: the noise is the diagonal Gaussian's, drawn per call")
        if getattr(module, "squash_output", False):
            raise ValueError("squash_output=True is not supported: the action is the unsquashed Gaussian sample")
        sd = {k: v for k, v in module.state_dict().items()}
        _refuse_foreign(sd)
        fn = getattr(module, "activation_fn", None)
        if activation is None and fn is not None:
            name = getattr(fn, "__name__", type(fn).__name__).lower()
            if name not in _ACTIVATIONS:
                raise ValueError(f"activation_fn {name!r} is not supported: tanh or relu")
            activation = name
        pi, vf = _hidden_of(sd, "policy_net"), _hidden_of(sd, "value_net")
        if not pi or not vf:
            raise ValueError("the module's state dict has no mlp_extractor.policy_net / mlp_extractor.value_net layers")
        pol = cls(envs, hidden=dict(pi=pi, vf=vf), activation=activation or "tanh", seed=seed, **dims)
        pol.load_state_dict(sd)
        return pol

    # ------------------------------------------------------------------------------------------------------- forward
    def _forward(self, obs, call, deterministic, out: dict):
        o, ag, dg = self._goal_obs(obs, "obs")
        cobs = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        cout = _abi.McgPolicyOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_policy_forward", C.byref(cobs), C.c_uint64(self.seed), C.c_uint64(int(call) & (2 ** 64 - 1)),
                   C.c_int64(self.env_id_offset), int(bool(deterministic)), C.byref(cout))

    def _new(self, *names):
        f32 = dict(dtype=torch.float32, device=self.device)
        N, A = self.num_envs, self.act_dim
        return {k: torch.empty((N, A) if k in ("action", "mean", "noise") else (N,), **f32) for k in names}

    def forward(self, obs, deterministic: bool = False, out: Optional[dict] = None):
        """``obs``: what ``envs.reset`` / ``envs.step`` returned (float64 device tensors, read in place) -> (action [N, A], value [N],
        log_prob [N]), float32 device tensors; one launch.  ``deterministic``: the action is the mean and no call number is used up.
        ``out``: the tensors to write into, under ``mcg_policy_out``'s names (action, value, log_prob, mean, noise: any subset)."""
        if out is None:
            out = self._new("action", "value", "log_prob")
        self._forward(obs, self.calls, deterministic, out)
        if not deterministic:
            self.calls += 1
        return out.get("action"), out.get("value"), out.get("log_prob")

    __call__ = forward

    def values(self, obs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The value net alone (the bootstrap of ``info["final_observation"]``, the last value of a rollout): float32 [N]; one launch."""
        v = self._new("value")["value"] if out is None else out
        self._forward(obs, 0, True, {"value": v})
        return v

    # ------------------------------------------------------------------------------------------------ on a minibatch
    def _minibatch(self, observations, actions, who, **more):
        """The minibatch as the C side takes it -> (``McgRolloutBatch``, B, the tensors it points into: keep them until the call).
        ``more``: further float32 [B] fields under ``mcg_rollout_batch``'s names."""
        B = minibatch_rows(observations, actions, self.obs_dim, self.act_dim, who)
        t = dict(obs=observations["observation"], achieved=observations["achieved_goal"], desired=observations["desired_goal"], action=actions)
        for k, x in more.items():
            if not torch.is_tensor(x) or x.dtype != torch.float32 or tuple(x.shape) != (B,):
                raise ValueError(f"{who}: {k}: expected a float32 tensor of shape {(B,)}, got {getattr(x, 'dtype', type(x).__name__)} "
                                 f"{tuple(getattr(x, 'shape', ()))}")
            t[k] = x
        for k, x in t.items():
            if x.device != self.device:
                raise ValueError(f"{who}: {k} lives on {x.device}, the policy on {self.device}")
        keep = [x if x.is_contiguous() else x.contiguous() for x in t.values()]
        return _abi.McgRolloutBatch(**{k: x.data_ptr() for k, x in zip(t, keep)}), B, keep

    def evaluate_actions(self, observations, actions, out: Optional[dict] = None):
        """SB3's ``evaluate_actions`` on a minibatch: ``observations`` is ``RolloutSamples.observations`` (the dict of float32 device
        tensors [B, .]), ``actions`` float32 [B, A] -> (value [B], log_prob [B], entropy [B]), float32; one launch.  B is any number of
        rows >= 1.  ``out``: the tensors to write into, under the names value, log_prob, entropy (any subset)."""
        batch, B, _keep = self._minibatch(observations, actions, "evaluate_actions")
        if out is None:
            out = {k: torch.empty(B, dtype=torch.float32, device=self.device) for k in ("value", "log_prob", "entropy")}
        cout = _abi.McgPolicyEvalOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_policy_evaluate", C.byref(batch), C.c_int64(B), C.byref(cout))
        return out.get("value"), out.get("log_prob"), out.get("entropy")
