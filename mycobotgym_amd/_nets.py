"""What every policy family shares on the host: PPO / A2C (policy.py, policy_update.py) and, through _offpolicy.py, SAC and TD3 / DDPG.

Nothing here knows "on-policy" or "off-policy".  The packing of Linear layers into a blob and back (csrc/mcg_policy.hip's and
csrc/mcg_sac.hip's heads state the layouts; a critic's first layer and a bare vector are restated here, once), the checks of a batch's
rows and of a caller's ``out`` tensors, ``Nets`` -- the base of every policy: the constructor's shared steps, the weights and their
state dict both ways, ``from_module``'s activation --, ``GaussianActorCritic`` -- what ``ActorCritic`` and ``CnnActorCritic`` share
beyond it: the orthogonal start, ``forward`` and ``values`` around a family's marshalling -- and ``Update`` -- the base of
``PPOUpdate`` and ``OffPolicyUpdate``: the scratch's size and the moments' checkpoint.  A family's words (its buffer, "minibatch" or
"batch", ``vf`` or ``qf``) are arguments or class attributes.  Private: users import from the families' modules, which re-export what
they always had.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Optional

import torch

from . import _abi
from ._devbuf import DeviceBuffer

_ACTIVATIONS = {"tanh": _abi.POLICY_TANH, "relu": _abi.POLICY_RELU}
_KEYS = ("observation", "achieved_goal", "desired_goal")


# ----------------------------------------------------------------------------------------------------------- the blobs
# A layer is its tiles -- tile (T, kb), float 16 g + i = W[16 T + i][k(kb, g)] -- then its bias.  First layer: k(kb, g) = 4 kb + g over
# the D + 6 columns padded with zeros to a multiple of 4.  Later layers: k(4 t + r, g) = 16 t + 4 g + r.
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


def _param(sd, m, out, k, device):
    W = torch.as_tensor(sd[m + ".weight"]).detach().to(device=device, dtype=torch.float32)
    b = torch.as_tensor(sd[m + ".bias"]).detach().to(device=device, dtype=torch.float32)
    if tuple(W.shape) != (out, k) or tuple(b.shape) != (out,):
        raise ValueError(f"{m}: expected weight {(out, k)} and bias {(out,)}, got {tuple(W.shape)} and {tuple(b.shape)}")
    return W, b


def pack_net(sd: dict, shapes, act_dim: int = 0, device=None) -> torch.Tensor:
    """The entries of a state dict under SB3's names that ``shapes`` lists -- rows (module, out, in, first layer?) -> their blob
    (float32), with plain torch ops.  ``act_dim`` (a critic blob): a first layer is its tiles over the D + 6 feature columns
    (first-layer order), its tiles over the action padded to 16 columns (later-layer order), then its bias.  A row whose `in` is None
    is the bare vector ``sd[module]`` of `out` <= 16 floats, padded to 16 (PPO's log_std)."""
    parts = []
    for m, out, k, first in shapes:
        if k is None:
            x = torch.as_tensor(sd[m]).detach().to(device=device, dtype=torch.float32)
            if tuple(x.shape) != (out,):
                raise ValueError(f"{m}: expected shape {(out,)}, got {tuple(x.shape)} (a state-dependent or gSDE {m} is not supported)")
            parts += [x, x.new_zeros(16 - out)]
            continue
        W, b = _param(sd, m, out, k, device)
        if first and act_dim:
            F = k - act_dim
            Wa = torch.zeros(out, 16, dtype=torch.float32, device=W.device)
            Wa[:, :act_dim] = W[:, F:]
            parts += [_pack_layer(W[:, :F], b, True)[0], *_pack_layer(Wa, b, False)]
        else:
            parts += _pack_layer(W, b, first)
    return torch.cat(parts).contiguous()


def unpack_net(blob: torch.Tensor, shapes, act_dim: int = 0) -> dict:
    """The inverse of ``pack_net``, bit for bit."""
    sd, at = {}, 0
    for m, out, k, first in shapes:
        if k is None:
            sd[m], used = blob[at:at + out].clone(), 16
        elif first and act_dim:
            F = k - act_dim
            feat = out * (-(-F // 4) * 4)                                       # the feature tiles; then the action tiles and the bias
            Wf = _unpack_layer(torch.cat([blob[at:at + feat], blob.new_zeros(out)]), out, F, True)[0]
            Wa, b, used = _unpack_layer(blob[at + feat:], out, 16, False)
            sd[m + ".weight"], sd[m + ".bias"], used = torch.cat([Wf, Wa[:, :act_dim]], dim=1), b, feat + used
        else:
            sd[m + ".weight"], sd[m + ".bias"], used = _unpack_layer(blob[at:], out, k, first)
        at += used
    return sd


def names_of(shapes):
    """The state-dict keys of ``shapes``' rows, in their order."""
    return [n for m, _out, k, _first in shapes for n in ([m] if k is None else [m + ".weight", m + ".bias"])]


def orthogonal_start(shapes, seed: int, trunk: float = math.sqrt(2.0), action_net: float = 0.01, value_net: float = 1.0) -> dict:
    """SB3's start of an actor-critic policy for the rows of ``shapes``: orthogonal weights [out, in] (the gain of the two heads by
    their names, ``trunk`` for every other layer), zero biases, a zero bare vector.  One ``randn`` of (max, min) of a row's shape per
    weight, in the rows' order, from a generator seeded with ``seed``: the weights of a seed are fixed by that order."""
    gen = torch.Generator().manual_seed(seed % (2 ** 63))
    gains, sd = {"action_net": action_net, "value_net": value_net}, {}
    for m, out, k, _first in shapes:
        if k is None:
            sd[m] = torch.zeros(out)
            continue
        q, r = torch.linalg.qr(torch.randn(max(out, k), min(out, k), generator=gen, dtype=torch.float64))
        q = q * torch.sign(torch.diagonal(r))
        sd[m + ".weight"] = (gains.get(m, trunk) * (q if out >= k else q.T)).float()
        sd[m + ".bias"] = torch.zeros(out)
    return sd


def _hidden_of(sd: dict, stem: str):
    """The widths of the Linear layers ``stem``.0, .2, .. (a critic's last one is its head)."""
    widths, L = [], 0
    while f"{stem}.{2 * L}.weight" in sd:
        widths.append(int(sd[f"{stem}.{2 * L}.weight"].shape[0]))
        L += 1
    return tuple(widths)


def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0] * 3)[:3])


# ---------------------------------------------------------------------------------------------------------- the checks
def checked_rows(observations, actions, obs_dim: int, act_dim: int, who: str, device=None, *, words) -> int:
    """Checks float32 rows as a buffer yields them (a dict of observation / achieved_goal / desired_goal, and ``actions``) -> their
    number B.  ``words``, which a family binds: (the buffer's call, "minibatch" or "batch", what the nets are, the class whose
    ``__call__`` takes float64, actions required?).  B is read from ``actions`` where they are required, else from the observation
    (``actions`` may be None then).  Needs no device."""
    source, noun, nets, caller, need_actions = words
    if not isinstance(observations, dict):
        raise ValueError(f"{who}: observations must be the dict of float32 tensors that {source} yields (observation, achieved_goal, "
                         f"desired_goal); the picture buffers' samples (-v1 ids) are not supported: {nets} of the -v0 state ids")
    missing = [k for k in _KEYS if k not in observations]
    if missing:
        raise ValueError(f"{who}: observations lacks {missing}")
    o = observations["observation"]
    if need_actions:
        if not torch.is_tensor(actions) or actions.dim() != 2 or actions.shape[1] != act_dim:
            raise ValueError(f"{who}: actions: expected a float32 tensor [B, {act_dim}], got {tuple(getattr(actions, 'shape', ()))}")
        B = int(actions.shape[0])
    else:
        B = int(o.shape[0]) if torch.is_tensor(o) and o.dim() else 0
    if B < 1:
        raise ValueError(f"{who}: the {noun} is empty (B must be >= 1)")
    rows = [("observations['observation']", o, obs_dim), ("observations['achieved_goal']", observations["achieved_goal"], 3),
            ("observations['desired_goal']", observations["desired_goal"], 3)]
    if actions is not None:
        rows.append(("actions", actions, act_dim))
    for name, t, cols in rows:
        if not torch.is_tensor(t) or t.dtype != torch.float32:
            raise ValueError(f"{who}: {name}: expected float32, got {getattr(t, 'dtype', type(t).__name__)} (the float64 observations of "
                             f"envs.step go through {source.split('.')[0]}, or {caller}.__call__)")
        if tuple(t.shape) != (B, cols):
            raise ValueError(f"{who}: {name}: expected shape {(B, cols)}, got {tuple(t.shape)}")
        if device is not None and t.device != device:
            raise ValueError(f"{who}: {name} lives on {t.device}, the policy on {device}")
    return B


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


def _finite(x) -> bool:
    return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(float(x))


# ---------------------------------------------------------------------------------------------------------- the policy
class Nets(DeviceBuffer):
    """A subclass sets ``_CRITIC`` (``hidden``'s second key and the attribute of those widths: vf or qf), ``_DICT_NOTE`` (what the
    refusal of other keys adds), ``_SHAPE`` and ``_WIDTHS`` (the unsupported-shape text), ``_HOST`` (the host fields of a state dict),
    ``_refuse_foreign`` and ``_refuse_widths`` (its module's functions), and gives ``_nets()`` -- per weight blob of ``self._t``:
    (blob name, its shapes, act_dim for a critic blob else 0), in the blobs' order -- and ``_count_floats()`` (keeps the blobs' sizes,
    0 for a refused shape); ``_fit()`` names the shape a state dict must fit.  A family that is no MLP (the CNN) uses ``_setup_dims``
    alone and overrides ``_as_rows`` / ``_as_sb3``; its ``_refuse_foreign`` may return the dict to go on with."""
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"))
    _DICT_NOTE = ""
    _refuse_widths = staticmethod(lambda widths: None)

    def _setup_dims(self, envs, seed, dims: dict, device, env_id_offset):
        """The constructor's steps that know no MLP: the dimensions (attributes under ``_FROM_ENVS``'s keywords), ``env_id_offset``, the
        seed and the call number."""
        for (k, _attr), v in zip(self._FROM_ENVS, self._resolve(envs, device, dims)):
            setattr(self, k, int(v))
        if env_id_offset is None:
            env_id_offset = int(envs._cfg.env_id_offset) if envs is not None and hasattr(envs, "_cfg") else 0
        self.env_id_offset = int(env_id_offset)
        self.seed = int(seed) & (2 ** 64 - 1)
        self.calls = 0                   # sampling calls of __call__ so far: the `call` word of the collection noise

    def _setup(self, envs, hidden, activation, seed, dims: dict, device, env_id_offset):
        """``_setup_dims``, then an MLP family's steps: ``hidden``, the activation, the widths' refusals, the blobs' sizes."""
        self._setup_dims(envs, seed, dims, device, env_id_offset)
        if isinstance(hidden, dict):
            if set(hidden) != {"pi", self._CRITIC}:
                raise ValueError(f"hidden: a dict must have exactly the keys 'pi' and '{self._CRITIC}'" + self._DICT_NOTE)
            self.pi, critic = tuple(int(w) for w in hidden["pi"]), tuple(int(w) for w in hidden[self._CRITIC])
        else:
            self.pi = critic = tuple(int(w) for w in hidden)
        setattr(self, self._CRITIC, critic)
        self._refuse_widths(self.pi); self._refuse_widths(critic)
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}, got {activation!r}")
        self.activation = activation
        if len(self.pi) > 3 or len(critic) > 3 or self._count_floats() == 0:
            raise ValueError(f"unsupported shape: obs_dim {self.obs_dim}, act_dim {self.act_dim} (1..16), {self._SHAPE.format(self.pi, critic)}: "
                             + self._WIDTHS)

    # ------------------------------------------------------------------------------------------------------- weights
    def _fit(self):
        return self._SHAPE.format(self.pi, getattr(self, self._CRITIC))

    def _as_rows(self, sd: dict) -> dict:
        """A state dict under SB3's names and shapes -> with the [out, in] weights that ``_nets()``'s rows name (the CNN flattens its
        convolutions)."""
        return sd

    def _as_sb3(self, sd: dict) -> dict:
        """The inverse, on the unpacked weights: SB3's shapes, and SB3's further names for them (the CNN's aliases)."""
        return sd

    def _load_weights(self, sd: dict):
        sd = self._as_rows(sd)
        for name, shapes, a in self._nets():
            blob, mine = pack_net(sd, shapes, a, self.device), self._t[name]
            assert blob.numel() == mine.numel(), (name, blob.numel(), mine.numel())
            mine.copy_(blob)             # in place: the struct keeps pointing at it

    def state_dict(self) -> dict:
        """The weights under SB3's names (device tensors, unpacked from the blobs), a blob that is no net under its own name (SAC's
        ``log_ent_coef``), and the host fields: ``seed``, ``calls`` and, off-policy, ``target_calls``."""
        sd, nets, t = {}, self._nets(), self._t
        for name, shapes, a in nets:
            sd.update(unpack_net(t[name], shapes, a))
        sd = self._as_sb3(sd)
        sd.update({k: x.clone() for k, x in t.items() if k not in [n for n, *_ in nets]})      # (SAC: log_ent_coef)
        sd.update({k: getattr(self, k) for k in self._HOST})
        return sd

    def load_state_dict(self, sd: dict):
        """Weights under SB3's names (an SB3 policy's ``state_dict()`` as it stands, or this class's); repacks the device blobs.  What
        else ``state_dict`` gives is taken where given."""
        sd, t = dict(sd), self._t
        host = {k: sd.pop(k) for k in self._HOST if k in sd}
        other = {k: sd.pop(k, None) for k in t if k not in [n for n, *_ in self._nets()]}
        kept = self._refuse_foreign(sd)
        sd = sd if kept is None else kept         # (the CNN's hands the dict back without the extractor's aliases)
        want = set(names_of([row for _name, shapes, _a in self._nets() for row in shapes]))
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise ValueError(f"state dict does not fit {self._fit()}: missing {missing}, unexpected {extra}")
        self._load_weights(sd)
        for k, v in other.items():
            if v is not None:
                t[k].copy_(torch.as_tensor(v).detach().to(device=self.device, dtype=torch.float32).reshape(t[k].shape))
        for k, v in host.items():
            setattr(self, k, int(v) & (2 ** 64 - 1) if k == "seed" else int(v))

    @staticmethod
    def _activation_of(module, activation, default):
        """``from_module``'s activation: ``module.activation_fn`` where it has one (SB3), else ``activation``, else ``default``."""
        fn = getattr(module, "activation_fn", None)
        if activation is None and fn is not None:
            name = getattr(fn, "__name__", type(fn).__name__).lower()
            if name not in _ACTIVATIONS:
                raise ValueError(f"activation_fn {name!r} is not supported: {' or '.join(sorted(_ACTIVATIONS, key=lambda a: a != default))}")
            activation = name
        return activation or default


class GaussianActorCritic(Nets):
    """The base of ``ActorCritic`` and ``CnnActorCritic``: one blob ``_blob`` (a one-row ``_nets()`` table) whose heads are
    ``action_net``, ``value_net`` and the bare vector ``log_std`` of a diagonal Gaussian.  A subclass gives ``_shapes()`` (output name ->
    the shape ``forward`` writes) and ``_forward(x, call, deterministic, out, who)`` (its input's marshalling and its entry);
    ``_caller_out`` is its check of a caller's ``out``."""
    _HOST = ("seed", "calls")
    _t = property(lambda self: {"blob": self._blob})      # (_blob is read at each use: it may be rebound, with _cbuf.blob)

    def _initial_weights(self) -> dict:
        return orthogonal_start(self._nets()[0][1], self.seed)

    @staticmethod
    def _refuse_module(module):
        """What ``from_module`` refuses of an SB3 policy's own attributes, whatever its extractor."""
        if getattr(module, "use_sde", False):
            raise ValueError("gSDE (use_sde=True) is not supported: the noise is the diagonal Gaussian's, drawn per call")
        if getattr(module, "squash_output", False):
            raise ValueError("squash_output=True is not supported: the action is the unsquashed Gaussian sample")

    def _caller_out(self, out, shapes: dict, who: str):
        return out

    def _new(self, *names):
        shapes = self._shapes()
        return {k: torch.empty(shapes[k], dtype=torch.float32, device=self.device) for k in names}

    def forward(self, obs, deterministic: bool = False, out: Optional[dict] = None):
        """``obs``: what ``envs.reset`` / ``envs.step`` returned (device tensors, read in place) -> (action [N, A], value [N],
        log_prob [N]), float32 device tensors.  ``deterministic``: the action is the mean and no call number is used up.  ``out``: the
        tensors to write into, under the names of the entry's out struct (``_shapes()``'s keys: any subset)."""
        out = self._new("action", "value", "log_prob") if out is None else self._caller_out(out, self._shapes(), "forward")
        self._forward(obs, self.calls, deterministic, out, "forward")
        if not deterministic:
            self.calls += 1
        return out.get("action"), out.get("value"), out.get("log_prob")

    __call__ = forward

    def values(self, obs, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The value alone (the bootstrap of ``info["final_observation"]``, the last value of a rollout): float32 [N]; the policy head
        is not evaluated and no call number is used up."""
        v = self._new("value")["value"] if out is None else out
        self._forward(obs, 0, True, self._caller_out({"value": v}, self._shapes(), "values"), "values")
        return v

    def _eval_out(self, B: int, out, who: str):
        """``evaluate_actions``' outputs for B rows, new or the caller's -> (the dict, ``McgPolicyEvalOut``)."""
        if out is None:
            out = {k: torch.empty(B, dtype=torch.float32, device=self.device) for k in ("value", "log_prob", "entropy")}
        else:
            out = self._caller_out(out, {k: (B,) for k in ("value", "log_prob", "entropy")}, who)
        return out, _abi.McgPolicyEvalOut(**{k: v.data_ptr() for k, v in out.items()})


# ---------------------------------------------------------------------------------------------------------- the update
class Update:
    """A subclass sets ``_WORK_ENTRY`` (its ``mcg_*_grad_work_floats``) and ``_NOUN`` (minibatch or batch), gives ``_nets()`` -- blob
    name -> (its shapes, act_dim for a critic blob else 0) of the blobs it differentiates, from the policy's dimensions alone -- and
    keeps ``policy``, ``steps``, the scratch ``_work`` (None at first) and Adam's moments ``m`` and ``v``."""

    def _work_for(self, B: int) -> torch.Tensor:
        """The scratch for B rows: it only grows, so it is sized for the largest B seen."""
        pol = self.policy
        need = int(getattr(pol._lib, self._WORK_ENTRY)(C.byref(pol._cbuf), C.c_int64(B)))
        if need == 0:
            raise ValueError(f"{type(self).__name__}: a {self._NOUN} of {B} rows is not supported (1 <= B < 2^27)")
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=pol.device)
        return self._work

    # --------------------------------------------------------------------------------------------------- checkpoints
    def _moments(self):
        """(m, v) as dicts by blob name, and how a refusal names blob ``k`` of ``m`` or ``v``."""
        return self.m, self.v, "{}[{!r}]"

    def _named(self, t: dict) -> dict:
        """Blobs by name (gradients or moments) -> their entries under SB3's state-dict names; a bare float (SAC: log_ent_coef) cloned."""
        sd, nets = {}, self._nets()
        for k in t:
            sd.update(unpack_net(t[k], *nets[k]) if k in nets else {k: t[k].clone()})
        return sd

    def _moments_state(self) -> dict:
        m, v, _ = self._moments()
        return {"m": {k: t.clone() for k, t in m.items()}, "v": {k: t.clone() for k, t in v.items()}, "exp_avg": self._named(m),
                "exp_avg_sq": self._named(v), "step": self.steps}

    def _load_moments(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``; and ``step``."""
        dev, nets, (m, v, label) = self.policy.device, self._nets(), self._moments()
        for blob, mine, names in (("m", m, "exp_avg"), ("v", v, "exp_avg_sq")):
            if blob in sd:
                src = {k: torch.as_tensor(sd[blob][k], device=dev) for k in mine}
            elif names in sd:
                src = {k: pack_net(sd[names], *nets[k], device=dev) if k in nets else torch.as_tensor(sd[names][k], device=dev).reshape(1)
                       for k in mine}
            else:
                raise ValueError(f"the state dict has neither {blob!r} nor {names!r}")
            for k, t in mine.items():
                if src[k].dtype != torch.float32 or tuple(src[k].shape) != tuple(t.shape):
                    raise ValueError(f"{label.format(blob, k)}: expected float32 {tuple(t.shape)}, got {src[k].dtype} {tuple(src[k].shape)}")
            for k, t in mine.items():
                t.copy_(src[k])
        self.steps = int(sd["step"])
