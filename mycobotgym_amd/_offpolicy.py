"""What the off-policy learners share on the host: SAC (sac_policy.py, sac_update.py) and TD3 / DDPG (td3_policy.py, td3_update.py).

The blobs' packing (csrc/mcg_sac.hip's head states the layouts; a critic's first layer is restated here, once), the checks of a replay
batch and of a caller's ``out`` tensors, ``OffPolicyNets`` -- the base of ``SACPolicy`` and ``TD3Policy``: the constructor's shared
steps, the weights and their state dict, the critics' forward and the marshalling of a replay batch -- and ``OffPolicyUpdate`` -- the
base of ``SACUpdate`` and ``TD3Update``: the scratch, the inputs of a step, Adam on a blob and the moments' checkpoint.  Each family
keeps its own networks' names, C struct, entries, refusals and the order of a step's launches.  Private: users import from the four
family modules, which re-export what they always had.
"""
from __future__ import annotations

import ctypes as C
import math
import numbers
from typing import Sequence

import torch

from . import _abi
from ._devbuf import DeviceBuffer, _ptr
from .policy import _ACTIVATIONS, _pack_layer, _unpack_layer

_HOST = ("seed", "calls", "target_calls")


# ----------------------------------------------------------------------------------------------------------- the blobs
def critic_shapes(obs_dim, act_dim, qf, prefix, n_critics=2):
    """(module, out, in, first layer?) in the order of the blob ``prefix`` = critic or critic_target: qf0, then qf1 with two critics;
    a first layer's `in` counts the action's columns."""
    rows = []
    for q in range(n_critics):
        k = obs_dim + 6 + act_dim
        for L, w in enumerate(qf):
            rows.append((f"{prefix}.qf{q}.{2 * L}", w, k, L == 0))
            k = w
        rows.append((f"{prefix}.qf{q}.{2 * len(qf)}", 1, k, False))
    return rows


def _param(sd, m, out, k, device):
    W = torch.as_tensor(sd[m + ".weight"]).detach().to(device=device, dtype=torch.float32)
    b = torch.as_tensor(sd[m + ".bias"]).detach().to(device=device, dtype=torch.float32)
    if tuple(W.shape) != (out, k) or tuple(b.shape) != (out,):
        raise ValueError(f"{m}: expected weight {(out, k)} and bias {(out,)}, got {tuple(W.shape)} and {tuple(b.shape)}")
    return W, b


def pack_net(sd: dict, shapes, act_dim: int = 0, device=None) -> torch.Tensor:
    """The entries of a state dict under SB3's names that ``shapes`` lists -> their blob (float32), with plain torch ops.  ``act_dim``
    (a critic blob): a first layer is its tiles over the D + 6 feature columns (first-layer order), its tiles over the action padded
    to 16 columns (later-layer order), then its bias."""
    parts = []
    for m, out, k, first in shapes:
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
        if first and act_dim:
            F = k - act_dim
            feat = out * (-(-F // 4) * 4)                                       # the feature tiles; then the action tiles and the bias
            Wf = _unpack_layer(torch.cat([blob[at:at + feat], blob.new_zeros(out)]), out, F, True)[0]
            Wa, b, used = _unpack_layer(blob[at + feat:], out, 16, False)
            sd[m + ".weight"], sd[m + ".bias"] = torch.cat([Wf, Wa[:, :act_dim]], dim=1), b
            at += feat + used
        else:
            sd[m + ".weight"], sd[m + ".bias"], used = _unpack_layer(blob[at:], out, k, first)
            at += used
    return sd


def pack_critic(sd: dict, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", n_critics: int = 2, device=None) -> torch.Tensor:
    """The ``critic.*`` (or ``critic_target.*``) entries -> that blob."""
    return pack_net(sd, critic_shapes(obs_dim, act_dim, qf, prefix, n_critics), act_dim, device)


def unpack_critic(blob: torch.Tensor, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", n_critics: int = 2) -> dict:
    """The inverse of ``pack_critic``, bit for bit."""
    return unpack_net(blob, critic_shapes(obs_dim, act_dim, qf, prefix, n_critics), act_dim)


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


def check_batch(batch, obs_dim: int, act_dim: int, device=None, who: str = "SACUpdate") -> int:
    """A ``HerSamples`` of ``HerBuffer.sample`` -> its rows B (no device needed); refuses the picture buffers' samples."""
    for k in ("observations", "actions", "next_observations", "dones", "rewards"):
        if not hasattr(batch, k):
            raise ValueError(f"{who}: the batch has no field {k!r}: pass what HerBuffer.sample yields (a HerSamples)")
    B = batch_rows(batch.observations, batch.actions, obs_dim, act_dim, who, device)
    if batch_rows(batch.next_observations, None, obs_dim, act_dim, who, device) != B:
        raise ValueError(f"{who}: next_observations has another number of rows than observations ({B})")
    _per_row(batch.rewards, B, "rewards", who, device)
    _per_row(batch.dones, B, "dones", who, device)
    return B


def _finite(x) -> bool:
    return isinstance(x, numbers.Real) and not isinstance(x, bool) and math.isfinite(float(x))


def check_common_hyper(learning_rate, gamma, tau, betas, eps, unbuilt: dict, refused: dict, sde_why: str, who: str):
    """The refusals both families' ``check_hyper`` start with: the keywords that are not built (``refused``: a family's own, keyword ->
    message) and the ranges of the hyper-parameters both have."""
    for k in unbuilt:
        if k in ("use_sde", "sde_sample_freq", "use_sde_at_warmup"):
            if unbuilt[k] in (False, None, -1):
                continue
            raise ValueError(f"gSDE ({k}) is not built: {sde_why}")
        if k in refused:
            raise ValueError(refused[k])
        if k in ("optimizer_class", "optimizer_kwargs"):
            raise ValueError(f"{k} is not built: the optimiser is torch.optim.Adam's rule without amsgrad or weight decay")
        raise TypeError(f"{who}: unexpected keyword {k!r}")
    if callable(learning_rate):
        raise ValueError("a learning-rate schedule is not built: learning_rate takes a float only (it may be set between steps)")
    if not _finite(learning_rate) or not float(learning_rate) > 0.0:
        raise ValueError(f"learning_rate must be a finite float > 0, got {learning_rate!r}")
    if not _finite(gamma) or not 0.0 <= float(gamma) <= 1.0:
        raise ValueError(f"gamma must be in [0, 1], got {gamma!r}")
    if not _finite(tau) or not 0.0 < float(tau) <= 1.0:
        raise ValueError(f"tau must be in (0, 1], got {tau!r}")
    if len(betas) != 2 or not all(_finite(b) and 0.0 <= float(b) < 1.0 for b in betas):
        raise ValueError(f"betas must be two numbers in [0, 1), got {betas!r}")
    if not _finite(eps) or float(eps) < 0.0:
        raise ValueError(f"eps must be finite and >= 0, got {eps!r}")


# ---------------------------------------------------------------------------------------------------------- the policy
class OffPolicyNets(DeviceBuffer):
    """A subclass sets ``_WIDTHS`` (the unsupported-shape text), ``_refuse_foreign`` and ``_state_names`` (its module's functions),
    ``n_critics``, and gives ``_nets()`` -- per weight blob of ``self._t``: (blob name, its shapes, act_dim for a critic blob else 0), in
    the blobs' order, each target ``X_target`` after its ``X`` -- ``_blob_floats()`` and ``_fit()``."""
    _FROM_ENVS = (("num_envs", "num_envs"), ("obs_dim", "obs_dim"), ("act_dim", "action_dim"))

    def _setup(self, envs, hidden, activation, seed, dims: dict, device, env_id_offset, blobs: Sequence[str], refuse_widths=None):
        """The constructor's shared steps: the dimensions, ``hidden``, the activation, the seed and call numbers, and the zeroed blobs
        ``self._t`` (``blobs``: their names; actor* of actor_floats, critic* of critic_floats)."""
        num_envs, obs_dim, act_dim = self._resolve(envs, device, dims)
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
        if refuse_widths is not None:
            refuse_widths(self.pi); refuse_widths(self.qf)
        if activation not in _ACTIVATIONS:
            raise ValueError(f"activation must be one of {sorted(_ACTIVATIONS)}, got {activation!r}")
        self.activation = activation
        self.seed = int(seed) & (2 ** 64 - 1)
        self.calls = 0                   # sampling calls of __call__ so far: the `call` word of the collection noise
        self.target_calls = 0            # td_target calls so far: the `call` word of the batch noise
        self.actor_floats, self.critic_floats = (0, 0) if len(self.pi) > 3 or len(self.qf) > 3 else self._blob_floats()
        if self.actor_floats == 0:
            raise ValueError(f"unsupported shape: obs_dim {self.obs_dim}, act_dim {self.act_dim} (1..16), actor {self.pi}, critics {self.qf}: "
                             + self._WIDTHS)
        self._t = {k: torch.zeros(self.actor_floats if k.startswith("actor") else self.critic_floats, dtype=torch.float32, device=self.device)
                   for k in blobs}

    def _floats_of(self, entry, *more):
        """(actor_floats, critic_floats) of this shape by ``entry``, an ``mcg_*_blob_floats`` (``more``: its own arguments after the widths)."""
        fa, fc = C.c_int64(0), C.c_int64(0)
        getattr(self._lib, entry)(self.obs_dim, self.act_dim, len(self.pi), _arr(self.pi), len(self.qf), _arr(self.qf), *more, C.byref(fa), C.byref(fc))
        return int(fa.value), int(fc.value)

    # ------------------------------------------------------------------------------------------------------- weights
    def _initial_weights(self) -> dict:
        gen = torch.Generator().manual_seed(self.seed % (2 ** 63))
        sd, nets = {}, self._nets()
        for name, shapes, _a in nets:
            if name.endswith("_target"):
                continue
            for m, out, k, _first in shapes:
                bound = 1.0 / math.sqrt(k)
                sd[m + ".weight"] = (torch.rand(out, k, generator=gen) * 2.0 - 1.0) * bound
                sd[m + ".bias"] = (torch.rand(out, generator=gen) * 2.0 - 1.0) * bound
        for name, _shapes, _a in nets:
            if name.endswith("_target"):
                net = name[:-len("_target")]
                sd.update({k.replace(net + ".", name + ".", 1): v for k, v in sd.items() if k.startswith(net + ".")})
        return sd

    def _load_weights(self, sd: dict):
        for name, shapes, a in self._nets():
            blob = pack_net(sd, shapes, a, self.device)
            assert blob.numel() == self._t[name].numel(), (name, blob.numel(), self._t[name].numel())
            self._t[name].copy_(blob)    # in place: the struct keeps pointing at it

    def _state_dict(self) -> dict:
        sd, nets = {}, self._nets()
        for name, shapes, a in nets:
            sd.update(unpack_net(self._t[name], shapes, a))
        sd.update({k: t.clone() for k, t in self._t.items() if k not in [n for n, *_ in nets]})      # (SAC: log_ent_coef)
        sd.update({k: getattr(self, k) for k in _HOST})
        return sd

    def _load_state_dict(self, sd: dict):
        sd = dict(sd)
        host = {k: sd.pop(k) for k in _HOST if k in sd}
        other = {k: sd.pop(k, None) for k in self._t if k not in [n for n, *_ in self._nets()]}
        type(self)._refuse_foreign(sd)
        want = set(self._state_names())
        missing, extra = sorted(want - set(sd)), sorted(set(sd) - want)
        if missing or extra:
            raise ValueError(f"state dict does not fit {self._fit()}: missing {missing}, unexpected {extra}")
        self._load_weights(sd)
        for k, v in other.items():
            if v is not None:
                self._t[k].copy_(torch.as_tensor(v).detach().to(device=self.device, dtype=torch.float32).reshape(self._t[k].shape))
        for k, v in host.items():
            setattr(self, k, int(v) & (2 ** 64 - 1) if k == "seed" else int(v))

    @staticmethod
    def _activation_of(module, activation):
        """``from_module``'s activation: ``module.activation_fn`` where it has one (SB3), else ``activation``, else relu."""
        fn = getattr(module, "activation_fn", None)
        if activation is None and fn is not None:
            name = getattr(fn, "__name__", type(fn).__name__).lower()
            if name not in _ACTIVATIONS:
                raise ValueError(f"activation_fn {name!r} is not supported: relu or tanh")
            activation = name
        return activation or "relu"

    # --------------------------------------------------------------------------------------------------- on a batch
    def _q_values(self, entry, which, observations, actions, out):
        B = batch_rows(observations, actions, self.obs_dim, self.act_dim, "q_values", self.device)
        keep = [observations[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [actions.contiguous()]
        rows = _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)})
        nc = self.n_critics
        q = torch.empty(nc, B, dtype=torch.float32, device=self.device) if out is None else out
        if not torch.is_tensor(q) or q.dtype != torch.float32 or tuple(q.shape) != (nc, B) or not q.is_contiguous() or q.device != self.device:
            raise ValueError(f"q_values: out: expected a contiguous float32 tensor {(nc, B)} on {self.device}")
        self._call(entry, which, C.byref(rows), C.c_int64(B), C.c_void_p(q.data_ptr()))
        return tuple(q[k] for k in range(nc))

    def _her_batch(self, batch, out, who):
        """A replay batch as ``td_target``'s entry takes it -> (B, ``McgHerBatch``, the tensors it points into: keep them until the
        call, the checked or fresh ``out``)."""
        nxt = batch.next_observations
        B = batch_rows(nxt, None, self.obs_dim, self.act_dim, who, self.device)
        reward, done = _per_row(batch.rewards, B, "rewards", who, self.device), _per_row(batch.dones, B, "dones", who, self.device)
        keep = [nxt[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [reward, done]
        cb = _abi.McgHerBatch(**{k: t.data_ptr() for k, t in zip(("next_obs", "next_achieved", "desired", "reward", "done"), keep)})
        out = self.new_target_out(B, "target") if out is None else check_out(out, self._target_shapes(B), "target", who, self.device)
        return B, cb, keep, out

    def new_target_out(self, B: int, *names) -> dict:
        """Fresh tensors for ``td_target``'s ``out`` under ``names``."""
        f32 = dict(dtype=torch.float32, device=self.device)
        shape = self._target_shapes(B)
        return {k: torch.empty(shape[k], **f32) for k in names}


# ---------------------------------------------------------------------------------------------------------- the update
class OffPolicyUpdate:
    """A subclass sets ``_WORK_ENTRY`` (its ``mcg_*_grad_work_floats``) and ``_N_ROWS`` (per-row float32 scratch vectors of a batch: y,
    and SAC's logp), gives ``_out_shapes(B)`` and ``_nets()`` -- blob name -> (its shapes, act_dim for the critic blob else 0) of the
    blobs it differentiates, from the policy's dimensions alone -- and keeps ``policy``."""

    def _bare(self, name, *args):
        pol = self.policy
        with torch.cuda.device(pol.device):
            _abi.check(getattr(pol._lib, name)(*args, pol._stream()), name)

    def _allocate(self, floats: dict):
        f32 = dict(dtype=torch.float32, device=self.policy.device)
        self.grad_blob = {k: torch.zeros(n, **f32) for k, n in floats.items()}
        self.m, self.v = {k: torch.zeros(n, **f32) for k, n in floats.items()}, {k: torch.zeros(n, **f32) for k, n in floats.items()}
        self.stats = torch.zeros(8, **f32)
        self._work, self._rows = None, {}      # the scratch, sized for the largest B seen; the per-row vectors per B

    def _buffers(self, B: int):
        pol = self.policy
        need = int(getattr(pol._lib, self._WORK_ENTRY)(C.byref(pol._cbuf), C.c_int64(B)))
        if need == 0:
            raise ValueError(f"{type(self).__name__}: a batch of {B} rows is not supported (1 <= B < 2^27)")
        if self._work is None or self._work.numel() < need:
            self._work = torch.empty(need, dtype=torch.float32, device=pol.device)
        if B not in self._rows:
            rows = tuple(torch.empty(B, dtype=torch.float32, device=pol.device) for _ in range(self._N_ROWS))
            self._rows = {B: rows if self._N_ROWS > 1 else rows[0]}          # (one vector: kept bare, as TD3Update always kept its y)
        rows = self._rows[B]
        return (self._work,) + (rows if isinstance(rows, tuple) else (rows,))

    def _adam(self, k, step=None):
        """Adam on blob ``k`` with its gradient; ``step``: the optimiser's count, ``self.steps`` where not given."""
        step = self.steps if step is None else step
        self._bare("mcg_sac_adam", _ptr(self.policy._t[k]), _ptr(self.grad_blob[k]), _ptr(self.m[k]), _ptr(self.v[k]),
                   C.c_int64(self.grad_blob[k].numel()), C.c_int64(step), C.c_double(self.learning_rate), C.c_double(self.betas[0]),
                   C.c_double(self.betas[1]), C.c_double(self.eps))

    def _inputs(self, batch):
        pol = self.policy
        if not float(self.learning_rate) > 0.0 or not math.isfinite(self.learning_rate):
            raise ValueError(f"learning_rate must be a finite float > 0, got {self.learning_rate!r}")
        B = check_batch(batch, pol.obs_dim, pol.act_dim, pol.device, type(self).__name__)
        keep = [batch.observations[k].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [batch.actions.contiguous()]
        rows = _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)})
        return (B, rows, keep) + self._buffers(B)

    def _check_out(self, out, B):
        if out is None:
            return None
        shapes = self._out_shapes(B)
        if not isinstance(out, dict) or not out:
            raise ValueError(f"{type(self).__name__}: out: a dict with any of {sorted(shapes)}")
        return check_out(out, shapes, next(iter(out)), type(self).__name__, self.policy.device)

    # --------------------------------------------------------------------------------------------------- checkpoints
    def _named(self, t: dict) -> dict:
        """Blobs by name (gradients or moments) -> their entries under SB3's state-dict names; a bare float (SAC: log_ent_coef) cloned."""
        sd, nets = {}, self._nets()
        for k in t:
            sd.update(unpack_net(t[k], *nets[k]) if k in nets else {k: t[k].clone()})
        return sd

    def _moments_state(self) -> dict:
        return {"m": {k: t.clone() for k, t in self.m.items()}, "v": {k: t.clone() for k, t in self.v.items()}, "exp_avg": self._named(self.m),
                "exp_avg_sq": self._named(self.v), "step": self.steps}

    def _load_moments(self, sd: dict):
        """The moments from the blobs ``m`` / ``v`` where given, else packed from ``exp_avg`` / ``exp_avg_sq``; and ``step``."""
        dev, nets = self.policy.device, self._nets()
        for blob, mine, names in (("m", self.m, "exp_avg"), ("v", self.v, "exp_avg_sq")):
            if blob in sd:
                src = {k: torch.as_tensor(sd[blob][k], device=dev) for k in mine}
            elif names in sd:
                src = {k: pack_net(sd[names], *nets[k], device=dev) if k in nets else torch.as_tensor(sd[names][k], device=dev).reshape(1)
                       for k in mine}
            else:
                raise ValueError(f"the state dict has neither {blob!r} nor {names!r}")
            for k, t in mine.items():
                if src[k].dtype != torch.float32 or tuple(src[k].shape) != tuple(t.shape):
                    raise ValueError(f"{blob}[{k!r}]: expected float32 {tuple(t.shape)}, got {src[k].dtype} {tuple(src[k].shape)}")
            for k, t in mine.items():
                t.copy_(src[k])
        self.steps = int(sd["step"])
