"""What the off-policy learners share on the host and is theirs alone: SAC (sac_policy.py, sac_update.py) and TD3 / DDPG (td3_policy.py,
td3_update.py).

The critics' shapes and blobs, the checks of a replay batch, ``check_common_hyper``, ``OffPolicyNets`` -- the base of ``SACPolicy`` and
``TD3Policy`` over _nets.py's ``Nets``: the blobs and the second call number, the ``nn.Linear`` start with the target copies, the
critics' forward and the marshalling of a replay batch -- and ``OffPolicyUpdate`` -- the base of ``SACUpdate`` and ``TD3Update`` over
_nets.py's ``Update``: the gradients, the per-row vectors, the inputs of a step and Adam on a blob.  What knows no replay batch, target
or critic (the layers' packing, the rows' and ``out`` checks, the state dict both ways, the moments' checkpoint) is _nets.py's, shared
with PPO.  Each family keeps its own networks' names, C struct, entries, refusals and the order of a step's launches.  Private: users
import from the four family modules, which re-export what they always had.
"""
from __future__ import annotations

import ctypes as C
import functools
import math
from typing import Sequence

import torch

from . import _abi
from ._devbuf import _ptr
from ._nets import _KEYS, Nets, Update, _arr, _finite, check_out, checked_rows, pack_net, unpack_net


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


def pack_critic(sd: dict, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", n_critics: int = 2, device=None) -> torch.Tensor:
    """The ``critic.*`` (or ``critic_target.*``) entries -> that blob."""
    return pack_net(sd, critic_shapes(obs_dim, act_dim, qf, prefix, n_critics), act_dim, device)


def unpack_critic(blob: torch.Tensor, obs_dim: int, act_dim: int, qf: Sequence[int], prefix: str = "critic", n_critics: int = 2) -> dict:
    """The inverse of ``pack_critic``, bit for bit."""
    return unpack_net(blob, critic_shapes(obs_dim, act_dim, qf, prefix, n_critics), act_dim)


# ---------------------------------------------------------------------------------------------------------- the checks
# batch_rows(observations, actions, obs_dim, act_dim, who, device=None): checks float32 rows as ``HerBuffer.sample`` yields them (a dict
# of observation / achieved_goal / desired_goal, and ``actions`` or None) -> their number B.  Needs no device.
batch_rows = functools.partial(checked_rows, words=("HerBuffer.sample", "batch", "the networks are the MLPs", "SACPolicy", False))


def _per_row(t, B, name, who, device):
    if not torch.is_tensor(t) or t.dtype != torch.float32:
        raise ValueError(f"{who}: {name}: expected float32, got {getattr(t, 'dtype', type(t).__name__)}")
    if tuple(t.shape) not in ((B,), (B, 1)):
        raise ValueError(f"{who}: {name}: expected shape {(B, 1)} or {(B,)}, got {tuple(t.shape)}")
    if device is not None and t.device != device:
        raise ValueError(f"{who}: {name} lives on {t.device}, the policy on {device}")
    return t.contiguous()


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


def _sac_rows(observations, actions):
    """Checked rows as the C side takes them -> (``McgSacRows``, the tensors it points into: keep them until the call)."""
    keep = [observations[k].contiguous() for k in _KEYS] + [actions.contiguous()]
    return _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)}), keep


# ---------------------------------------------------------------------------------------------------------- the policy
class OffPolicyNets(Nets):
    """A subclass sets what ``Nets`` asks for but ``_count_floats`` -- its ``_nets()`` lists each target ``X_target`` after its ``X``
    --, ``n_critics``, and gives ``_blob_floats()`` and ``_target_shapes(B)``."""
    _CRITIC, _SHAPE, _HOST = "qf", "actor {}, critics {}", ("seed", "calls", "target_calls")

    def _setup(self, envs, hidden, activation, seed, dims: dict, device, env_id_offset, blobs: Sequence[str]):
        """``Nets``' steps, then the second call number and the zeroed blobs ``self._t`` (``blobs``: their names; actor* of
        actor_floats, critic* of critic_floats)."""
        super()._setup(envs, hidden, activation, seed, dims, device, env_id_offset)
        self.target_calls = 0            # td_target calls so far: the `call` word of the batch noise
        self._t = {k: torch.zeros(self.actor_floats if k.startswith("actor") else self.critic_floats, dtype=torch.float32, device=self.device)
                   for k in blobs}

    def _count_floats(self):
        self.actor_floats, self.critic_floats = self._blob_floats()
        return self.actor_floats

    def _floats_of(self, entry, *more):
        """(actor_floats, critic_floats) of this shape by ``entry``, an ``mcg_*_blob_floats`` (``more``: its own arguments after the widths)."""
        fa, fc = C.c_int64(0), C.c_int64(0)
        getattr(self._lib, entry)(self.obs_dim, self.act_dim, len(self.pi), _arr(self.pi), len(self.qf), _arr(self.qf), *more, C.byref(fa), C.byref(fc))
        return int(fa.value), int(fc.value)

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

    # --------------------------------------------------------------------------------------------------- on a batch
    def _q_values(self, entry, which, observations, actions, out):
        B = batch_rows(observations, actions, self.obs_dim, self.act_dim, "q_values", self.device)
        rows, _keep = _sac_rows(observations, actions)
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
        keep = [nxt[k].contiguous() for k in _KEYS] + [reward, done]
        cb = _abi.McgHerBatch(**{k: t.data_ptr() for k, t in zip(("next_obs", "next_achieved", "desired", "reward", "done"), keep)})
        out = self.new_target_out(B, "target") if out is None else check_out(out, self._target_shapes(B), "target", who, self.device)
        return B, cb, keep, out

    def new_target_out(self, B: int, *names) -> dict:
        """Fresh tensors for ``td_target``'s ``out`` under ``names``."""
        f32 = dict(dtype=torch.float32, device=self.device)
        shape = self._target_shapes(B)
        return {k: torch.empty(shape[k], **f32) for k in names}


# ---------------------------------------------------------------------------------------------------------- the update
class OffPolicyUpdate(Update):
    """A subclass sets what ``Update`` asks for but ``_NOUN``, and ``_N_ROWS`` (per-row float32 scratch vectors of a batch: y, and
    SAC's logp), and gives ``_out_shapes(B)``."""
    _NOUN = "batch"

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
        work = self._work_for(B)
        if B not in self._rows:
            rows = tuple(torch.empty(B, dtype=torch.float32, device=self.policy.device) for _ in range(self._N_ROWS))
            self._rows = {B: rows if self._N_ROWS > 1 else rows[0]}          # (one vector: kept bare, as TD3Update always kept its y)
        rows = self._rows[B]
        return (work,) + (rows if isinstance(rows, tuple) else (rows,))

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
        return (B, *_sac_rows(batch.observations, batch.actions)) + self._buffers(B)

    def _check_out(self, out, B):
        if out is None:
            return None
        shapes = self._out_shapes(B)
        if not isinstance(out, dict) or not out:
            raise ValueError(f"{type(self).__name__}: out: a dict with any of {sorted(shapes)}")
        return check_out(out, shapes, next(iter(out)), type(self).__name__, self.policy.device)
