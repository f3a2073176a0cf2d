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

What is this policy's own here: the blob's order and SB3's names for it, the refusals of SB3 configurations, the two entries'
marshalling.  The layers' packing, the rows' check, the constructor's steps and the state dict both ways are _nets.py's, shared
with SAC and TD3 / DDPG; the orthogonal start, ``forward`` / ``values`` and the outputs of ``evaluate_actions`` are its
``GaussianActorCritic``'s, shared with ``CnnActorCritic``.
"""
from __future__ import annotations

import ctypes as C
import functools
from typing import Optional, Sequence

import torch

from . import _abi
from ._nets import _ACTIVATIONS, GaussianActorCritic, _arr, _hidden_of, checked_rows, names_of, pack_net, unpack_net

# minibatch_rows(observations, actions, obs_dim, act_dim, who): checks a minibatch as ``RolloutBuffer.get`` yields it
# (``RolloutSamples.observations``: the dict of float32 tensors, and ``actions``) -> its rows B.  Needs no device.
minibatch_rows = functools.partial(checked_rows, words=("RolloutBuffer", "minibatch", "the policy is the MLP", "ActorCritic", True))


# ------------------------------------------------------------------------------------------------------------ the blob
# csrc/mcg_policy.hip's head states the layout; restated: the policy net's layers, its head (A rows padded to 16), the value net's
# layers, its head (1 row padded to 16), log_std padded to 16; each layer as _nets.py's pack_net packs it.
def blob_shapes(obs_dim, act_dim, pi, vf):
    """(weight key, out, in, first layer?) in the blob's order; the last row is the bare vector log_std."""
    rows = []
    for net, widths, head, head_out in (("policy_net", pi, "action_net", act_dim), ("value_net", vf, "value_net", 1)):
        k = obs_dim + 6
        for L, w in enumerate(widths):
            rows.append((f"mlp_extractor.{net}.{2 * L}", w, k, L == 0))
            k = w
        rows.append((head, head_out, k, False))
    return rows + [("log_std", act_dim, None, False)]


def state_names(n_pi: int, n_vf: int):
    """The keys of a state dict, in the blob's order."""
    return names_of(blob_shapes(1, 1, [16] * n_pi, [16] * n_vf))


def pack(sd: dict, obs_dim: int, act_dim: int, pi: Sequence[int], vf: Sequence[int], device=None) -> torch.Tensor:
    """A state dict under SB3's names -> the blob (float32 [blob_floats]), with plain torch ops."""
    return pack_net(sd, blob_shapes(obs_dim, act_dim, pi, vf), device=device)


def unpack(blob: torch.Tensor, obs_dim: int, act_dim: int, pi: Sequence[int], vf: Sequence[int]) -> dict:
    """The inverse of ``pack``: the blob -> the state dict, bit for bit."""
    return unpack_net(blob, blob_shapes(obs_dim, act_dim, pi, vf))


def _refuse_foreign(keys):
    """Names an unsupported SB3 configuration by the keys its state dict carries."""
    keys = list(keys)
    if any(".shared_net." in k for k in keys):
        raise ValueError("shared layers (mlp_extractor.shared_net) are not supported: SB3 >= 1.8 builds separate policy and value trunks")
    if any("cnn" in k.lower() for k in keys):
        raise ValueError("a CNN features extractor is not supported: ActorCritic serves the -v0 state ids (a Dict of Boxes)")
    if any(k.startswith(("features_extractor.", "pi_features_extractor.", "vf_features_extractor.")) for k in keys):
        raise ValueError("a features extractor with parameters is not supported: the features are the concatenated observation keys")


class ActorCritic(GaussianActorCritic):
    _NO_IMAGES = ("the -v1 image ids observe uint8 pictures, which SB3 gives a CNN extractor: ActorCritic is the MLP policy of the -v0 "
                  "state ids; CNN policies are not supported")
    _CRITIC, _DICT_NOTE = "vf", " (shared layers are not supported)"
    _SHAPE, _WIDTHS = "trunks {} / {}", "1 to 3 hidden layers, each width a multiple of 16, at most 256"
    _refuse_foreign = staticmethod(_refuse_foreign)

    def __init__(self, envs=None, hidden=(64, 64), activation: str = "tanh", seed: int = 0, *, num_envs: Optional[int] = None,
                 obs_dim: Optional[int] = None, act_dim: Optional[int] = None, device=None, env_id_offset: Optional[int] = None):
        """``envs``: a ``MyCobotVecEnv`` to take the dimensions, the device and ``env_id_offset`` from; or give them by keyword.
        ``hidden``: the widths of both trunks, or ``dict(pi=[...], vf=[...])`` (SB3's ``net_arch``): 1 to 3 layers, multiples of 16 up
        to 256.  The weights start as SB3 initialises them (orthogonal: gain sqrt 2 in the trunks, 0.01 for the action head, 1 for the
        value head; zero biases and ``log_std``), from ``seed``."""
        self._setup(envs, hidden, activation, seed, dict(num_envs=num_envs, obs_dim=obs_dim, act_dim=act_dim), device, env_id_offset)
        self._blob = torch.zeros(self.blob_floats, dtype=torch.float32, device=self.device)
        self._cbuf = _abi.McgPolicy(blob=self._blob.data_ptr(), n_envs=self.num_envs, obs_dim=self.obs_dim, act_dim=self.act_dim,
                                    n_pi=len(self.pi), n_vf=len(self.vf), pi_width=_arr(self.pi), vf_width=_arr(self.vf),
                                    activation=_ACTIVATIONS[activation], blob_floats=self.blob_floats)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _nets(self):
        return (("blob", blob_shapes(self.obs_dim, self.act_dim, self.pi, self.vf), 0),)

    def _count_floats(self):
        self.blob_floats = int(self._lib.mcg_policy_blob_floats(self.obs_dim, self.act_dim, len(self.pi), _arr(self.pi), len(self.vf), _arr(self.vf)))
        return self.blob_floats

    @classmethod
    def from_module(cls, module, envs=None, activation: Optional[str] = None, seed: int = 0, **dims):
        """From any ``nn.Module`` whose ``state_dict()`` carries SB3's names (an SB3 ``ActorCriticPolicy`` / ``MultiInputPolicy``'s does).
        The trunks' widths come from the weights' shapes; the activation from ``module.activation_fn`` where it has one (SB3), else
        ``activation`` (default tanh).  gSDE, ``squash_output``, a CNN extractor and shared layers are refused."""
        cls._refuse_module(module)
        sd = {k: v for k, v in module.state_dict().items()}
        _refuse_foreign(sd)
        activation = cls._activation_of(module, activation, "tanh")
        pi, vf = _hidden_of(sd, "mlp_extractor.policy_net"), _hidden_of(sd, "mlp_extractor.value_net")
        if not pi or not vf:
            raise ValueError("the module's state dict has no mlp_extractor.policy_net / mlp_extractor.value_net layers")
        pol = cls(envs, hidden=dict(pi=pi, vf=vf), activation=activation, seed=seed, **dims)
        pol.load_state_dict(sd)
        return pol

    # ------------------------------------------------------------------------------------------------------- forward
    def _forward(self, obs, call, deterministic, out: dict, who=None):
        """``obs``: float64 device tensors, read in place; one launch.  ``out``: under ``mcg_policy_out``'s names."""
        o, ag, dg = self._goal_obs(obs, "obs")
        cobs = _abi.McgStepOut(obs=o.data_ptr(), achieved_goal=ag.data_ptr(), desired_goal=dg.data_ptr())
        cout = _abi.McgPolicyOut(**{k: v.data_ptr() for k, v in out.items()})
        self._call("mcg_policy_forward", C.byref(cobs), C.c_uint64(self.seed), C.c_uint64(int(call) & (2 ** 64 - 1)),
                   C.c_int64(self.env_id_offset), int(bool(deterministic)), C.byref(cout))

    def _shapes(self):
        N, A = self.num_envs, self.act_dim
        return {"action": (N, A), "mean": (N, A), "noise": (N, A), "value": (N,), "log_prob": (N,)}

    # ------------------------------------------------------------------------------------------------ on a minibatch
    def _minibatch(self, observations, actions, who, **more):
        """The minibatch as the C side takes it -> (``McgRolloutBatch``, B, the tensors it points into: keep them until the call).
        ``more``: further fields under ``mcg_rollout_batch``'s names, float32 [B] as ``check_minibatch`` (policy_update.py) has seen
        to."""
        B = minibatch_rows(observations, actions, self.obs_dim, self.act_dim, who)
        t = dict(obs=observations["observation"], achieved=observations["achieved_goal"], desired=observations["desired_goal"], action=actions)
        t.update(more)
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
        out, cout = self._eval_out(B, out, "evaluate_actions")
        self._call("mcg_policy_evaluate", C.byref(batch), C.c_int64(B), C.byref(cout))
        return out.get("value"), out.get("log_prob"), out.get("entropy")
