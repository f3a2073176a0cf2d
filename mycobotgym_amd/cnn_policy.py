"""``CnnActorCritic`` -- the policy line of on-policy collection for the -v1 picture ids in HIP: action, value and log-prob from the
uint8 picture, read where the environment, ``FrameStack`` or a buffer left it.

The -v1 observation is a plain ``Box(0, 255, (C, S, S), uint8)``, for which SB3's ``CnnPolicy`` is ``ActorCriticCnnPolicy``: the byte
divided by 255, a ``NatureCNN`` features extractor shared by actor and critic (Conv2d(C, 32, 8, stride 4), Conv2d(32, 64, 4, stride 2),
Conv2d(64, 64, 3, stride 1), each with ReLU, no padding; Flatten; Linear(64 o3^2, F) with ReLU), ``net_arch=[]`` -- the two heads
``action_net`` and ``value_net`` directly on the F features -- and a diagonal Gaussian with a state-independent ``log_std``.  This file
owns the weights (one float32 device blob), the scratch between the two launches, the seed and the call number; the C side
(``mcg_cnn_forward``, ``mcg_cnn_evaluate``: csrc/mcg_cnn.hip) keeps no state and no call synchronises.

    envs = make("MyCobotReach-Sparse-joint-v1", num_envs=8192)      # or fs = FrameStack(envs, 4)
    pol = CnnActorCritic(envs, features_dim=512, seed=0)            # or CnnActorCritic.from_module(sb3_cnn_policy, envs)
    img, info = envs.reset(seed=0);  buf.start(img)
    for _ in range(32):
        a, v, logp = pol(img)                                       # two launches
        img, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, img, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
    buf.finish(last_values=pol.values(img))
    for mb in buf.get(4096):
        value, log_prob, entropy = pol.evaluate_actions(mb.observations, mb.actions)

No CPU or PyTorch fallback: the kernels are the only implementation of the forward.  Not built: the backward pass and an update for
this policy, CNN actors and critics for SAC / TD3 / DDPG, a non-empty ``net_arch``, separate extractors, bf16, S above 96.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import torch

from . import _abi
from ._nets import GaussianActorCritic, check_out, names_of, pack_net, unpack_net

_EXTRACTOR = "features_extractor."
_ALIASES = ("pi_features_extractor.", "vf_features_extractor.")      # SB3 >= 1.8: the same modules under two more names
_CONVS = {"features_extractor.cnn.0": (8, 4), "features_extractor.cnn.2": (4, 2), "features_extractor.cnn.4": (3, 1)}     # kernel, stride
_DOMAIN = "channels 1..16, image_size 36..96, features_dim a multiple of 16 in 16..512, act_dim 1..16"


def conv_sizes(image_size: int):
    """(o1, o2, o3): the three convolutions' output sizes for an S x S picture (no padding; the floor drops rows and columns)."""
    o1 = (image_size - 8) // 4 + 1
    o2 = (o1 - 4) // 2 + 1
    return o1, o2, o2 - 2


def accepted(channels: int, image_size: int, features_dim: int, act_dim: int) -> bool:
    return (1 <= channels <= 16 and 36 <= image_size <= 96 and 16 <= features_dim <= 512 and features_dim % 16 == 0
            and 1 <= act_dim <= 16)


# ------------------------------------------------------------------------------------------------------------ the blob
# csrc/mcg_cnn.hip's head states the layout; restated: conv1, conv2, conv3 (each weight as [out, in * k * k], PyTorch's own
# flattening), the linear layer, action_net (A rows padded to 16), value_net (1 row padded to 16), log_std padded to 16; every layer as
# _nets.py packs a later layer (all the K are multiples of 16), then its bias.
def blob_shapes(channels: int, image_size: int, features_dim: int, act_dim: int):
    """(weight key, out, in, first layer?) in the blob's order, a convolution's `in` flattened; the last row is the bare vector log_std."""
    o3 = conv_sizes(image_size)[2]
    return [("features_extractor.cnn.0", 32, channels * 64, False), ("features_extractor.cnn.2", 64, 32 * 16, False),
            ("features_extractor.cnn.4", 64, 64 * 9, False), ("features_extractor.linear.0", features_dim, 64 * o3 * o3, False),
            ("action_net", act_dim, features_dim, False), ("value_net", 1, features_dim, False), ("log_std", act_dim, None, False)]


def state_names(aliases: bool = True):
    """The keys of a state dict: the blob's order, then SB3 >= 1.8's aliases of the extractor."""
    names = names_of(blob_shapes(1, 64, 16, 1))
    return names + [a + n[len(_EXTRACTOR):] for a in _ALIASES for n in names if n.startswith(_EXTRACTOR)] if aliases else names


def blob_floats(channels: int, image_size: int, features_dim: int, act_dim: int) -> int:
    """The blob's size, counted here (``mcg_cnn_blob_floats`` counts it on the C side)."""
    return sum(16 if k is None else -(-out // 16) * 16 * (k + 1) for _m, out, k, _f in blob_shapes(channels, image_size, features_dim, act_dim))


def scratch_floats(image_size: int, rows: int) -> int:
    return rows * 64 * conv_sizes(image_size)[2] ** 2


def _flat(sd: dict, channels: int) -> dict:
    """The convolutions' weights [out, in, k, k] -> [out, in * k * k]."""
    sd = dict(sd)
    for (m, (k, _stride)), cin, out in zip(_CONVS.items(), (channels, 32, 64), (32, 64, 64)):
        W = torch.as_tensor(sd[m + ".weight"])
        if tuple(W.shape) != (out, cin, k, k):
            raise ValueError(f"{m}: expected weight {(out, cin, k, k)}, got {tuple(W.shape)}")
        sd[m + ".weight"] = W.detach().reshape(out, cin * k * k)
    return sd


def pack(sd: dict, channels: int, image_size: int, features_dim: int, act_dim: int, device=None) -> torch.Tensor:
    """A state dict under SB3's names (the aliases are not read) -> the blob (float32 [blob_floats]), with plain torch ops."""
    return pack_net(_flat(sd, channels), blob_shapes(channels, image_size, features_dim, act_dim), device=device)


def _unflat(sd: dict, channels: int, aliases: bool = True) -> dict:
    """The inverse of ``_flat``, in place; ``aliases``: and the extractor's entries again (cloned) under SB3 >= 1.8's two more names."""
    for (m, (k, _stride)), cin in zip(_CONVS.items(), (channels, 32, 64)):
        sd[m + ".weight"] = sd[m + ".weight"].reshape(-1, cin, k, k)
    if aliases:
        sd.update({a + n[len(_EXTRACTOR):]: v.clone() for a in _ALIASES for n, v in list(sd.items()) if n.startswith(_EXTRACTOR)})
    return sd


def unpack(blob: torch.Tensor, channels: int, image_size: int, features_dim: int, act_dim: int, aliases: bool = True) -> dict:
    """The inverse of ``pack``: the blob -> the state dict, bit for bit; ``aliases``: with SB3 >= 1.8's two more names of the extractor."""
    return _unflat(unpack_net(blob, blob_shapes(channels, image_size, features_dim, act_dim)), channels, aliases)


def _refuse_foreign(sd: dict) -> dict:
    """Names an unsupported SB3 configuration by the keys its state dict carries -> ``sd`` without the aliases of the extractor."""
    if any(k.startswith("mlp_extractor.") for k in sd):
        raise ValueError("a non-empty net_arch (mlp_extractor.* layers) is not supported: CnnPolicy's default net_arch=[] puts action_net "
                         "and value_net directly on the features")
    out = {}
    for k, v in sd.items():
        alias = next((a for a in _ALIASES if k.startswith(a)), None)
        if alias is None:
            out[k] = v
            continue
        shared = sd.get(_EXTRACTOR + k[len(alias):])
        if shared is None or tuple(shared.shape) != tuple(v.shape) or not torch.equal(torch.as_tensor(shared).detach().cpu(), torch.as_tensor(v).detach().cpu()):
            raise ValueError(f"share_features_extractor=False is not supported: {k} differs from {_EXTRACTOR + k[len(alias):]} (actor and "
                             "critic share one NatureCNN)")
    return out


class CnnActorCritic(GaussianActorCritic):
    _IMAGES = True
    _FROM_ENVS = (("num_envs", "num_envs"), ("channels", "channels"), ("image_size", "image_size"), ("act_dim", "action_dim"))
    _NO_STATES = ("the -v0 ids observe float64 states with their goals, which SB3 gives an MLP policy: CnnActorCritic is the CNN policy of "
                  "the -v1 picture ids; ActorCritic is the policy for them")
    _refuse_foreign = staticmethod(_refuse_foreign)

    def __init__(self, envs=None, features_dim: int = 512, seed: int = 0, *, num_envs: Optional[int] = None, channels: Optional[int] = None,
                 image_size: Optional[int] = None, act_dim: Optional[int] = None, device=None, env_id_offset: Optional[int] = None):
        """``envs``: a ``MyCobotImgVecEnv`` or a ``FrameStack`` (whose ``channels`` is k * C) to take the dimensions, the device and
        ``env_id_offset`` from; or give them by keyword.  ``features_dim``: the extractor's F, a multiple of 16 up to 512.  The weights
        start as SB3 initialises them (orthogonal: gain sqrt 2 in the extractor, 0.01 for the action head, 1 for the value head; zero
        biases and ``log_std``), from ``seed``."""
        self._setup_dims(envs, seed, dict(num_envs=num_envs, channels=channels, image_size=image_size, act_dim=act_dim), device, env_id_offset)
        self.features_dim = int(features_dim)
        shape = self._shape()
        if self.num_envs < 1 or not accepted(*shape):
            raise ValueError(f"unsupported shape: num_envs {self.num_envs}, channels {self.channels}, image_size {self.image_size}, "
                             f"features_dim {self.features_dim}, act_dim {self.act_dim}: " + _DOMAIN)
        self.blob_floats = int(self._lib.mcg_cnn_blob_floats(*shape))
        assert self.blob_floats == blob_floats(*shape), (self.blob_floats, blob_floats(*shape))
        self._blob = torch.zeros(self.blob_floats, dtype=torch.float32, device=self.device)
        self._cbuf = _abi.McgCnnPolicy(blob=self._blob.data_ptr(), n_envs=self.num_envs, channels=self.channels, image_size=self.image_size,
                                       features_dim=self.features_dim, act_dim=self.act_dim, blob_floats=self.blob_floats)
        self._scratch = None
        self._scratch_for(self.num_envs)
        self._load_weights(self._initial_weights())

    # ------------------------------------------------------------------------------------------------------- weights
    def _shape(self):
        return self.channels, self.image_size, self.features_dim, self.act_dim

    def _nets(self):
        return (("blob", blob_shapes(*self._shape()), 0),)

    def _fit(self):
        return "CnnPolicy with net_arch=[]"

    def _as_rows(self, sd: dict) -> dict:
        return _flat(sd, self.channels)

    def _as_sb3(self, sd: dict) -> dict:
        return _unflat(sd, self.channels)

    def _scratch_for(self, rows: int) -> None:
        """The scratch between the two launches for ``rows`` pictures: it only grows, so it is sized for the most rows seen."""
        need = int(self._lib.mcg_cnn_scratch_floats(*self._shape(), C.c_int64(rows)))
        if need == 0:
            raise ValueError(f"CnnActorCritic: {rows} rows are not supported (1 <= rows < 2^27)")
        if self._scratch is None or self._scratch.numel() < need:
            self._scratch = torch.empty(need, dtype=torch.float32, device=self.device)
            self._cbuf.scratch, self._cbuf.scratch_floats = self._scratch.data_ptr(), need

    def _initial_weights(self) -> dict:
        return _unflat(super()._initial_weights(), self.channels, aliases=False)      # (orthogonal on the flattened weight, as torch's)

    @classmethod
    def from_module(cls, module, envs=None, seed: int = 0, **dims):
        """From any ``nn.Module`` whose ``state_dict()`` carries SB3's names (an SB3 ``ActorCriticCnnPolicy``'s does).  ``features_dim``
        comes from the linear layer's shape.  gSDE, ``squash_output``, a non-empty ``net_arch`` and separate extractors are refused."""
        cls._refuse_module(module)
        if getattr(module, "share_features_extractor", True) is False:
            raise ValueError("share_features_extractor=False is not supported: actor and critic share one NatureCNN")
        sd = _refuse_foreign({k: v for k, v in module.state_dict().items()})
        if "features_extractor.linear.0.weight" not in sd:
            raise ValueError("the module's state dict has no features_extractor.linear.0 layer (a NatureCNN's)")
        pol = cls(envs, features_dim=int(sd["features_extractor.linear.0.weight"].shape[0]), seed=seed, **dims)
        pol.load_state_dict(sd)
        return pol

    # ------------------------------------------------------------------------------------------------------- forward
    def _pictures(self, img, name, rows, dtypes):
        """[rows, C, S, S] whose [S, S] planes are contiguous -> (``McgCnnObs``, the tensor it points into: keep it until the call).
        The environment's own layout (the [N, C, S, S] view of [C, N, S, S] planes) and a contiguous tensor pass without a copy."""
        if not torch.is_tensor(img):
            raise ValueError(f"{name}: expected a device tensor {dtypes[0]} [{rows}, {self.channels}, {self.image_size}, {self.image_size}], "
                             f"got {type(img).__name__}")
        if img.dtype not in dtypes:
            raise ValueError(f"{name}: expected {' or '.join(str(d) for d in dtypes)} pictures, got {img.dtype}")
        shape = (rows, self.channels, self.image_size, self.image_size)
        if tuple(img.shape) != shape:
            raise ValueError(f"{name}: expected shape {shape}, got {tuple(img.shape)}")
        if img.device != self.device:
            raise ValueError(f"{name} lives on {img.device}, the policy on {self.device}")
        if not img[0, 0].is_contiguous() or (self.channels > 1 and img.stride(1) < self.image_size ** 2) or (rows > 1 and img.stride(0) < 0):
            img = img.contiguous()
        kind = _abi.CNN_UINT8 if img.dtype == torch.uint8 else _abi.CNN_FLOAT32
        return _abi.McgCnnObs(pixels=img.data_ptr(), dtype=kind, env_stride=img.stride(0), chan_stride=img.stride(1)), img

    def _shapes(self):
        N, A, F = self.num_envs, self.act_dim, self.features_dim
        return {"action": (N, A), "mean": (N, A), "noise": (N, A), "value": (N,), "log_prob": (N,), "features": (N, F)}

    def _caller_out(self, out, shapes: dict, who: str):
        if not isinstance(out, dict) or not out:
            raise ValueError(f"{who}: out: a dict with at least one of {sorted(shapes)}")
        return check_out(out, shapes, next(iter(out)), who, self.device)

    def _forward(self, img, call, deterministic, out: dict, who):
        """``img``: uint8 [N, C, S, S], read in place; two launches.  ``out``: under ``mcg_cnn_out``'s names (``features`` too)."""
        cobs, _keep = self._pictures(img, who + ": img", self.num_envs, (torch.uint8,))
        cout = _abi.McgCnnOut(**{k: v.data_ptr() for k, v in out.items()})
        self._scratch_for(self.num_envs)
        self._call("mcg_cnn_forward", C.byref(cobs), C.c_uint64(self.seed), C.c_uint64(int(call) & (2 ** 64 - 1)),
                   C.c_int64(self.env_id_offset), int(bool(deterministic)), C.byref(cout))

    # ------------------------------------------------------------------------------------------------ on a minibatch
    def evaluate_actions(self, observations, actions, out: Optional[dict] = None):
        """SB3's ``evaluate_actions`` on a minibatch of ``ImageRolloutBuffer.get``: ``observations`` float32 [B, C, S, S] (the byte / 255:
        ``normalize=True``) or uint8 (``normalize=False``), ``actions`` float32 [B, A] -> (value [B], log_prob [B], entropy [B]), float32;
        two launches.  B is any number of rows >= 1.  ``out``: the tensors to write into, under the names value, log_prob, entropy."""
        who = "evaluate_actions"
        if isinstance(observations, dict):
            raise ValueError(f"{who}: observations must be the pictures [B, C, S, S] that ImageRolloutBuffer yields; the dict of a -v0 state id "
                             "is not supported: CnnActorCritic is the CNN policy of the -v1 picture ids")
        if not torch.is_tensor(actions) or actions.dim() != 2 or actions.shape[1] != self.act_dim or actions.dtype != torch.float32:
            raise ValueError(f"{who}: actions: expected a float32 tensor [B, {self.act_dim}], got {getattr(actions, 'dtype', type(actions).__name__)} "
                             f"{tuple(getattr(actions, 'shape', ()))}")
        B = int(actions.shape[0])
        if B < 1:
            raise ValueError(f"{who}: the minibatch is empty (B must be >= 1)")
        cobs, _keep = self._pictures(observations, who + ": observations", B, (torch.uint8, torch.float32))
        if actions.device != self.device:
            raise ValueError(f"{who}: actions lives on {actions.device}, the policy on {self.device}")
        a = actions if actions.is_contiguous() else actions.contiguous()
        out, cout = self._eval_out(B, out, who)
        self._scratch_for(B)
        self._call("mcg_cnn_evaluate", C.byref(cobs), C.c_void_p(a.data_ptr()), C.c_int64(B), C.byref(cout))
        return out.get("value"), out.get("log_prob"), out.get("entropy")
