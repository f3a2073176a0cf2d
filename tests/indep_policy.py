"""The actor-critic policy's rule, restated (test infrastructure; numpy float64, Python integers, and an eager torch twin).

Nothing here is shared with csrc/ or with mycobotgym_amd/policy.py.

The rule (SB3 >= 1.8's ActorCriticPolicy for a Dict space of Boxes, as recalled): the features are the observation's keys flattened
and concatenated in sorted key order -- achieved_goal (3), desired_goal (3), observation (D).  Two trunks without shared layers,
``mlp_extractor.policy_net`` and ``mlp_extractor.value_net``: Linear layers at the even indices 0, 2, .., each followed by the
activation (Tanh or ReLU).  Heads: ``action_net`` [A, H] on the policy trunk gives the mean, ``value_net`` [1, H] on the value trunk
the value.  Distribution (DiagGaussianDistribution): action = mean + exp(log_std) * eps;
log_prob = sum_k (-(action_k - mean_k)^2 / (2 exp(log_std_k)^2) - log_std_k - ln(2 pi) / 2), which at the sampled action is
sum_k (-eps_k^2 / 2 - log_std_k - ln(2 pi) / 2).

The noise (include/mcg.h: mcg_policy_forward).  Philox4x32-10 (Salmon et al. 2011), key = seed (low word, high word), counter
((uint32) gid, (uint32) call, pair ^ ((call >> 32) << 8), 6 ^ ((gid >> 32) << 8)), gid = env_id_offset + env the global environment
id, call the number of the sampling call, pair = 0 .. ceil(A / 2) - 1.  The block's words (r0, r1, r2, r3) give two uniforms of 53 bits,
u0 = ((r0 << 32 | r1) >> 11) 2^-53 and u1 likewise from (r2, r3); Box-Muller in float64:
    eps[2 pair] = sqrt(-2 ln(1 - u0)) cos(2 pi u1),    eps[2 pair + 1] = sqrt(-2 ln(1 - u0)) sin(2 pi u1)
each rounded to float32 once.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

MASK = 0xFFFFFFFF
DOMAIN = 6
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
KEYS = ("achieved_goal", "desired_goal", "observation")          # sorted: the concatenation order


# ---------------------------------------------------------------------------------------------------------------- noise
def philox4x32_10(ctr, key):
    """Restated from the paper's reference rounds: per round, (hi, lo) of the two 32 x 32 products, then the key's Weyl step."""
    c = [int(x) & MASK for x in ctr]
    k = [int(x) & MASK for x in key]
    for _ in range(10):
        hi0, lo0 = divmod(0xD2511F53 * c[0], 1 << 32)
        hi1, lo1 = divmod(0xCD9E8D57 * c[2], 1 << 32)
        c = [hi1 ^ c[1] ^ k[0], lo1, hi0 ^ c[3] ^ k[1], lo0]
        k = [(k[0] + 0x9E3779B9) & MASK, (k[1] + 0xBB67AE85) & MASK]
    return c


def counter(gid: int, call: int, pair: int):
    gid &= 2 ** 64 - 1
    call &= 2 ** 64 - 1
    return [gid & MASK, call & MASK, (pair ^ ((call >> 32) << 8)) & MASK, (DOMAIN ^ ((gid >> 32) << 8)) & MASK]


def block(seed: int, gid: int, call: int, pair: int):
    seed &= 2 ** 64 - 1
    return philox4x32_10(counter(gid, call, pair), [seed & MASK, seed >> 32])


def uniforms(words):
    return (((words[0] << 32) | words[1]) >> 11) * 2.0 ** -53, (((words[2] << 32) | words[3]) >> 11) * 2.0 ** -53


def noise64(seed: int, call: int, n_envs: int, act_dim: int, env_id_offset: int = 0) -> np.ndarray:
    """eps [N, A] in float64, before the one rounding to float32."""
    eps = np.zeros((n_envs, 2 * ((act_dim + 1) // 2)))
    for e in range(n_envs):
        for p in range((act_dim + 1) // 2):
            u0, u1 = uniforms(block(seed, env_id_offset + e, call, p))
            rad = math.sqrt(-2.0 * math.log(1.0 - u0))
            eps[e, 2 * p], eps[e, 2 * p + 1] = rad * math.cos(2.0 * math.pi * u1), rad * math.sin(2.0 * math.pi * u1)
    return eps[:, :act_dim]


def noise(seed: int, call: int, n_envs: int, act_dim: int, env_id_offset: int = 0) -> np.ndarray:
    return noise64(seed, call, n_envs, act_dim, env_id_offset).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ the rule, float64
def features(obs: dict) -> np.ndarray:
    return np.concatenate([np.asarray(obs[k], dtype=np.float64).reshape(len(obs[k]), -1) for k in KEYS], axis=1)


def round32(obs: dict) -> dict:
    """The inputs as the kernel sees them: float64 -> float32 (round to nearest even), held as float64 again."""
    return {k: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64) for k, v in obs.items()}


def _trunk(sd: dict, net: str, x: np.ndarray, activation: str) -> np.ndarray:
    L = 0
    while f"mlp_extractor.{net}.{2 * L}.weight" in sd:
        x = x @ np.asarray(sd[f"mlp_extractor.{net}.{2 * L}.weight"], np.float64).T + np.asarray(sd[f"mlp_extractor.{net}.{2 * L}.bias"], np.float64)
        x = np.tanh(x) if activation == "tanh" else np.maximum(x, 0.0)
        L += 1
    assert L >= 1
    return x


def rule(sd: dict, obs: dict, activation: str):
    """-> (mean [N, A], value [N]) in float64; ``sd``: numpy arrays under SB3's names."""
    x = features(obs)
    mean = _trunk(sd, "policy_net", x, activation) @ np.asarray(sd["action_net.weight"], np.float64).T + np.asarray(sd["action_net.bias"], np.float64)
    value = _trunk(sd, "value_net", x, activation) @ np.asarray(sd["value_net.weight"], np.float64).T + np.asarray(sd["value_net.bias"], np.float64)
    return mean, value[:, 0]


def log_prob(action, mean, log_std) -> np.ndarray:
    a, m, ls = (np.asarray(x, dtype=np.float64) for x in (action, mean, log_std))
    return (-((a - m) ** 2) / (2.0 * np.exp(ls) ** 2) - ls - LOG_SQRT_2PI).sum(axis=-1)


def sample(mean, log_std, eps) -> np.ndarray:
    return np.asarray(mean, np.float64) + np.exp(np.asarray(log_std, np.float64)) * np.asarray(eps, np.float64)


# ------------------------------------------------------------------------------------------------------------- the twin
class _Extractor(nn.Module):
    def __init__(self, k, pi, vf, act):
        super().__init__()
        def mlp(widths):
            layers, last = [], k
            for w in widths:
                layers += [nn.Linear(last, w), act()]
                last = w
            return nn.Sequential(*layers)
        self.policy_net, self.value_net = mlp(pi), mlp(vf)


class Twin(nn.Module):
    """An nn.Module with exactly SB3's parameter names whose forward is SB3's formula in eager torch (stable_baselines3 is not
    installed; this stands in for it): the casts, cat, Linear, Tanh / ReLU, Normal(mean, std).log_prob(a).sum(-1)."""

    def __init__(self, obs_dim: int, act_dim: int, pi=(64, 64), vf=None, activation: str = "tanh"):
        super().__init__()
        vf = pi if vf is None else vf
        self.activation_fn = {"tanh": nn.Tanh, "relu": nn.ReLU}[activation]
        self.mlp_extractor = _Extractor(obs_dim + 6, pi, vf, self.activation_fn)
        self.action_net = nn.Linear(pi[-1], act_dim)
        self.value_net = nn.Linear(vf[-1], 1)
        self.log_std = nn.Parameter(torch.zeros(act_dim))

    def randomize(self, seed: int):
        """Random weights with non-zero biases and a non-zero log_std (in [-0.5, 0.3]); weights of a scale that keeps tanh off its
        flat ends."""
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name == "log_std":
                    p.copy_(torch.rand(p.shape, generator=gen) * 0.8 - 0.5)
                elif name.endswith(".bias"):
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) / math.sqrt(p.shape[1]))
        return self

    def _dtype(self):
        return self.log_std.dtype

    def _features(self, obs: dict) -> torch.Tensor:
        return torch.cat([torch.as_tensor(obs[k]).to(self._dtype()).flatten(1) for k in KEYS], dim=1)

    def forward(self, obs: dict, noise=None, deterministic: bool = False):
        """-> (action, value [N], log_prob, mean); ``noise``: the eps to sample with (None: torch's own normal draw)."""
        x = self._features(obs)
        mean = self.action_net(self.mlp_extractor.policy_net(x))
        value = self.value_net(self.mlp_extractor.value_net(x)).flatten()
        std = torch.ones_like(mean) * self.log_std.exp()
        if deterministic:
            action = mean
        else:
            eps = torch.randn_like(mean) if noise is None else torch.as_tensor(noise).to(mean)
            action = mean + std * eps
        logp = torch.distributions.Normal(mean, std).log_prob(action).sum(-1)
        return action, value, logp, mean

    def predict_values(self, obs: dict) -> torch.Tensor:
        return self.value_net(self.mlp_extractor.value_net(self._features(obs))).flatten()

    def evaluate_actions(self, obs: dict, actions):
        x = self._features(obs)
        mean = self.action_net(self.mlp_extractor.policy_net(x))
        value = self.value_net(self.mlp_extractor.value_net(x)).flatten()
        dist = torch.distributions.Normal(mean, torch.ones_like(mean) * self.log_std.exp())
        return value, dist.log_prob(torch.as_tensor(actions).to(mean)).sum(-1), dist.entropy().sum(-1)

    def numpy_state(self) -> dict:
        return {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}


def random_obs(n: int, obs_dim: int, seed: int) -> dict:
    """Float64 inputs that are not float32 numbers, of the engine's magnitudes (positions below a metre, velocities of a few)."""
    rng = np.random.default_rng(seed)
    return {"observation": rng.normal(size=(n, obs_dim)) * 0.7, "achieved_goal": rng.normal(size=(n, 3)) * 0.2,
            "desired_goal": rng.normal(size=(n, 3)) * 0.2}


# The trunks the tests use: (pi widths, vf widths, activation)
TRUNKS = {"64x64-tanh": ((64, 64), (64, 64), "tanh"), "48x32-relu-vf16": ((48, 32), (16,), "relu"), "16-tanh": ((16,), (16,), "tanh"),
          "256x256-relu": ((256, 256), (256, 256), "relu"),
          # the shape edges of tests/policy_shape_cases.py
          "32x48x16-tanh-16x48x32": ((32, 48, 16), (16, 48, 32), "tanh"), "80x16x112-relu-96x240x16": ((80, 16, 112), (96, 240, 16), "relu"),
          "32-relu-80": ((32,), (80,), "relu"), "144x16-tanh-48": ((144, 16), (48,), "tanh"), "64x64x64-relu": ((64, 64, 64), (64, 64, 64), "relu")}
DIMS = ((10, 7), (25, 4), (25, 8))
