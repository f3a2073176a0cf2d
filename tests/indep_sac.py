"""SAC's actor, twin critics and TD target, restated (test infrastructure; numpy float64, Python integers, and an eager torch twin).

Nothing here is shared with csrc/ or with mycobotgym_amd/sac_policy.py.

The rule (SB3's SACPolicy for a Dict space of Boxes, as recalled; stable_baselines3 is not installed).  Features: the observation's
keys flattened and concatenated in sorted key order -- achieved_goal (3), desired_goal (3), observation (D).  Actor: ``latent_pi``,
Linear layers at the even indices 0, 2, .., each followed by the activation (ReLU by default, or Tanh); two linear heads on it, ``mu``
[A, H] and ``log_std`` [A, H]; log_std clamped to [-20, 2]; u = mu + exp(log_std) eps; action = tanh(u);
    log_prob = sum_k (-eps_k^2 / 2 - log_std_k - ln(2 pi) / 2) - sum_k ln(1 - action_k^2 + 1e-6).
SB3 writes the Gaussian term as Normal(mu, std).log_prob(u).sum(-1), which at u = mu + std eps is the expression above identically;
the twin evaluates the expression in eps, because at log_std = -20 the quotient (u - mu) / std is ill-conditioned in any precision
(test_sac_cpu checks the two forms against each other where the lower clamp does not act).  Critics: ``qf0``, ``qf1``, the same kind
of MLP on cat(features, action) with a Linear [1, H] last; ``critic_target`` a second pair.  Target line of SAC.train:
    a', logp' = action_log_prob(next_obs);  next_q = min(critic_target(next_obs, a')) - alpha logp';
    target = reward + (1 - done) gamma next_q.
Polyak: target <- (1 - tau) target + tau critic.

The noise (include/mcg.h: mcg_sac_act, mcg_sac_target).  Philox4x32-10 (Salmon et al. 2011), key = seed (low word, high word),
counter ((uint32) id, (uint32) call, pair ^ ((call >> 32) << 8), dom ^ ((id >> 32) << 8)); dom = 7 with id = env_id_offset + env for
the collection action, dom = 8 with id = the sample's index for the TD target; pair = 0 .. ceil(A / 2) - 1.  The block's words
(r0, r1, r2, r3) give two uniforms of 53 bits, u0 = ((r0 << 32 | r1) >> 11) 2^-53 and u1 likewise from (r2, r3); Box-Muller in float64:
    eps[2 pair] = sqrt(-2 ln(1 - u0)) cos(2 pi u1),    eps[2 pair + 1] = sqrt(-2 ln(1 - u0)) sin(2 pi u1)
each rounded to float32 once.
"""
from __future__ import annotations

import math
from collections import namedtuple
from fractions import Fraction

import numpy as np
import torch
from torch import nn

MASK = 0xFFFFFFFF
DOMAIN_ACT, DOMAIN_TARGET = 7, 8
LOG_SQRT_2PI = 0.5 * math.log(2.0 * math.pi)
LOG_STD_MIN, LOG_STD_MAX, EPSILON = -20.0, 2.0, 1e-6
KEYS = ("achieved_goal", "desired_goal", "observation")          # sorted: the concatenation order
MAX_SQUASHED = 0.99                                              # the makers keep |tanh(u)| at or below this
CLAMP_MARGIN = 1e-3                                              # and every pre-clamp log_std this far from both bounds

Batch = namedtuple("Batch", ["observations", "actions", "next_observations", "dones", "rewards"])


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


def counter(domain: int, ident: int, call: int, pair: int):
    ident &= 2 ** 64 - 1
    call &= 2 ** 64 - 1
    return [ident & MASK, call & MASK, (pair ^ ((call >> 32) << 8)) & MASK, (domain ^ ((ident >> 32) << 8)) & MASK]


def block(domain: int, seed: int, ident: int, call: int, pair: int):
    seed &= 2 ** 64 - 1
    return philox4x32_10(counter(domain, ident, call, pair), [seed & MASK, seed >> 32])


def uniforms(words):
    return (((words[0] << 32) | words[1]) >> 11) * 2.0 ** -53, (((words[2] << 32) | words[3]) >> 11) * 2.0 ** -53


def noise64(domain: int, seed: int, call: int, rows: int, act_dim: int, id_offset: int = 0) -> np.ndarray:
    """eps [rows, A] in float64, before the one rounding to float32."""
    eps = np.zeros((rows, 2 * ((act_dim + 1) // 2)))
    for e in range(rows):
        for p in range((act_dim + 1) // 2):
            u0, u1 = uniforms(block(domain, seed, id_offset + e, call, p))
            rad = math.sqrt(-2.0 * math.log(1.0 - u0))
            eps[e, 2 * p], eps[e, 2 * p + 1] = rad * math.cos(2.0 * math.pi * u1), rad * math.sin(2.0 * math.pi * u1)
    return eps[:, :act_dim]


def noise(domain: int, seed: int, call: int, rows: int, act_dim: int, id_offset: int = 0) -> np.ndarray:
    return noise64(domain, seed, call, rows, act_dim, id_offset).astype(np.float32)


# ------------------------------------------------------------------------------------------------------ the rule, float64
def features(obs: dict) -> np.ndarray:
    return np.concatenate([np.asarray(obs[k], dtype=np.float64).reshape(len(obs[k]), -1) for k in KEYS], axis=1)


def round32(obs: dict) -> dict:
    """The inputs as the kernel sees them: float64 -> float32 (round to nearest even), held as float64 again."""
    return {k: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64) for k, v in obs.items()}


def _linear(sd, m, x):
    return x @ np.asarray(sd[m + ".weight"], np.float64).T + np.asarray(sd[m + ".bias"], np.float64)


def _act(x, activation):
    return np.tanh(x) if activation == "tanh" else np.maximum(x, 0.0)


def _layers(sd, stem):
    L = 0
    while f"{stem}.{2 * L}.weight" in sd:
        L += 1
    return L


def actor_rule(sd: dict, obs: dict, activation: str):
    """-> (mu [N, A], log_std [N, A] clamped, the same before the clamp) in float64; ``sd``: numpy arrays under SB3's names."""
    x = features(obs)
    n = _layers(sd, "actor.latent_pi")
    assert n >= 1
    for L in range(n):
        x = _act(_linear(sd, f"actor.latent_pi.{2 * L}", x), activation)
    raw = _linear(sd, "actor.log_std", x)
    return _linear(sd, "actor.mu", x), np.clip(raw, LOG_STD_MIN, LOG_STD_MAX), raw


def pre_squash(mu, log_std, eps) -> np.ndarray:
    return np.asarray(mu, np.float64) + np.exp(np.asarray(log_std, np.float64)) * np.asarray(eps, np.float64)


def log_prob(eps, log_std, action) -> np.ndarray:
    e, ls, a = (np.asarray(x, dtype=np.float64) for x in (eps, log_std, action))
    return (-0.5 * e ** 2 - ls - LOG_SQRT_2PI).sum(-1) - np.log(1.0 - a ** 2 + EPSILON).sum(-1)


def q_rule(sd: dict, prefix: str, obs: dict, action, activation: str) -> np.ndarray:
    """-> [2, B] in float64: qf0 and qf1 of ``prefix`` (critic or critic_target)."""
    x0 = np.concatenate([features(obs), np.asarray(action, np.float64)], axis=1)
    out = []
    for q in range(2):
        stem = f"{prefix}.qf{q}"
        n = _layers(sd, stem) - 1
        assert n >= 1
        x = x0
        for L in range(n):
            x = _act(_linear(sd, f"{stem}.{2 * L}", x), activation)
        out.append(_linear(sd, f"{stem}.{2 * n}", x)[:, 0])
    return np.stack(out)


def target_rule(sd: dict, nxt: dict, reward, done, eps, gamma: float, alpha: float, activation: str) -> dict:
    """The target line in float64 -> target [B], next_action, next_log_prob, next_q [2, B]."""
    mu, ls, _ = actor_rule(sd, nxt, activation)
    a = np.tanh(pre_squash(mu, ls, eps))
    lp = log_prob(eps, ls, a)
    q = q_rule(sd, "critic_target", nxt, a, activation)
    r, d = np.asarray(reward, np.float64).reshape(-1), np.asarray(done, np.float64).reshape(-1)
    return {"target": r + (1.0 - d) * gamma * (q.min(axis=0) - alpha * lp), "next_action": a, "next_log_prob": lp, "next_q": q}


def polyak_rule(critic, target, tau: float) -> np.ndarray:
    return (1.0 - tau) * np.asarray(target, np.float64) + tau * np.asarray(critic, np.float64)


def polyak_restated(critic, target, tau: float) -> np.ndarray:
    """include/mcg.h's expression, rounding by rounding: (float32) fma(tau, (double) c, (1.0 - tau) * (double) t), the fma by exact
    rational arithmetic rounded to float64 once; tau = 1 the copy of the critic's bits, as the header special-cases it.  Finite inputs
    (a Fraction holds no others) unless tau = 1."""
    c, t = np.asarray(critic, np.float32).reshape(-1), np.asarray(target, np.float32).reshape(-1)
    if float(tau) == 1.0:
        return c.copy().reshape(np.shape(critic))
    omt, ft = 1.0 - float(tau), Fraction(float(tau))
    out = np.empty(c.shape, np.float32)
    for j in range(c.size):
        prod = omt * float(t[j])                                 # rounded to float64
        out[j] = np.float32(float(ft * Fraction(float(c[j])) + Fraction(prod)))
    return out.reshape(np.shape(critic))


# ------------------------------------------------------------------------------------------------------------- the twin
def _mlp(k, widths, act, head=None):
    layers, last = [], k
    for w in widths:
        layers += [nn.Linear(last, w), act()]
        last = w
    if head is not None:
        layers.append(nn.Linear(last, head))
    return nn.Sequential(*layers)


class _Actor(nn.Module):
    def __init__(self, k, act_dim, pi, act):
        super().__init__()
        self.latent_pi = _mlp(k, pi, act)
        self.mu, self.log_std = nn.Linear(pi[-1], act_dim), nn.Linear(pi[-1], act_dim)


class _Critic(nn.Module):
    n_critics = 2

    def __init__(self, k, qf, act):
        super().__init__()
        self.qf0, self.qf1 = _mlp(k, qf, act, head=1), _mlp(k, qf, act, head=1)


class Twin(nn.Module):
    """An nn.Module with exactly SB3's parameter names whose forward is SB3's formula in eager torch, usable in float32 and float64."""

    def __init__(self, obs_dim: int, act_dim: int, pi=(256, 256), qf=None, activation: str = "relu"):
        super().__init__()
        qf = pi if qf is None else qf
        self.activation_fn = {"tanh": nn.Tanh, "relu": nn.ReLU}[activation]
        self.activation, self.pi, self.qf = activation, tuple(pi), tuple(qf)
        self.actor = _Actor(obs_dim + 6, act_dim, pi, self.activation_fn)
        self.critic = _Critic(obs_dim + 6 + act_dim, qf, self.activation_fn)
        self.critic_target = _Critic(obs_dim + 6 + act_dim, qf, self.activation_fn)

    def randomize(self, seed: int, obs_dim: int):
        """Random weights with non-zero biases; critic_target differs from critic; the log_std head rescaled so that its output
        before the clamp has mean -9 and deviation 7.5 over random observations: both clamp bounds act in some rows."""
        gen = torch.Generator().manual_seed(seed)
        with torch.no_grad():
            for name, p in self.named_parameters():
                if name.endswith(".bias"):
                    p.copy_(torch.randn(p.shape, generator=gen) * 0.3)
                else:
                    p.copy_(torch.randn(p.shape, generator=gen) / math.sqrt(p.shape[1]))
            raw = actor_rule(self.numpy_state(), round32(random_obs(256, obs_dim, seed + 1)), self.activation)[2]
            scale = 7.5 / raw.std()
            self.actor.log_std.weight.mul_(scale)
            self.actor.log_std.bias.copy_((self.actor.log_std.bias.double() - raw.mean()) * scale - 9.0)
        return self

    def _dtype(self):
        return self.actor.mu.weight.dtype

    def _features(self, obs: dict) -> torch.Tensor:
        return torch.cat([torch.as_tensor(obs[k]).to(self._dtype()).flatten(1) for k in KEYS], dim=1)

    def action_log_prob(self, obs: dict, noise=None, deterministic: bool = False):
        """-> (action, log_prob, mu, log_std, u); ``noise``: the eps to sample with."""
        h = self.actor.latent_pi(self._features(obs))
        mu, log_std = self.actor.mu(h), torch.clamp(self.actor.log_std(h), LOG_STD_MIN, LOG_STD_MAX)
        eps = torch.zeros_like(mu) if deterministic else torch.as_tensor(noise).to(mu)
        u = mu + log_std.exp() * eps
        action = torch.tanh(u)
        logp = (-0.5 * eps ** 2 - log_std - LOG_SQRT_2PI).sum(-1) - torch.log(1.0 - action ** 2 + EPSILON).sum(-1)
        return action, logp, mu, log_std, u

    @staticmethod
    def gaussian_terms_sb3_form(mu, log_std, u):
        """SB3's own spelling of the Gaussian term, before its sum over the components: Normal(mu, std).log_prob(u) [N, A]."""
        return torch.distributions.Normal(mu, log_std.exp()).log_prob(u)

    def q(self, obs: dict, action, target: bool = False) -> torch.Tensor:
        """-> [2, B]"""
        net = self.critic_target if target else self.critic
        x = torch.cat([self._features(obs), torch.as_tensor(action).to(self._dtype())], dim=1)
        return torch.stack([net.qf0(x).flatten(), net.qf1(x).flatten()])

    def target(self, nxt: dict, reward, done, noise, gamma: float, alpha: float) -> dict:
        a, lp, *_ = self.action_log_prob(nxt, noise)
        q = self.q(nxt, a, target=True)
        r, d = (torch.as_tensor(x).to(self._dtype()).flatten() for x in (reward, done))
        next_q = torch.min(q, dim=0).values - alpha * lp
        return {"target": r + (1.0 - d) * gamma * next_q, "next_action": a, "next_log_prob": lp, "next_q": q}

    def numpy_state(self) -> dict:
        return {k: v.detach().cpu().numpy() for k, v in self.state_dict().items()}


# ----------------------------------------------------------------------------------------------------------- the makers
def random_obs(n: int, obs_dim: int, seed: int) -> dict:
    """Float64 inputs that are not float32 numbers, of the engine's magnitudes (positions below a metre, velocities of a few)."""
    rng = np.random.default_rng(seed)
    return {"observation": rng.normal(size=(n, obs_dim)) * 0.7, "achieved_goal": rng.normal(size=(n, 3)) * 0.2,
            "desired_goal": rng.normal(size=(n, 3)) * 0.2}


def conditions(sd: dict, obs: dict, eps, activation: str) -> np.ndarray:
    """Per row: |tanh(u)| <= 0.99 in the float64 rule for every component, and every pre-clamp log_std at least 1e-3 from both bounds."""
    mu, ls, raw = actor_rule(sd, round32(obs), activation)
    ok = np.abs(np.tanh(pre_squash(mu, ls, eps))) <= MAX_SQUASHED
    ok &= (np.abs(raw - LOG_STD_MIN) >= CLAMP_MARGIN) & (np.abs(raw - LOG_STD_MAX) >= CLAMP_MARGIN)
    return ok.all(axis=1)


def conditioned_obs(sd: dict, activation: str, n: int, obs_dim: int, seed: int, eps) -> dict:
    """``random_obs`` whose rows all meet ``conditions`` under the noise ``eps`` [n, A]: a row that does not is drawn again (the noise
    of a row is fixed by its index, so only the observation changes).  Past |tanh(u)| = 0.99 the correction term of the log-prob is
    ill-conditioned, and a comparison there would measure that conditioning, not the code under test."""
    obs = random_obs(n, obs_dim, seed)
    for attempt in range(1, 400):
        bad = ~conditions(sd, obs, eps, activation)
        if not bad.any():
            return obs
        fresh = random_obs(n, obs_dim, seed + 7919 * attempt)
        for k in obs:
            obs[k][bad] = fresh[k][bad]
    raise AssertionError("no observation found for some rows")


def replay_batch(sd: dict, activation: str, B: int, obs_dim: int, act_dim: int, seed: int, eps) -> Batch:
    """A replay batch in HerBuffer.sample's shapes, float32 numpy: next observations conditioned under ``eps`` (the TD target's noise),
    rewards of either sign, `done` with both values (B > 1)."""
    rng = np.random.default_rng(seed + 1)
    f32 = lambda d: {k: v.astype(np.float32) for k, v in d.items()}
    obs, nxt = f32(random_obs(B, obs_dim, seed + 2)), f32(conditioned_obs(sd, activation, B, obs_dim, seed + 3, eps))
    nxt["desired_goal"] = obs["desired_goal"] = nxt["desired_goal"]            # one goal per transition
    done = (rng.random(B) < 0.4).astype(np.float32)
    if B > 1:
        done[0], done[1] = 0.0, 1.0
    return Batch(observations=obs, actions=rng.uniform(-1.0, 1.0, (B, act_dim)).astype(np.float32), next_observations=nxt,
                 dones=done.reshape(B, 1), rewards=rng.normal(size=(B, 1)).astype(np.float32))


# The trunks the tests use: (actor widths, critic widths, activation)
TRUNKS = {"16-relu": ((16,), (16,), "relu"), "48x32-relu-qf16": ((48, 32), (16,), "relu"), "64x64-tanh": ((64, 64), (64, 64), "tanh"),
          "256x256-relu": ((256, 256), (256, 256), "relu"),
          # the shape edges of tests/policy_shape_cases.py
          "32x48x16-tanh-16x48x32": ((32, 48, 16), (16, 48, 32), "tanh"), "80x16x112-relu-96x240x16": ((80, 16, 112), (96, 240, 16), "relu"),
          "32-relu-80": ((32,), (80,), "relu"), "144x16-tanh-48": ((144, 16), (48,), "tanh"), "64x64x64-relu": ((64, 64, 64), (64, 64, 64), "relu")}
DIMS = ((10, 7), (25, 4), (25, 8))
CASES = [(D, A, name) for (D, A) in DIMS for name in ("16-relu", "48x32-relu-qf16", "64x64-tanh")] + [(25, 4, "256x256-relu")]
