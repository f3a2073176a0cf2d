"""The policy update's rule, restated (test infrastructure; torch float64 with autograd on ``indep_policy.Twin``, numpy float64 for
clip-by-norm and Adam).  Nothing here is shared with csrc/ or with mycobotgym_amd/policy.py / policy_update.py.

The loss (SB3's PPO.train / A2C.train on one minibatch, as recalled; include/mcg.h: mcg_policy_grad restates it):
    value, log_prob, entropy = evaluate_actions(obs, actions)
    adv <- (adv - mean) / (std + 1e-8) with torch.std (unbiased) where normalize_advantage and B > 1
    PPO: ratio = exp(log_prob - old_log_prob); policy_loss = -mean(min(adv ratio, adv clamp(ratio, 1 - c, 1 + c)))
    A2C: policy_loss = -mean(adv log_prob)
    value_loss = mean((returns - value)^2); entropy_loss = -mean(entropy); loss = policy_loss + ent_coef entropy_loss + vf_coef value_loss
    approx_kl = mean((ratio - 1) - ln ratio); clip_fraction = mean(|ratio - 1| > c)
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from tests import indep_policy as ip

STATS = ("loss", "policy_loss", "value_loss", "entropy_loss", "approx_kl", "clip_fraction")
HYPER = dict(loss="ppo", clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True)


# ----------------------------------------------------------------------------------------------------------------- loss
def loss_terms(twin: ip.Twin, batch: dict, loss="ppo", clip_range=0.2, ent_coef=0.0, vf_coef=0.5, normalize_advantage=True) -> dict:
    """The six stats as tensors of the twin's dtype (``loss`` carries the graph); ``batch``: numpy arrays under the names obs (the
    dict), actions, old_log_prob, advantages, returns."""
    dt = twin.log_std.dtype
    t = lambda x: torch.as_tensor(np.asarray(x)).to(dt)
    value, log_prob, entropy = twin.evaluate_actions({k: t(v) for k, v in batch["obs"].items()}, t(batch["actions"]))
    adv, ret = t(batch["advantages"]), t(batch["returns"])
    if normalize_advantage and len(adv) > 1:
        adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    if loss == "ppo":
        ratio = torch.exp(log_prob - t(batch["old_log_prob"]))
        policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - clip_range, 1 + clip_range)).mean()
        log_ratio = log_prob - t(batch["old_log_prob"])
        approx_kl = ((torch.exp(log_ratio) - 1) - log_ratio).mean().detach()
        clip_fraction = ((ratio - 1).abs() > clip_range).to(dt).mean().detach()
    else:
        assert loss == "a2c", loss
        policy_loss = -(adv * log_prob).mean()
        approx_kl = clip_fraction = torch.zeros((), dtype=dt)
    value_loss = ((ret - value) ** 2).mean()
    entropy_loss = -entropy.mean()
    return {"loss": policy_loss + ent_coef * entropy_loss + vf_coef * value_loss, "policy_loss": policy_loss, "value_loss": value_loss,
            "entropy_loss": entropy_loss, "approx_kl": approx_kl, "clip_fraction": clip_fraction}


def grad_and_stats(twin: ip.Twin, batch: dict, **hyper):
    """-> (gradient per parameter name, the six stats), numpy float64, by autograd in the twin's own dtype."""
    twin.zero_grad(set_to_none=True)
    terms = loss_terms(twin, batch, **hyper)
    terms["loss"].backward()
    grads = {k: (p.grad if p.grad is not None else torch.zeros_like(p)).detach().double().numpy().copy() for k, p in twin.named_parameters()}
    twin.zero_grad(set_to_none=True)
    return grads, {k: float(v.detach()) for k, v in terms.items()}


# ------------------------------------------------------------------------------------------------- clip-by-norm, Adam
def global_norm(grads: dict) -> float:
    return math.sqrt(sum(float((np.asarray(g, np.float64) ** 2).sum()) for g in grads.values()))


def clip_coef(norm: float, max_grad_norm: float) -> float:
    """clip_grad_norm_'s factor; max_grad_norm <= 0: no clipping."""
    return min(1.0, max_grad_norm / (norm + 1e-6)) if max_grad_norm > 0 else 1.0


def adam_step(p, g, m, v, step: int, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-5):
    """torch.optim.Adam's rule without amsgrad or weight decay -> (p, m, v), numpy float64."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** step)) * m / (np.sqrt(v) / math.sqrt(1 - beta2 ** step) + eps)
    return p, m, v


def twin_update(twin: ip.Twin, opt_state: dict, batch: dict, step: int, max_grad_norm=0.5, lr=3e-4, betas=(0.9, 0.999), eps=1e-5, **hyper):
    """One full update of the twin's parameters in float64 numpy arithmetic: autograd's gradient, the clip, Adam.  ``opt_state``: name ->
    (m, v), updated in place."""
    grads, stats = grad_and_stats(twin, batch, **hyper)
    coef = clip_coef(global_norm(grads), max_grad_norm)
    with torch.no_grad():
        for k, p in twin.named_parameters():
            m, v = opt_state.get(k, (np.zeros(p.shape), np.zeros(p.shape)))
            new, m, v = adam_step(p.detach().double().numpy(), coef * grads[k], m, v, step, lr, betas[0], betas[1], eps)
            opt_state[k] = (m, v)
            p.copy_(torch.from_numpy(new).to(p.dtype))
    return stats


# ------------------------------------------------------------------------------------------------------ the batch maker
def _min_relu_margin(twin: ip.Twin, x: torch.Tensor) -> torch.Tensor:
    """Per sample: the smallest |pre-activation| over both trunks' Linear layers."""
    worst = torch.full((len(x),), math.inf, dtype=x.dtype)
    for trunk in (twin.mlp_extractor.policy_net, twin.mlp_extractor.value_net):
        y = x
        for mod in trunk:
            y = mod(y)
            if isinstance(mod, nn.Linear):
                worst = torch.minimum(worst, y.abs().min(dim=1).values)
    return worst


def make_batch(twin64: ip.Twin, D: int, A: int, B: int, seed: int, clip_range: float = 0.2, relu: bool = False):
    """-> (batch, census).  Every array is a float32 number held in float64.  20 % more candidates than needed are drawn and the first
    B kept whose (a) relu pre-activations are all at least 1e-5 from 0 and (b) ratio is at least 1e-3 from both clip bounds, so that
    float32 and float64 take the same branch everywhere; fewer than 10 % of the candidates may be dropped."""
    n = int(math.ceil(1.2 * B)) + 1
    r32 = lambda x: np.asarray(x, np.float64).astype(np.float32).astype(np.float64)
    rng = np.random.default_rng(seed + 1000)
    obs = ip.round32(ip.random_obs(n, D, seed))
    with torch.no_grad():
        tobs = {k: torch.from_numpy(v) for k, v in obs.items()}
        _, value, _, mean = twin64(tobs, deterministic=True)
        actions = r32(mean.numpy() + np.exp(twin64.log_std.numpy()) * rng.normal(size=(n, A)))
        _, lp, _ = twin64.evaluate_actions(tobs, torch.from_numpy(actions))
        margin = _min_relu_margin(twin64, twin64._features(tobs)).numpy() if relu else np.full(n, np.inf)
    old = r32(lp.numpy() + rng.normal(size=n) * 0.15)
    adv = r32(0.3 + 2.0 * rng.normal(size=n))
    ret = r32(value.numpy() + rng.normal(size=n))
    ratio = np.exp(lp.numpy() - old)
    ok = (margin >= 1e-5) & (np.abs(ratio - (1 - clip_range)) >= 1e-3) & (np.abs(ratio - (1 + clip_range)) >= 1e-3)
    dropped = float((~ok).mean())
    assert dropped < 0.10, dropped
    keep = np.flatnonzero(ok)[:B]
    assert len(keep) == B, (len(keep), B)
    batch = {"obs": {k: v[keep] for k, v in obs.items()}, "actions": actions[keep], "old_log_prob": old[keep], "advantages": adv[keep],
             "returns": ret[keep]}
    census = {"dropped": dropped, "clip_fraction": float((np.abs(ratio[keep] - 1) > clip_range).mean()),
              "clip_margin": float(np.minimum(np.abs(ratio[keep] - (1 - clip_range)), np.abs(ratio[keep] - (1 + clip_range))).min()),
              "positive_advantages": float((adv[keep] > 0).mean())}
    return batch, census
