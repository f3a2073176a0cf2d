"""SAC's update, restated (test infrastructure; torch autograd on ``indep_sac.Twin`` in the twin's own dtype, numpy float64 for Adam
and for the head derivative).  Nothing here is shared with csrc/ or with mycobotgym_amd/sac_update.py.

One gradient step of SB3's SAC.train, as recalled (stable_baselines3 is not installed), in its order:
    alpha = exp(log_ent_coef).detach()                            (before this step's alpha update; or the constant)
    a', logp' = actor(next_obs); y = r + (1 - done) gamma (min critic_target(next_obs, a') - alpha logp')
    critic_loss = 0.5 (mse(q0, y) + mse(q1, y)) on (obs, actions); critic.optimizer.step()              (no clipping)
    a, logp = actor(obs), fresh noise; actor_loss = mean(alpha logp - min critic(obs, a)); actor.optimizer.step()   (the new critic)
    ent_coef_loss = -mean(log_ent_coef (logp + target_entropy).detach()); ent_coef_optimizer.step()      (SB3 forms it before the
    critic loss from the same logp; it depends on the critic nowhere, so its place does not change a bit)
    polyak_update(critic, critic_target, tau) every target_update_interval steps
The actor loss's derivative at the heads (``head_derivative``), with a = tanh(u), s = 1 - a^2:
    d/du = (alpha 2 a s / (s + 1e-6) - dQ/da s) / B;  d/dmu = d/du;  d/dlog_std = d/du exp(log_std) eps - alpha / B, 0 where the clamp acts.
"""
from __future__ import annotations

import math

import numpy as np
import torch
from torch import nn

from tests import indep_sac as isac

DOMAIN_ACTOR_LOSS = 9
Q_GAP, RELU_MARGIN, MIN_EACH, FIRST_ROWS = 1e-3, 1e-4, 8, 75
STATS = ("critic_loss", "actor_loss", "ent_coef_loss", "ent_coef", "q0_mean", "q1_mean", "log_prob_mean")


def _t(twin, x):
    return torch.as_tensor(np.asarray(x)).to(twin._dtype())


def _obs(twin, obs: dict) -> dict:
    return {k: _t(twin, v) for k, v in obs.items()}


# --------------------------------------------------------------------------------------------------------------- losses
def td_target(twin, batch, eps_target, gamma: float, alpha: float) -> torch.Tensor:
    with torch.no_grad():
        return twin.target(_obs(twin, batch.next_observations), _t(twin, batch.rewards), _t(twin, batch.dones), _t(twin, eps_target), gamma,
                           alpha)["target"]


def critic_loss(twin, batch, y):
    q = twin.q(_obs(twin, batch.observations), _t(twin, batch.actions))
    return 0.5 * (((q[0] - y) ** 2).mean() + ((q[1] - y) ** 2).mean()), q


def actor_loss(twin, batch, eps_actor, alpha: float):
    """-> (loss, logp, q_pi [2, B], action, (mu, log_std, u))"""
    a, logp, mu, log_std, u = twin.action_log_prob(_obs(twin, batch.observations), _t(twin, eps_actor))
    q = twin.q(_obs(twin, batch.observations), a)
    return (alpha * logp - torch.min(q, dim=0).values).mean(), logp, q, a, (mu, log_std, u)


def ent_coef_loss(log_ent_coef, logp, target_entropy: float):
    return -(log_ent_coef * (logp.detach() + target_entropy)).mean()


def _grads_of(loss, named):
    named = list(named)
    gs = torch.autograd.grad(loss, [p for _, p in named], allow_unused=True)
    return {k: (torch.zeros_like(p) if g is None else g).detach().double().numpy().copy() for (k, p), g in zip(named, gs)}


def grads(twin, batch, eps_target, eps_actor, gamma: float, log_alpha=None, alpha=None, target_entropy: float = 0.0) -> dict:
    """The three gradients on the twin's parameters as they stand (no step in between), the stats and the intermediates, numpy
    float64, computed in the twin's own dtype.  ``log_alpha``: ent_coef = "auto"; else the constant ``alpha``."""
    dt = twin._dtype()
    lec = None if log_alpha is None else torch.tensor([float(log_alpha)], dtype=dt, requires_grad=True)
    al = float(alpha) if lec is None else float(torch.exp(lec.detach())[0])
    y = td_target(twin, batch, eps_target, gamma, al)
    closs, q = critic_loss(twin, batch, y)
    g = _grads_of(closs, [(k, p) for k, p in twin.named_parameters() if k.startswith("critic.")])
    aloss, logp, q_pi, a, _ = actor_loss(twin, batch, eps_actor, al)
    g.update(_grads_of(aloss, [(k, p) for k, p in twin.named_parameters() if k.startswith("actor.")]))
    a2 = a.detach().clone().requires_grad_(True)
    dq_da = torch.autograd.grad(torch.min(twin.q(_obs(twin, batch.observations), a2), dim=0).values.sum(), a2)[0]
    stats = {"critic_loss": float(closs.detach()), "actor_loss": float(aloss.detach()), "ent_coef_loss": 0.0, "ent_coef": al, "q0_mean": float(q[0].mean().detach()),
             "q1_mean": float(q[1].mean().detach()), "log_prob_mean": float(logp.mean().detach())}
    if lec is not None:
        eloss = ent_coef_loss(lec, logp, target_entropy)
        g["log_ent_coef"] = torch.autograd.grad(eloss, lec)[0].detach().double().numpy().copy()
        stats["ent_coef_loss"] = float(eloss.detach())
    mid = {"y": y, "q_pi": q_pi, "dq_da": dq_da, "logp": logp, "action": a}
    return {"grad": g, "stats": stats, "mid": {k: v.detach().double().numpy() for k, v in mid.items()}}


# -------------------------------------------------------------------------------------------------- the head derivative
def head_derivative(action, log_std_raw, eps, alpha: float, dq_da, B: int):
    """The actor loss's derivative with respect to the heads' outputs mu and log_std (before the clamp), numpy float64 [B, A] each."""
    a, raw, e, dq = (np.asarray(x, np.float64) for x in (action, log_std_raw, eps, dq_da))
    s = 1.0 - a * a
    du = (alpha * 2.0 * a * s / (s + isac.EPSILON) - dq * s) / B
    ls = np.clip(raw, isac.LOG_STD_MIN, isac.LOG_STD_MAX)
    dls = du * np.exp(ls) * e - alpha / B
    return du, np.where((raw < isac.LOG_STD_MIN) | (raw > isac.LOG_STD_MAX), 0.0, dls)


# ----------------------------------------------------------------------------------------------------------------- Adam
def adam_step(p, g, m, v, step: int, lr=3e-4, beta1=0.9, beta2=0.999, eps=1e-8):
    """torch.optim.Adam's rule without amsgrad or weight decay -> (p, m, v), numpy float64."""
    p, g, m, v = (np.asarray(x, np.float64) for x in (p, g, m, v))
    m = beta1 * m + (1 - beta1) * g
    v = beta2 * v + (1 - beta2) * g * g
    p = p - (lr / (1 - beta1 ** step)) * m / (np.sqrt(v) / math.sqrt(1 - beta2 ** step) + eps)
    return p, m, v


def _apply(twin, names, g, opt_state, step, lr, betas, eps):
    with torch.no_grad():
        for k, p in twin.named_parameters():
            if k in names:
                m, v = opt_state.get(k, (np.zeros(p.shape), np.zeros(p.shape)))
                new, m, v = adam_step(p.detach().double().numpy(), g[k], m, v, step, lr, betas[0], betas[1], eps)
                opt_state[k] = (m, v)
                p.copy_(torch.from_numpy(new).to(p.dtype))


def twin_step(twin, state: dict, batch, eps_target, eps_actor, step: int, gamma=0.99, tau=0.005, lr=3e-4, betas=(0.9, 0.999), eps=1e-8,
              auto=True, alpha=None, target_entropy=0.0, target_update_interval=1) -> dict:
    """One gradient step of the twin in SB3's order: the gradients by autograd in the twin's dtype, Adam in float64 arithmetic rounded
    to the twin's dtype.  ``state``: {"opt": name -> (m, v), "log_ent_coef": float}, updated in place.  -> the stats."""
    dt = twin._dtype()
    opt = state.setdefault("opt", {})
    lec = torch.tensor([float(state["log_ent_coef"])], dtype=dt, requires_grad=True) if auto else None
    al = float(torch.exp(lec.detach())[0]) if auto else float(alpha)
    y = td_target(twin, batch, eps_target, gamma, al)
    closs, q = critic_loss(twin, batch, y)
    names = [k for k, _ in twin.named_parameters() if k.startswith("critic.")]
    _apply(twin, names, _grads_of(closs, [(k, p) for k, p in twin.named_parameters() if k in names]), opt, step, lr, betas, eps)
    aloss, logp, _, _, _ = actor_loss(twin, batch, eps_actor, al)
    names = [k for k, _ in twin.named_parameters() if k.startswith("actor.")]
    _apply(twin, names, _grads_of(aloss, [(k, p) for k, p in twin.named_parameters() if k in names]), opt, step, lr, betas, eps)
    stats = {"critic_loss": float(closs.detach()), "actor_loss": float(aloss.detach()), "ent_coef_loss": 0.0, "ent_coef": al, "q0_mean": float(q[0].mean().detach()),
             "q1_mean": float(q[1].mean().detach()), "log_prob_mean": float(logp.mean().detach())}
    if auto:
        eloss = ent_coef_loss(lec, logp, target_entropy)
        g = torch.autograd.grad(eloss, lec)[0].detach().double().numpy()
        m, v = opt.get("log_ent_coef", (np.zeros(1), np.zeros(1)))
        new, m, v = adam_step(lec.detach().double().numpy(), g, m, v, step, lr, betas[0], betas[1], eps)
        opt["log_ent_coef"] = (m, v)
        state["log_ent_coef"] = float(torch.from_numpy(new).to(dt)[0])
        stats["ent_coef_loss"] = float(eloss.detach())
    if step % target_update_interval == 0:
        with torch.no_grad():
            for c, t in zip(twin.critic.parameters(), twin.critic_target.parameters()):
                t.copy_(torch.from_numpy(isac.polyak_rule(c.double().numpy(), t.double().numpy(), tau)).to(dt))
    return stats


# ------------------------------------------------------------------------------------------------------ the batch maker
def _margins(seq: nn.Sequential, x: torch.Tensor) -> torch.Tensor:
    """Per row: the smallest |pre-activation| / (the layer's largest over the batch), over the Linear layers that an activation follows."""
    worst = torch.full((len(x),), math.inf, dtype=x.dtype)
    mods = list(seq)
    for j, mod in enumerate(mods):
        x = mod(x)
        if isinstance(mod, nn.Linear) and j + 1 < len(mods):
            worst = torch.minimum(worst, x.abs().min(dim=1).values / x.abs().max())
    return worst


def row_conditions(twin64, obs: dict, actions, eps_actor) -> dict:
    """Per row, in the float64 twin on the float32 inputs: every condition of the maker, by name."""
    act = twin64.activation
    with torch.no_grad():
        tobs = _obs(twin64, obs)
        a, _, _, _, _ = twin64.action_log_prob(tobs, _t(twin64, eps_actor))
        q = twin64.q(tobs, a)
        ok = {"squash_and_clamp_margin": isac.conditions(twin64.numpy_state(), obs, eps_actor, act),
              "q_gap": ((q[0] - q[1]).abs() >= Q_GAP * q.abs().max()).numpy()}
        if act == "relu":
            f = twin64._features(tobs)
            worst = _margins(twin64.actor.latent_pi, f)
            for x in (torch.cat([f, a], dim=1), torch.cat([f, _t(twin64, actions)], dim=1)):
                for net in (twin64.critic.qf0, twin64.critic.qf1):
                    worst = torch.minimum(worst, _margins(net, x))
            ok["relu_margin"] = (worst >= RELU_MARGIN).numpy()
    return ok, (q[1] < q[0]).numpy()


def make_batch(twin64, D: int, A: int, B: int, seed: int, noise_seed: int, calls=(0, 0)):
    """-> (isac.Batch of float32 numpy arrays, eps_target, eps_actor, census).  The noises are the restated Philox's of domains 8 and 9
    at the call numbers ``calls``.  Every row meets ``row_conditions`` (a failing row's observation and achieved goal are drawn again
    from the next seed; none is left out), the next observations meet indep_sac's conditions under eps_target, both clamps act in some
    rows (B >= 75), and each critic is the smaller one in at least 8 of the first 75 rows: where the twin's critics do not give that,
    ``twin64``'s qf1 head bias is shifted, in place, by the median of q0 - q1 (the census says by how much)."""
    act = twin64.activation
    eps_t = isac.noise(isac.DOMAIN_TARGET, noise_seed, calls[0], B, A)
    eps_a = isac.noise(DOMAIN_ACTOR_LOSS, noise_seed, calls[1], B, A)
    batch = isac.replay_batch(twin64.numpy_state(), act, B, D, A, seed, eps_t)
    obs = {k: v.copy() for k, v in batch.observations.items()}
    head = twin64.critic.qf1[-1]
    shift = 0.0
    if B >= FIRST_ROWS:
        with torch.no_grad():
            tobs = _obs(twin64, obs)
            q = twin64.q(tobs, twin64.action_log_prob(tobs, _t(twin64, eps_a))[0])[:, :FIRST_ROWS]
            n1 = int((q[1] < q[0]).sum())
            if min(n1, FIRST_ROWS - n1) < 2 * MIN_EACH:
                shift = float((q[0] - q[1]).median())
                head.bias.add_(shift)
                head.bias.copy_(head.bias.float().double())      # (the weights stay float32 numbers)
    for attempt in range(1, 400):
        ok, _ = row_conditions(twin64, obs, batch.actions, eps_a)
        bad = ~np.logical_and.reduce(list(ok.values()))
        if not bad.any():
            break
        fresh = isac.random_obs(B, D, seed + 104729 * attempt)
        for k in ("observation", "achieved_goal"):
            obs[k][bad] = fresh[k][bad].astype(np.float32)
    ok, second = row_conditions(twin64, obs, batch.actions, eps_a)
    assert all(v.all() and len(v) == B for v in ok.values()), {k: int((~v).sum()) for k, v in ok.items()}
    raw = isac.actor_rule(twin64.numpy_state(), isac.round32(obs), act)[2]
    census = {"attempts": attempt, "bias_shift": shift, "qf1_smaller_in_first_rows": int(second[:FIRST_ROWS].sum()),
              "lower_clamp_rows": int((raw < isac.LOG_STD_MIN).any(axis=1).sum()), "upper_clamp_rows": int((raw > isac.LOG_STD_MAX).any(axis=1).sum())}
    if B >= FIRST_ROWS:
        n1 = census["qf1_smaller_in_first_rows"]
        assert MIN_EACH <= n1 <= FIRST_ROWS - MIN_EACH, census
        assert census["lower_clamp_rows"] > 0 and census["upper_clamp_rows"] > 0, census
    assert isac.conditions(twin64.numpy_state(), batch.next_observations, eps_t, act).all()
    return batch._replace(observations=obs), eps_t, eps_a, census


# The trunks and sizes the GPU tests use: (D, A, trunk name of TRUNKS, B)
TRUNKS = {"64x64-relu": ((64, 64), (64, 64), "relu"), "48x32-tanh-qf16": ((48, 32), (16,), "tanh"), "16-tanh": ((16,), (16,), "tanh"),
          "256x256-relu": ((256, 256), (256, 256), "relu"),
          # the shape edges of tests/policy_shape_cases.py
          "32x48x16-tanh-16x48x32": ((32, 48, 16), (16, 48, 32), "tanh"), "80x16x112-relu-96x240x16": ((80, 16, 112), (96, 240, 16), "relu"),
          "32-relu-80": ((32,), (80,), "relu"), "144x16-tanh-48": ((144, 16), (48,), "tanh"), "64x64x64-relu": ((64, 64, 64), (64, 64, 64), "relu")}
SHAPES = [(D, A, name) for (D, A) in isac.DIMS for name in ("64x64-relu", "48x32-tanh-qf16", "16-tanh")] + [(25, 4, "256x256-relu")]
GRAD_CASES = [(D, A, t, 75) for D, A, t in SHAPES] + [(D, A, t, B) for (D, A, t) in ((10, 7, "64x64-relu"), (25, 8, "48x32-tanh-qf16"),
                                                                                      (25, 4, "256x256-relu")) for B in (600, 1)]
WEIGHTS_SEED, BATCH_SEED, NOISE_SEED = 3, 5, 21


def twins(D, A, trunk, weights_seed=WEIGHTS_SEED):
    """(float32 twin, float64 twin) with the same random weights; the float32 one is the float64 one's rounding."""
    pi, qf, act = TRUNKS[trunk]
    t64 = isac.Twin(D, A, pi, qf, act).randomize(weights_seed, D).double()
    return isac.Twin(D, A, pi, qf, act), t64


def case(D, A, trunk, B, calls=(0, 0)):
    """-> (twin32, twin64, batch, eps_target, eps_actor, census): the maker run on fresh twins (the bias shift, where one is made, is in
    both twins)."""
    t32, t64 = twins(D, A, trunk)
    # the weights are float32 numbers held in float64, so that the three implementations start from the same values
    made = make_batch(t64, D, A, B, BATCH_SEED, NOISE_SEED, calls)
    t32.load_state_dict({k: v.float() for k, v in t64.state_dict().items()})
    return (t32, t64) + made
