#!/usr/bin/env python3
"""Device-event timing of SAC's update (mycobotgym_amd.SACUpdate) against the same gradient step in eager PyTorch, and of the
collection-plus-update loop beside the bare Reach step.

    python tools/sac_update_bench.py [--envs 8192] [--reps 20] [--inner 50] [--out profiles/sac_update/sac_update_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream; reported: median and min / max of the per-call time.  Shapes: (D, A) = (10, 7) and (25, 4), trunks (64, 64) and (256, 256)
relu, batches of 256, 4096 and 65536 rows.

    step            opt.step(batch): the public call, Python included (td_target, critic gradient + Adam, actor gradient + Adam, the
                    alpha step, polyak: 11 launches)
    target / critic / actor / alpha / polyak      its launch groups alone
    twin_step_load  the path users had, in the same process: tests/indep_sac.py's Twin in eager float32 on the GPU -- the target, the
                    three losses, backward, three torch.optim.Adam steps, the Polyak update -- then SACPolicy.load_state_dict, so
                    that the HIP forward sees the new weights
    env_step        the bare Reach step (step_async)
    loop            one step of off-policy training on MyCobotReach-Dense-joint-v0: pol -> step_async -> HerBuffer.add -> sample(256)
                    -> opt.step
"""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
import mycobotgym_amd as mg  # noqa: E402
from _timing import timed  # noqa: E402
from tests.indep_sac import EPSILON, LOG_SQRT_2PI, Twin, random_obs  # noqa: E402

ENV_ID = "MyCobotReach-Dense-joint-v0"
SHAPES = ((10, 7), (25, 4))
TRUNKS = ((64, 64), (256, 256))
BATCHES = (256, 4096, 65536)
GAMMA, TAU, LR = 0.99, 0.005, 3e-4


def twin_updater(twin, pol, A):
    """One gradient step of SB3's SAC.train on the twin, eager float32, then the repack."""
    log_ent_coef = torch.zeros(1, device=pol.device, requires_grad=True)
    opts = [torch.optim.Adam(twin.critic.parameters(), lr=LR), torch.optim.Adam(twin.actor.parameters(), lr=LR), torch.optim.Adam([log_ent_coef], lr=LR)]

    def step(b):
        B = b.actions.shape[0]
        alpha = log_ent_coef.detach().exp()
        with torch.no_grad():
            y = twin.target(b.next_observations, b.rewards, b.dones, torch.randn(B, A, device=pol.device), GAMMA, alpha)["target"]
        q = twin.q(b.observations, b.actions)
        critic_loss = 0.5 * (torch.nn.functional.mse_loss(q[0], y) + torch.nn.functional.mse_loss(q[1], y))
        opts[0].zero_grad(set_to_none=True); critic_loss.backward(); opts[0].step()
        a, logp, *_ = twin.action_log_prob(b.observations, torch.randn(B, A, device=pol.device))
        actor_loss = (alpha * logp - torch.min(twin.q(b.observations, a), dim=0).values).mean()
        opts[1].zero_grad(set_to_none=True); actor_loss.backward(); opts[1].step()
        ent_coef_loss = -(log_ent_coef * (logp.detach() - float(A))).mean()
        opts[2].zero_grad(set_to_none=True); ent_coef_loss.backward(); opts[2].step()
        with torch.no_grad():
            for c, t in zip(twin.critic.parameters(), twin.critic_target.parameters()):
                t.mul_(1.0 - TAU).add_(c, alpha=TAU)
        pol.load_state_dict(twin.state_dict())
    return step


def random_batch(B, D, A, dev):
    gen = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    obs = {k: torch.from_numpy(v).float().to(dev) for k, v in random_obs(B, D, seed=0).items()}
    nxt = {k: torch.from_numpy(v).float().to(dev) for k, v in random_obs(B, D, seed=1).items()}
    nxt["desired_goal"] = obs["desired_goal"]
    return mg.HerSamples(observations=obs, actions=torch.tanh(r(B, A)), next_observations=nxt, dones=(r(B, 1) > 0.5).float(), rewards=r(B, 1),
                         index=torch.zeros(B, dtype=torch.int64, device=dev))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sac_update_bench needs the GPU: a timing taken anywhere else says nothing")
    n, dev = args.envs, torch.device("cuda:0")
    t = lambda fn: timed(fn, warmup=10, reps=args.reps, inner=args.inner)
    cases = []

    def report(what, r, **kw):
        r.update(what=what, device=torch.cuda.get_device_name(0), **kw)
        cases.append(r)
        print(json.dumps(r), flush=True)
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                json.dump({"cases": cases}, f, indent=1); f.write("\n")

    for D, A in SHAPES:
        for hidden in TRUNKS:
            twin = Twin(D, A, hidden, hidden, "relu").randomize(0, D).to(dev)
            for B in BATCHES:
                b = random_batch(B, D, A, dev)
                pol = mg.SACPolicy.from_module(twin, num_envs=n, obs_dim=D, act_dim=A, device=dev)
                opt = mg.SACUpdate(pol, learning_rate=LR, gamma=GAMMA, tau=TAU)
                kw = dict(obs_dim=D, act_dim=A, hidden=list(hidden), activation="relu", batch=B)
                report("step", t(lambda: opt.step(b)), **kw)
                _, rows, _keep, work, y, logp = opt._inputs(b)
                report("target", t(lambda: pol.td_target(b, gamma=GAMMA, out={"target": y})), **kw)
                report("critic", t(lambda: (opt._critic_grad(rows, y, B, work), opt._adam("critic"))), **kw)
                report("actor", t(lambda: (opt._actor_grad(rows, logp, B, work), opt._adam("actor"))), **kw)
                report("alpha", t(lambda: opt._alpha_step(logp, B, LR)), **kw)
                report("polyak", t(lambda: pol.polyak(TAU)), **kw)
                report("twin_step_load", t(lambda f=twin_updater(twin, pol, A): f(b)), **kw)

    # ---- the off-policy loop on the engine
    envs = mg.make(ENV_ID, num_envs=n, seed=1)
    obs0, _ = envs.reset(seed=1)
    a0 = torch.rand(n, envs.action_dim, device=dev) * 2 - 1
    report("env_step", t(lambda: envs.step_async(a0)), env_id=ENV_ID, envs=n)
    for hidden in TRUNKS:
        pol = mg.SACPolicy(envs, hidden=hidden, activation="relu", seed=0)
        opt = mg.SACUpdate(pol)
        buf = mg.HerBuffer(envs, capacity=2 * envs.max_episode_steps, seed=0)
        buf.start(obs0)
        state = {"obs": obs0}

        def one_step():
            a = pol(state["obs"])
            b = envs.step_async(a)
            state["obs"] = {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}
            final = {"observation": b["final_obs"], "achieved_goal": b["final_achieved"], "desired_goal": b["final_desired"]}
            buf.add(a, state["obs"], b["reward"], b["terminated"], b["truncated"], {"final_observation": final})
            opt.step(buf.sample(256, check=False))
        with torch.no_grad():
            report("loop", t(one_step), env_id=ENV_ID, envs=n, hidden=list(hidden), activation="relu", batch=256)
    envs.close()


if __name__ == "__main__":
    main()
