#!/usr/bin/env python3
"""Device-event timing of TD3 / DDPG on the device (mycobotgym_amd.TD3Policy, TD3Update) against the same rule in eager PyTorch and
against SACUpdate.step at the same shape, and of the collection-plus-update loop beside the bare Reach step.

    python tools/td3_bench.py [--envs 8192] [--reps 20] [--inner 50] [--out profiles/td3/td3_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream; reported: median and min / max of the per-call time (min / max over the windows: the run's own repeat-to-repeat spread).
`inner` is even, so a TD3 figure averages steps with and without the delayed actor update.  Shapes: (D, A) = (10, 7) and (25, 4),
trunks (64, 64) and (256, 256) relu, batches of 256, 4096 and 65536 rows.

    act             pol(obs) at --envs environments
    target / q / polyak      pol.td_target, pol.q_values, pol.polyak: one launch each (polyak: two)
    step            TD3Update.step(batch), policy_delay = 2: the public call, Python included
    ddpg_step       DDPGUpdate.step on a DDPGPolicy (one critic, the actor every step)
    sac_step        SACUpdate.step at the same shape and batch, timed right after `step` in the same run
    twin_step_load  the path users had: tests/indep_td3.py's Twin in eager float32 on the GPU -- the target, two losses, two backward
                    passes, two torch.optim.Adam steps (the actor's every second call), two Polyak loops -- then
                    TD3Policy.load_state_dict, so that the HIP forward sees the new weights
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
from tests.indep_sac import Twin as SacTwin  # noqa: E402
from tests.indep_td3 import Twin, random_obs  # noqa: E402

ENV_ID = "MyCobotReach-Dense-joint-v0"
SHAPES = ((10, 7), (25, 4))
TRUNKS = ((64, 64), (256, 256))
BATCHES = (256, 4096, 65536)
GAMMA, TAU, LR, SIGMA, CLIP, DELAY = 0.99, 0.005, 1e-3, 0.2, 0.5, 2


def twin_updater(twin, pol, A):
    """One gradient step of SB3's TD3.train on the twin, eager float32, then the repack."""
    opts = [torch.optim.Adam(twin.critic.parameters(), lr=LR), torch.optim.Adam(twin.actor.parameters(), lr=LR)]
    count = {"n": 0}

    def step(b):
        B = b.actions.shape[0]
        count["n"] += 1
        with torch.no_grad():
            n = (torch.randn(B, A, device=pol.device) * SIGMA).clamp(-CLIP, CLIP)
            a = (twin.act(b.next_observations, target=True) + n).clamp(-1.0, 1.0)
            q = torch.min(twin.q(b.next_observations, a, target=True), dim=0).values
            y = b.rewards.flatten() + (1.0 - b.dones.flatten()) * GAMMA * q
        q = twin.q(b.observations, b.actions)
        critic_loss = sum(torch.nn.functional.mse_loss(q[k], y) for k in range(twin.n_critics))
        opts[0].zero_grad(set_to_none=True); critic_loss.backward(); opts[0].step()
        if count["n"] % DELAY == 0:
            actor_loss = -twin.q(b.observations, twin.act(b.observations))[0].mean()
            opts[1].zero_grad(set_to_none=True); actor_loss.backward(); opts[1].step()
            with torch.no_grad():
                for net, tgt in ((twin.critic, twin.critic_target), (twin.actor, twin.actor_target)):
                    for c, t in zip(net.parameters(), tgt.parameters()):
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
    ap.add_argument("--batches", type=int, nargs="*", default=list(BATCHES))
    ap.add_argument("--no-twin", action="store_true", help="skip the eager PyTorch figures")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if args.inner % 2:
        sys.exit("--inner must be even: a TD3 figure averages steps with and without the actor update")
    if not torch.cuda.is_available():
        sys.exit("td3_bench needs the GPU: a timing taken anywhere else says nothing")
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
            twin = Twin(D, A, hidden, hidden, "relu", 2).randomize(0).to(dev)
            pol = mg.TD3Policy.from_module(twin, num_envs=n, obs_dim=D, act_dim=A, device=dev)
            obs = {k: torch.from_numpy(v).to(dev) for k, v in random_obs(n, D, seed=2).items()}
            kw = dict(obs_dim=D, act_dim=A, hidden=list(hidden), activation="relu")
            report("act", t(lambda: pol(obs, noise_std=0.1)), envs=n, **kw)
            for B in args.batches:
                b = random_batch(B, D, A, dev)
                kw["batch"] = B
                opt = mg.TD3Update(pol, learning_rate=LR, gamma=GAMMA, tau=TAU, policy_delay=DELAY, target_policy_noise=SIGMA, target_noise_clip=CLIP)
                sac = mg.SACPolicy.from_module(SacTwin(D, A, hidden, hidden, "relu").randomize(0, D), num_envs=n, obs_dim=D, act_dim=A, device=dev)
                sac_opt = mg.SACUpdate(sac, gamma=GAMMA, tau=TAU)
                report("step", t(lambda: opt.step(b)), **kw)
                report("sac_step", t(lambda: sac_opt.step(b)), **kw)
                report("step", t(lambda: opt.step(b)), again=True, **kw)          # (the pair once more, the other way round)
                y = opt._rows[B]
                report("target", t(lambda: pol.td_target(b, GAMMA, SIGMA, CLIP, out={"target": y})), **kw)
                q = torch.empty(2, B, device=dev)
                report("q", t(lambda: pol.q_values(b.observations, b.actions, out=q)), **kw)
                report("polyak", t(lambda: pol.polyak(TAU)), **kw)
                ddpg = mg.DDPGPolicy(num_envs=n, obs_dim=D, act_dim=A, hidden=hidden, device=dev)
                dopt = mg.DDPGUpdate(ddpg, learning_rate=LR, gamma=GAMMA, tau=TAU)
                report("ddpg_step", t(lambda: dopt.step(b)), **kw)
                if not args.no_twin:
                    report("twin_step_load", t(lambda f=twin_updater(twin, pol, A): f(b)), **kw)
                    pol.load_state_dict(twin.state_dict())

    # ---- the off-policy loop on the engine
    envs = mg.make(ENV_ID, num_envs=n, seed=1)
    obs0, _ = envs.reset(seed=1)
    a0 = torch.rand(n, envs.action_dim, device=dev) * 2 - 1
    report("env_step", t(lambda: envs.step_async(a0)), env_id=ENV_ID, envs=n)
    for hidden in TRUNKS:
        pol = mg.TD3Policy(envs, hidden=hidden, activation="relu", seed=0)
        opt = mg.TD3Update(pol)
        buf = mg.HerBuffer(envs, capacity=2 * envs.max_episode_steps, seed=0)
        buf.start(obs0)
        state = {"obs": obs0}

        def one_step():
            a = pol(state["obs"], noise_std=0.1)
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
