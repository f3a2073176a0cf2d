#!/usr/bin/env python3
"""Device-event timing of the policy update (mycobotgym_amd.PPOUpdate) against the same update in eager PyTorch, and of one full PPO
iteration with each.

    python tools/policy_update_bench.py [--envs 8192] [--batch 4096] [--reps 20] [--inner 50] [--out profiles/policy_update/policy_update_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream; reported: median and min / max of the per-call time.  Shapes: (D, A) = (10, 7) and (25, 4), trunks (64, 64) tanh and
(256, 256) relu, minibatches of `batch` samples.

    step            opt.step(mb): mcg_policy_grad + mcg_policy_adam, the public call, Python included
    grad / adam     its two entries alone (opt.compute_grad(mb), opt.apply())
    evaluate        pol.evaluate_actions(mb.observations, mb.actions)
    twin_step       the path users had: the torch twin (tests/indep_policy.py: SB3's formula in eager float32 on the GPU) forward, SB3's
                    loss, backward, clip_grad_norm_, torch.optim.Adam.step, zero_grad
    twin_step_load  the same followed by pol.load_state_dict(twin.state_dict()), so that the HIP forward sees the new weights
    iteration       one PPO iteration on MyCobotReach-Dense-joint-v0: 64 collection steps (policy -> step -> RolloutBuffer.add), finish,
                    10 epochs of minibatches; collection and update timed apart; iteration_twin: the update by the twin with the repack
                    after every minibatch's step (its collection is the same HIP loop)
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
from tests.indep_policy import Twin, random_obs  # noqa: E402

ENV_ID = "MyCobotReach-Dense-joint-v0"
SHAPES = ((10, 7), (25, 4))
TRUNKS = (((64, 64), "tanh"), ((256, 256), "relu"))
CLIP, ENT, VF, MAX_NORM = 0.2, 0.0, 0.5, 0.5


def twin_loss(twin, mb):
    """SB3's PPO loss on one minibatch, eager float32."""
    value, log_prob, entropy = twin.evaluate_actions(mb.observations, mb.actions)
    adv = mb.advantages
    adv = (adv - adv.mean()) / (adv.std() + 1e-8)
    ratio = torch.exp(log_prob - mb.old_log_prob)
    policy_loss = -torch.min(adv * ratio, adv * torch.clamp(ratio, 1 - CLIP, 1 + CLIP)).mean()
    return policy_loss + ENT * -entropy.mean() + VF * torch.nn.functional.mse_loss(mb.returns, value)


def twin_updater(twin, pol=None):
    opt = torch.optim.Adam(twin.parameters(), lr=3e-4, eps=1e-5)

    def step(mb):
        twin_loss(twin, mb).backward()
        torch.nn.utils.clip_grad_norm_(twin.parameters(), MAX_NORM)
        opt.step()
        opt.zero_grad(set_to_none=True)
        if pol is not None:
            pol.load_state_dict(twin.state_dict())
    return step


def random_minibatch(B, D, A, dev):
    obs = {k: torch.from_numpy(v).float().to(dev) for k, v in random_obs(B, D, seed=0).items()}
    gen = torch.Generator(device="cpu").manual_seed(0)
    r = lambda *shape: torch.randn(*shape, generator=gen).to(dev)
    return mg.RolloutSamples(observations=obs, actions=r(B, A), old_values=r(B), old_log_prob=r(B) * 0.1 - 1.2 * A, advantages=r(B),
                             returns=r(B), index=torch.zeros(B, dtype=torch.int32, device=dev))


def windows(fn, reps):
    """`fn` once per window between two events -> ms per window."""
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); fn(); b.record(); b.synchronize()
        ms.append(a.elapsed_time(b))
    ms.sort()
    return {"median_ms": ms[len(ms) // 2], "min_ms": ms[0], "max_ms": ms[-1], "reps": reps}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--batch", type=int, default=4096)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--iterations", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_update_bench needs the GPU: a timing taken anywhere else says nothing")
    n, B, dev = args.envs, args.batch, torch.device("cuda:0")
    t = lambda fn: timed(fn, warmup=10, reps=args.reps, inner=args.inner)
    cases = []

    def report(what, r, **kw):
        r.update(what=what, batch=B, device=torch.cuda.get_device_name(0), **kw)
        cases.append(r)
        print(json.dumps(r), flush=True)

    for D, A in SHAPES:
        mb = random_minibatch(B, D, A, dev)
        for hidden, act in TRUNKS:
            twin = Twin(D, A, hidden, hidden, act).randomize(0).to(dev)
            pol = mg.ActorCritic.from_module(twin, num_envs=n, obs_dim=D, act_dim=A, device=dev)
            opt = mg.PPOUpdate(pol, clip_range=CLIP, ent_coef=ENT, vf_coef=VF, max_grad_norm=MAX_NORM)
            kw = dict(obs_dim=D, act_dim=A, hidden=list(hidden), activation=act)
            report("step", t(lambda: opt.step(mb)), **kw)
            report("grad", t(lambda: opt.compute_grad(mb)), **kw)
            report("adam", t(lambda: opt.apply()), **kw)
            report("evaluate", t(lambda: pol.evaluate_actions(mb.observations, mb.actions)), **kw)
            report("twin_step", t(lambda f=twin_updater(twin): f(mb)), **kw)
            report("twin_step_load", t(lambda f=twin_updater(twin, pol): f(mb)), **kw)

    # ---- one PPO iteration on the engine
    T, epochs = 64, 10
    envs = mg.make(ENV_ID, num_envs=n, seed=1)
    D, A = envs.obs_dim, envs.action_dim
    for hidden, act in TRUNKS:
        for name in ("iteration", "iteration_twin"):
            twin = Twin(D, A, hidden, hidden, act).randomize(0).to(dev)
            pol = mg.ActorCritic.from_module(twin, envs)
            update = mg.PPOUpdate(pol).step if name == "iteration" else twin_updater(twin, pol)
            buf = mg.RolloutBuffer(envs, n_steps=T, seed=0)
            obs, _ = envs.reset(seed=1)
            buf.start(obs)
            state = {"obs": obs}

            def collect():
                buf.reset()
                obs = state["obs"]
                with torch.no_grad():
                    for _ in range(T):
                        a, v, logp = pol(obs)
                        obs, r, term, trunc, info = envs.step(a)
                        buf.add(a, v, logp, obs, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
                    buf.finish(last_values=pol.values(obs))
                state["obs"] = obs

            def train():
                for _ in range(epochs):
                    for mb in buf.get(B):
                        update(mb)

            collect(); train(); torch.cuda.synchronize()          # warm-up
            col, upd = [], []
            for _ in range(args.iterations):
                col.append(windows(collect, 1)["median_ms"])
                upd.append(windows(train, 1)["median_ms"])
            col.sort(); upd.sort()
            report(name, {"collect_ms": col[len(col) // 2], "update_ms": upd[len(upd) // 2], "update_min_ms": upd[0], "update_max_ms": upd[-1],
                          "minibatches": epochs * -(-n * T // B), "reps": args.iterations},
                   env_id=ENV_ID, envs=n, hidden=list(hidden), activation=act, n_steps=T, epochs=epochs)
    envs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"cases": cases}, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
