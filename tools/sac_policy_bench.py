#!/usr/bin/env python3
"""Device-event timing of SAC's gradient-free half (mycobotgym_amd.SACPolicy) against the same policy in eager PyTorch, and of the
off-policy collection loop.

    python tools/sac_policy_bench.py [--envs 8192] [--reps 20] [--inner 50] [--out profiles/sac_policy/sac_policy_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream (reps * inner >= 1000 calls); reported: median and min / max of the per-call time.  Shapes: (D, A) = (10, 7) and (25, 4), actor
and critics (256, 256) relu (SB3's default) and (64, 64) relu.

    act             a = pol(obs) at `envs` environments: the public call, output allocation and Python included
    td_target       y = pol.td_target(batch) at B = 256 (SB3's default batch), 4096 and 65536: one launch
    q_values        pol.q_values(batch.observations, batch.actions) at the same B
    polyak          pol.polyak(0.005)
    twin_*          the torch twin (tests/indep_sac.py: SB3's formula in eager float32 on the same GPU) producing the same outputs;
                    twin_act and twin_td_target include drawing the twin's noise (one torch.randn launch per call, as SB3's rsample
                    draws it; the kernels draw theirs inside the launch); twin_polyak is SB3's polyak_update loop over the critics'
                    parameters
    alt_act_plus_q  a stand-in for the three-launch alternative to the fused target, without its combine step: pol(obs) at B rows
                    with the outputs the target line needs (action, log_prob) plus q_values on the target blob: the sum of two
                    measured medians.  The actor part reads float64 engine-style observations where the real alternative would read
                    the batch's float32 rows, so its first layer loads twice the bytes: a slight overestimate of that part, while the
                    missing combine launch makes the sum an underestimate
    step            the bare Reach step (step_async)
    loop            one step of the collection loop on MyCobotReach-Dense-joint-v0: pol -> step_async -> HerBuffer.add
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
from tests.indep_sac import Batch, Twin, random_obs  # noqa: E402

ENV_ID = "MyCobotReach-Dense-joint-v0"
SHAPES = ((10, 7), (25, 4))
TRUNKS = ((256, 256), (64, 64))
BATCHES = (256, 4096, 65536)


def random_batch(B, D, A, dev, seed=0):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen).to(dev)
    obs = {"observation": r(B, D) * 0.7, "achieved_goal": r(B, 3) * 0.2, "desired_goal": r(B, 3) * 0.2}
    nxt = {"observation": r(B, D) * 0.7, "achieved_goal": r(B, 3) * 0.2, "desired_goal": obs["desired_goal"]}
    return Batch(observations=obs, actions=torch.rand(B, A, generator=gen).to(dev) * 2 - 1, next_observations=nxt,
                 dones=(torch.rand(B, 1, generator=gen) < 0.1).float().to(dev), rewards=r(B, 1))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("sac_policy_bench needs the GPU: a timing taken anywhere else says nothing")
    n, dev = args.envs, torch.device("cuda:0")
    t = lambda fn, inner=args.inner: timed(fn, warmup=10, reps=args.reps, inner=inner)
    cases = []

    def report(what, r, **kw):
        r.update(what=what, device=torch.cuda.get_device_name(0), **kw)
        cases.append(r)
        print(json.dumps(r), flush=True)
        return r["median_ms"]

    def polyak_twin(twin, tau=0.005):          # SB3's polyak_update
        for p, tp in zip(twin.critic.parameters(), twin.critic_target.parameters()):
            tp.data.mul_(1 - tau)
            torch.add(tp.data, p.data, alpha=tau, out=tp.data)

    for D, A in SHAPES:
        obs = {k: torch.from_numpy(v).to(dev) for k, v in random_obs(n, D, seed=0).items()}
        for hidden in TRUNKS:
            twin = Twin(D, A, hidden, hidden, "relu").to(dev)
            pol = mg.SACPolicy.from_module(twin, num_envs=n, obs_dim=D, act_dim=A, device=dev)
            kw = dict(obs_dim=D, act_dim=A, hidden=list(hidden), activation="relu")
            with torch.no_grad():
                report("act", t(lambda: pol(obs)), envs=n, **kw)
                report("twin_act", t(lambda: twin.action_log_prob(obs, torch.randn(n, A, device=dev))[0]), envs=n, **kw)
                report("polyak", t(lambda: pol.polyak(0.005)), **kw)
                report("twin_polyak", t(lambda: polyak_twin(twin)), **kw)
                for B in BATCHES:
                    b = random_batch(B, D, A, dev)
                    nxt, r, d = b.next_observations, b.rewards, b.dones
                    report("td_target", t(lambda: pol.td_target(b, gamma=0.99)), batch=B, **kw)
                    report("twin_td_target", t(lambda: twin.target(nxt, r, d, torch.randn(B, A, device=dev), 0.99, 0.2)["target"]), batch=B, **kw)
                    q = report("q_values", t(lambda: pol.q_values(b.observations, b.actions, target=True)), batch=B, **kw)
                    report("twin_q_values", t(lambda: twin.q(b.observations, b.actions, target=True)), batch=B, **kw)
                    wide = mg.SACPolicy.from_module(twin, num_envs=B, obs_dim=D, act_dim=A, device=dev)
                    wobs = {k: torch.from_numpy(v).to(dev) for k, v in random_obs(B, D, seed=1).items()}
                    wout = wide._new("action", "log_prob")
                    a = t(lambda: wide(wobs, out=wout))["median_ms"]
                    report("alt_act_plus_q", {"median_ms": a + q, "act_ms": a, "q_ms": q}, batch=B, **kw)

    envs = mg.make(ENV_ID, num_envs=n, seed=1)
    obs0, _ = envs.reset(seed=1)
    a0 = torch.rand(n, envs.action_dim, device=dev) * 2 - 1
    report("step", t(lambda: envs.step_async(a0)), env_id=ENV_ID, envs=n)
    for hidden in TRUNKS:
        pol = mg.SACPolicy(envs, hidden=hidden, activation="relu", seed=0)
        buf = mg.HerBuffer(envs, capacity=2 * envs.max_episode_steps, seed=0)
        buf.start(obs0)
        state = {"obs": obs0}

        def one_step():
            a = pol(state["obs"])
            b = envs.step_async(a)
            state["obs"] = {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}
            final = {"observation": b["final_obs"], "achieved_goal": b["final_achieved"], "desired_goal": b["final_desired"]}
            buf.add(a, state["obs"], b["reward"], b["terminated"], b["truncated"], {"final_observation": final})
        with torch.no_grad():
            report("loop", t(one_step), env_id=ENV_ID, envs=n, hidden=list(hidden), activation="relu")
    envs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"cases": cases}, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
