#!/usr/bin/env python3
"""Device-event timing of the actor-critic policy forward (mycobotgym_amd.ActorCritic) against the same policy in eager PyTorch, and of
the on-policy collection loop with each.

    python tools/policy_bench.py [--envs 8192] [--reps 20] [--inner 50] [--out profiles/policy/policy_bench.json]

One GPU, one process.  Every figure: warm-up calls, then `reps` windows of `inner` back-to-back calls between two events on the launch
stream (reps * inner >= 1000 calls); reported: median and min / max of the per-call time.  Shapes: (D, A) = (10, 7) and (25, 4), trunks
(64, 64) tanh and (256, 256) relu.

    forward          a, v, logp = pol(obs): the public call, output allocation and Python included
    values           pol.values(obs)
    load_state_dict  pol.load_state_dict(sd): the repack after an optimiser update (plain torch ops; off the step path)
    twin_forward     the torch twin (tests/indep_policy.py: SB3's formula in eager float32 on the GPU) producing the same three outputs
    twin_values      its value net alone
    step             the bare Reach step (step_async)
    loop             one step of a 64-step collection loop on MyCobotReach-Dense-joint-v0: policy -> step_async -> RolloutBuffer.add
                     with values of the final observation; loop_twin: the same with the twin
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--envs", type=int, default=8192)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--inner", type=int, default=50)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("policy_bench needs the GPU: a timing taken anywhere else says nothing")
    n, dev = args.envs, torch.device("cuda:0")
    t = lambda fn, inner=args.inner: timed(fn, warmup=10, reps=args.reps, inner=inner)
    cases = []

    def report(what, r, **kw):
        r.update(what=what, envs=n, device=torch.cuda.get_device_name(0), **kw)
        cases.append(r)
        print(json.dumps(r), flush=True)

    for D, A in SHAPES:
        obs = {k: torch.from_numpy(v).to(dev) for k, v in random_obs(n, D, seed=0).items()}
        for hidden, act in TRUNKS:
            twin = Twin(D, A, hidden, hidden, act).randomize(0).to(dev)
            pol = mg.ActorCritic.from_module(twin, num_envs=n, obs_dim=D, act_dim=A, device=dev)
            sd = twin.state_dict()
            kw = dict(obs_dim=D, act_dim=A, hidden=list(hidden), activation=act)
            with torch.no_grad():
                report("forward", t(lambda: pol(obs)), **kw)
                report("values", t(lambda: pol.values(obs)), **kw)
                report("load_state_dict", t(lambda: pol.load_state_dict(sd)), **kw)
                report("twin_forward", t(lambda: twin(obs)), **kw)
                report("twin_values", t(lambda: twin.predict_values(obs)), **kw)

    envs = mg.make(ENV_ID, num_envs=n, seed=1)
    obs0, _ = envs.reset(seed=1)
    a0 = torch.rand(n, envs.action_dim, device=dev) * 2 - 1
    report("step", t(lambda: envs.step_async(a0)), env_id=ENV_ID)
    D, A, T = envs.obs_dim, envs.action_dim, 64
    for hidden, act in TRUNKS:
        twin = Twin(D, A, hidden, hidden, act).randomize(0).to(dev)
        pol = mg.ActorCritic.from_module(twin, envs)
        for name, policy, value_fn in (("loop", lambda o: pol(o), pol.values),
                                       ("loop_twin", lambda o: twin(o)[:3], twin.predict_values)):
            buf = mg.RolloutBuffer(envs, n_steps=T, seed=0)
            buf.start(obs0)
            state = {"obs": obs0}

            def one_step():
                if buf.full:
                    buf.reset()
                a, v, logp = policy(state["obs"])
                b = envs.step_async(a.clamp(-1, 1) if name == "loop_twin" else a)      # (the engine clips what it reads: the clamp is the twin's launch, as SB3 clips)
                state["obs"] = {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}
                final = {"observation": b["final_obs"], "achieved_goal": b["final_achieved"], "desired_goal": b["final_desired"]}
                buf.add(a, v, logp, state["obs"], b["reward"], b["terminated"], b["truncated"], None, final_values=value_fn(final))
            with torch.no_grad():
                report(name, t(one_step, inner=T), env_id=ENV_ID, hidden=list(hidden), activation=act, n_steps=T)
    envs.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump({"cases": cases}, f, indent=1); f.write("\n")


if __name__ == "__main__":
    main()
