"""The actor-critic policy forward on the GPU (mycobotgym_amd/policy.py, csrc/mcg_policy.hip) against the restated rule and its torch
twin (tests/indep_policy.py).  N = 40 is two full tiles of 16 environments and one of 8 rows.

Bound of the parity tests, per case and per output: 10 x the largest error of the twin's CPU float32 forward against the float64 rule
on the same float32-rounded inputs, the maximum over the case's rows (the project's "10 x a twin" margin: it covers another order of
summation and another tanhf).  The measured ratios are in profiles/policy/parity.md."""
import functools

import numpy as np
import pytest
import torch

from tests import indep_policy as ip

pytestmark = pytest.mark.gpu

N, SEED = 40, 21
CASES = [(D, A, name) for (D, A) in ip.DIMS for name in ("64x64-tanh", "48x32-relu-vf16", "16-tanh")] + [(25, 4, "256x256-relu")]
NAMES = ("action", "value", "log_prob", "mean", "noise")


def dev(obs: dict) -> dict:
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in obs.items()}


def policy_for(D, A, trunk, weights_seed=3, n=N, **kw):
    from mycobotgym_amd import ActorCritic
    pi, vf, act = ip.TRUNKS[trunk]
    twin = ip.Twin(D, A, pi, vf, act).randomize(weights_seed)
    pol = ActorCritic(num_envs=n, obs_dim=D, act_dim=A, hidden=dict(pi=pi, vf=vf), activation=act, seed=SEED, **kw)
    pol.load_state_dict(twin.state_dict())
    return pol, twin


def run(pol, obs: dict, deterministic=False) -> dict:
    """All five outputs of one call as numpy arrays."""
    out = pol._new(*NAMES)
    pol.forward(dev(obs), deterministic=deterministic, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a: dict, b: dict, rows=slice(None), names=NAMES):
    for k in names:
        assert np.array_equal(bits(a[k]), bits(b[k][rows])), k


@functools.lru_cache(maxsize=None)
def reference(D, A, trunk, weights_seed=3, call=0, n=N):
    """Computed once per case and shared: the inputs, the float64 rule on their float32 roundings, the twin's float32 forward with
    the restated noise of call `call`, and the twin's errors, which are the bounds' yardstick."""
    pi, vf, act = ip.TRUNKS[trunk]
    twin = ip.Twin(D, A, pi, vf, act).randomize(weights_seed)
    sd = twin.numpy_state()
    obs = ip.random_obs(n, D, seed=5)
    mean64, value64 = ip.rule(sd, ip.round32(obs), act)
    eps = ip.noise(SEED, call, n, A)
    with torch.no_grad():
        a, v, lp, m = (x.numpy() for x in twin({k: torch.from_numpy(x) for k, x in obs.items()}, noise=torch.from_numpy(eps)))
    err = {"mean": np.abs(m - mean64).max(), "value": np.abs(v - value64).max(),
           "log_prob": np.abs(lp - ip.log_prob(a, mean64, sd["log_std"])).max()}
    assert all(e > 0 for e in err.values()), err
    return {"obs": obs, "sd": sd, "mean64": mean64, "value64": value64, "eps": eps, "twin_err": err}


def kernel_errors(got: dict, ref: dict) -> dict:
    return {"mean": np.abs(got["mean"] - ref["mean64"]).max(), "value": np.abs(got["value"] - ref["value64"]).max(),
            "log_prob": np.abs(got["log_prob"] - ip.log_prob(got["action"], ref["mean64"], ref["sd"]["log_std"])).max()}


def assert_parity(got, ref, what):
    err = kernel_errors(got, ref)
    for k, e in err.items():
        print(f"parity {what} {k}: kernel {e:.3e}, twin {ref['twin_err'][k]:.3e}, ratio {e / ref['twin_err'][k]:.2f}")
    for k, e in err.items():
        assert e <= 10.0 * ref["twin_err"][k], (what, k, e, ref["twin_err"][k])


def ulps32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


# ---------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("D,A,trunk", CASES)
def test_parity_with_the_float64_rule(built, D, A, trunk):
    """mean, value and log_prob against the float64 rule on the float32-rounded inputs; log_prob is judged on the kernel's own
    action: the float64 formula at (kernel action, float64 mean, log_std)."""
    pol, _ = policy_for(D, A, trunk)
    ref = reference(D, A, trunk)
    got = run(pol, ref["obs"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert_parity(got, ref, f"D={D} A={A} {trunk}")


# ----------------------------------------------------------------------------------------------------------- 2. noise
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 8, "48x32-relu-vf16"), (25, 4, "256x256-relu")])
def test_noise_action_and_deterministic(built, D, A, trunk):
    pol, _ = policy_for(D, A, trunk)
    ref = reference(D, A, trunk)
    got = run(pol, ref["obs"])
    assert pol.calls == 1
    # the noise is the restatement's within 1 float32 ulp in every element (evaluated in double: only rounding ties are left)
    assert (np.abs(got["noise"].astype(np.float64) - ref["eps"]) <= ulps32(ref["eps"])).all()
    print("noise elements that differ from the restatement:", int((bits(got["noise"]) != bits(ref["eps"])).sum()), "of", ref["eps"].size)
    # the action is mean + exp(log_std) noise from the kernel's own mean and noise, within 1 ulp
    want = ip.sample(got["mean"], ref["sd"]["log_std"], got["noise"]).astype(np.float32)
    assert (np.abs(got["action"].astype(np.float64) - want) <= ulps32(want)).all()
    det = run(pol, ref["obs"], deterministic=True)
    assert pol.calls == 1                                        # not advanced
    assert np.array_equal(bits(det["action"]), bits(det["mean"])) and np.array_equal(bits(det["mean"]), bits(got["mean"]))
    assert not det["noise"].any()
    # log_prob of the mean: sum of A terms (-log_std - ln(2 pi) / 2), each one float32 subtraction, summed in float32: at most
    # A + 1 roundings of magnitudes below the sum of the terms' magnitudes
    ls = ref["sd"]["log_std"].astype(np.float64)
    lp64 = (-ls - ip.LOG_SQRT_2PI).sum()
    assert np.abs(det["log_prob"] - lp64).max() <= (A + 1) * 2.0 ** -24 * (np.abs(ls) + ip.LOG_SQRT_2PI).sum()
    assert np.array_equal(bits(det["value"]), bits(got["value"]))


# ------------------------------------------------------------------------------------------------- 3. value-only path
def test_values_is_the_full_calls_value(built):
    D, A, trunk = 25, 7, "48x32-relu-vf16"
    pol, _ = policy_for(D, A, trunk)
    obs = ip.random_obs(N, D, seed=5)
    full = run(pol, obs)
    calls = pol.calls
    v = pol.values(dev(obs))
    final = {k: x.clone() for k, x in dev(obs).items()}          # a final_observation-shaped dict holding the same numbers
    v2 = pol.values(final)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and tuple(v.shape) == (N,)
    assert np.array_equal(bits(v.cpu().numpy()), bits(full["value"])) and np.array_equal(bits(v2.cpu().numpy()), bits(full["value"]))
    assert pol.calls == calls


# ---------------------------------------------------------------------------------------- 4. tile position, sharding
@pytest.mark.parametrize("D,A,trunk", [(25, 7, "64x64-tanh"), (10, 7, "256x256-relu")])
def test_a_row_depends_on_itself_and_the_global_id(built, D, A, trunk):
    obs = ip.random_obs(N, D, seed=5)
    whole = run(policy_for(D, A, trunk)[0], obs)
    part = run(policy_for(D, A, trunk, n=16, env_id_offset=24)[0], {k: v[24:] for k, v in obs.items()})
    same_bits(part, whole, slice(24, 40))
    for n in (1, 17):
        same_bits(run(policy_for(D, A, trunk, n=n)[0], {k: v[:n] for k, v in obs.items()}), whole, slice(0, n))


# --------------------------------------------------------------------------------------------- 5. calls, checkpoints
def test_calls_and_checkpoints(built):
    from mycobotgym_amd import ActorCritic
    D, A, trunk = 25, 8, "64x64-tanh"
    obs = ip.random_obs(N, D, seed=5)
    pol, _ = policy_for(D, A, trunk)
    other, _ = policy_for(D, A, trunk)
    first, again = run(pol, obs), run(other, obs)
    same_bits(first, again)                                      # equal (seed, calls): equal outputs
    second = run(pol, obs)
    assert (second["noise"] != first["noise"]).any(axis=1).all() and (second["action"] != first["action"]).any(axis=1).all()
    assert np.array_equal(bits(second["mean"]), bits(first["mean"]))
    eps1 = ip.noise(SEED, 1, N, A)                               # the call number is the noise's second word
    assert (np.abs(second["noise"].astype(np.float64) - eps1) <= ulps32(eps1)).all()
    sd = pol.state_dict()
    assert sd["seed"] == SEED and sd["calls"] == 2
    pi, vf, act = ip.TRUNKS[trunk]
    fresh = ActorCritic(num_envs=N, obs_dim=D, act_dim=A, hidden=dict(pi=pi, vf=vf), activation=act, seed=999)
    fresh.load_state_dict(sd)
    assert (fresh.seed, fresh.calls) == (SEED, 2)
    for k, v in pol.state_dict().items():
        if torch.is_tensor(v):
            assert torch.equal(v, fresh.state_dict()[k]), k
    same_bits(run(fresh, obs), run(pol, obs))                    # the third call of the sequence, on both
    assert fresh.calls == pol.calls == 3


# ---------------------------------------------------------------------------------------------------- 6. fresh weights
def test_load_state_dict_replaces_the_blob(built):
    D, A, trunk = 25, 4, "64x64-tanh"
    pol, _ = policy_for(D, A, trunk, weights_seed=3)
    one, two = reference(D, A, trunk, 3), reference(D, A, trunk, 4)
    assert_parity(run(pol, one["obs"]), one, "first weights")
    pi, vf, act = ip.TRUNKS[trunk]
    pol.load_state_dict(ip.Twin(D, A, pi, vf, act).randomize(4).state_dict())
    pol.calls = 0
    got = run(pol, two["obs"])
    assert_parity(got, two, "second weights")
    stale = kernel_errors(got, one)
    assert stale["mean"] > 1e3 * one["twin_err"]["mean"] and stale["value"] > 1e3 * one["twin_err"]["value"], stale


# ---------------------------------------------------------------------------------------------------- 7. stray writes
@pytest.mark.parametrize("n", [40, 17])
def test_no_stray_writes(built, n):
    D, A, trunk, G = 25, 7, "64x64-tanh", 3
    pol, _ = policy_for(D, A, trunk, n=n)
    obs = {k: v[:n] for k, v in ip.random_obs(N, D, seed=5).items()}
    big = {k: torch.full((n + 2 * G, A) if k in ("action", "mean", "noise") else (n + 2 * G,), -77.25, device="cuda") for k in NAMES}
    pol.forward(dev(obs), out={k: v[G:G + n] for k, v in big.items()})
    torch.cuda.synchronize()
    plain = run(policy_for(D, A, trunk, n=n)[0], obs)
    for k, v in big.items():
        v = v.cpu().numpy()
        assert (v[:G] == -77.25).all() and (v[G + n:] == -77.25).all(), k
        assert np.array_equal(bits(v[G:G + n]), bits(plain[k])), k
    guard = torch.full((n + 2 * G,), -77.25, device="cuda")
    pol.values(dev(obs), out=guard[G:G + n])
    torch.cuda.synchronize()
    assert (guard[:G] == -77.25).all() and (guard[G + n:] == -77.25).all()
    assert np.array_equal(bits(guard[G:G + n].cpu().numpy()), bits(plain["value"]))


# ---------------------------------------------------------------------------------------------------- 8. on the engine
def test_on_the_engine_with_the_rollout_buffer(built):
    from mycobotgym_amd import ActorCritic, RolloutBuffer, _abi, make
    T = 8
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=N)
    D, A = envs.obs_dim, envs.action_dim
    twin = ip.Twin(D, A, (64, 64), (64, 64), "tanh").randomize(3)
    pol = ActorCritic.from_module(twin, envs, seed=SEED)
    assert (pol.pi, pol.vf, pol.activation, pol.obs_dim, pol.act_dim) == ((64, 64), (64, 64), "tanh", D, A)
    buf = RolloutBuffer(envs, n_steps=T, seed=0)
    obs, _ = envs.reset(seed=0)
    buf.start(obs)
    kept = []
    for t in range(T):
        in_place = [x.data_ptr() for x in pol._goal_obs(obs, "obs")]
        assert in_place == [obs[k].data_ptr() for k in ("observation", "achieved_goal", "desired_goal")]      # read where they lie
        a, v, logp = pol(obs)
        kept.append((a.clone(), v.clone(), logp.clone()))
        obs, r, term, trunc, info = envs.step(a, copy=(t % 2 == 0))
        if t % 2 == 1:
            assert obs["observation"].data_ptr() == envs._buf["obs"].data_ptr()                                # the engine's own buffers
        buf.add(a, v, logp, obs, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
    buf.finish(last_values=pol.values(obs))
    torch.cuda.synchronize()
    assert pol.calls == T
    rec = buf.records().cpu().numpy().reshape(T, N, -1).view(_abi.rollout_record_dtype(D, A))[..., 0]
    values = buf.planes()["value"].cpu().numpy()
    for t, (a, v, logp) in enumerate(kept):
        assert np.array_equal(bits(rec["action"][t]), bits(a.cpu().numpy())), t
        assert np.array_equal(bits(rec["log_prob"][t]), bits(logp.cpu().numpy())), t
        assert np.array_equal(bits(values[t]), bits(v.cpu().numpy())), t
    mb = next(iter(buf.get(batch_size=None)))
    mobs = {k: v.cpu() for k, v in mb.observations.items()}
    with torch.no_grad():
        _, lp32, _ = twin.evaluate_actions(mobs, mb.actions.cpu())
    sd = twin.numpy_state()
    mean64, _ = ip.rule(sd, {k: v.numpy().astype(np.float64) for k, v in mobs.items()}, "tanh")
    lp64 = ip.log_prob(mb.actions.cpu().numpy(), mean64, sd["log_std"])
    twin_err = np.abs(lp32.numpy() - lp64).max()
    gap = np.abs(lp32.numpy() - mb.old_log_prob.cpu().numpy()).max()
    print(f"engine: |twin evaluate_actions - old_log_prob| {gap:.3e}, twin's own error {twin_err:.3e}, ratio {gap / twin_err:.2f}")
    assert twin_err > 0 and gap <= 10.0 * twin_err
    envs.close()


def test_image_ids_and_foreign_policies_are_refused(built):
    from mycobotgym_amd import ActorCritic, make
    envs = make("MyCobotReach-Dense-joint-v1", num_envs=2)
    with pytest.raises(ValueError, match="CNN"):
        ActorCritic(envs)
    envs.close()
    with pytest.raises(ValueError, match="unsupported shape"):
        ActorCritic(num_envs=4, obs_dim=10, act_dim=7, hidden=(64, 40))
    with pytest.raises(ValueError, match="unsupported shape"):
        ActorCritic(num_envs=4, obs_dim=10, act_dim=7, hidden=(64, 64, 64, 64))
    with pytest.raises(ValueError, match="activation"):
        ActorCritic(num_envs=4, obs_dim=10, act_dim=7, activation="gelu")
    pol = ActorCritic(num_envs=4, obs_dim=10, act_dim=7)
    sd = pol.state_dict()
    assert float(sd["log_std"].abs().max()) == 0.0 and float(sd["action_net.bias"].abs().max()) == 0.0
    w = sd["mlp_extractor.policy_net.2.weight"].double()
    assert torch.allclose(w @ w.T, 2.0 * torch.eye(64, dtype=torch.float64, device=w.device), atol=1e-5)      # orthogonal, gain sqrt 2
    with pytest.raises(ValueError, match="does not fit"):
        pol.load_state_dict({k: v for k, v in sd.items() if k != "value_net.bias"})
