"""SAC's actor, twin critics, TD target and Polyak step on the GPU (mycobotgym_amd/sac_policy.py, csrc/mcg_sac.hip) against the restated
rule and its torch twin (tests/indep_sac.py).  N = 40 is two full tiles of 16 environments and one of 8 rows, B = 75 four full tiles and
one of 11; N = 17 and B = 1 are a tile of one row.

Bound of the parity tests, per case and per output: 10 x the largest error of the twin's CPU float32 result against the float64 rule on
the same float32-rounded inputs and the same restated noise, the maximum over the case's rows (the project's "10 x a twin" margin: the
twin is the yardstick, never the kernel), floored at 2^-23 of the output's largest magnitude.  The collection call's log_prob is judged
at the kernel's own u (the float64 formula at the kernel's noise, the float64 log_std and tanh of the kernel's own pre-squash value),
the twin's at its own; everything else against the float64 rule from the inputs on.  The measured ratios are in
profiles/sac_policy/parity.md.

The parity test itself runs at N = 40 and B = 75 alone.  N = 17 and 1 and B = 17 and 1 are held to the float64 rule through those
runs: test_a_row_depends_on_itself_and_its_id asserts that their outputs (all five of the collection call, all five of td_target, both
rows of q_values) are the larger run's first rows bit for bit, for two of the trunks (64x64-tanh and 256x256-relu, one per kernel
instantiation); test_no_stray_writes runs N = 17 and B = 1 between guard rows and sentinel borders.  A bitwise-equal row has the larger
run's error, so no second bound is needed."""
import contextlib
import ctypes as C
import functools
import math
import warnings

import numpy as np
import pytest
import torch

from tests import indep_sac as isac

pytestmark = pytest.mark.gpu

N, B, SEED = 40, 75, 21
GAMMA = float(np.float32(0.97))                                   # (the C entry takes gamma as a float32)
LOG_ALPHA = float(np.float32(math.log(0.3)))                      # what log_ent_coef holds in the parity tests
ALPHA = float(np.float32(math.exp(LOG_ALPHA)))                    # and the alpha the kernel forms from it
ACT_NAMES = ("action", "log_prob", "mean", "log_std", "noise")
TARGET_NAMES = ("target", "next_action", "next_log_prob", "next_q", "noise")


def dev(obs: dict) -> dict:
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in obs.items()}


def dev_batch(b) -> isac.Batch:
    t = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
    return isac.Batch(observations=dev(b.observations), actions=t(b.actions), next_observations=dev(b.next_observations), dones=t(b.dones),
                      rewards=t(b.rewards))


def rows_of(b, rows) -> isac.Batch:
    cut = lambda d: {k: v[rows] for k, v in d.items()}
    return isac.Batch(observations=cut(b.observations), actions=b.actions[rows], next_observations=cut(b.next_observations),
                      dones=b.dones[rows], rewards=b.rewards[rows])


@functools.lru_cache(maxsize=None)
def twin_for(D, A, trunk, weights_seed=3):
    pi, qf, act = isac.TRUNKS[trunk]
    return isac.Twin(D, A, pi, qf, act).randomize(weights_seed, D)


def policy_for(D, A, trunk, n=N, weights_seed=3, **kw):
    from mycobotgym_amd import SACPolicy
    pi, qf, act = isac.TRUNKS[trunk]
    pol = SACPolicy(num_envs=n, obs_dim=D, act_dim=A, hidden=dict(pi=pi, qf=qf), activation=act, seed=SEED, **kw)
    pol.load_state_dict(twin_for(D, A, trunk, weights_seed).state_dict())
    pol.log_ent_coef.fill_(LOG_ALPHA)
    return pol


def run_act(pol, obs: dict, deterministic=False) -> dict:
    """All five outputs of one collection call as numpy arrays."""
    out = pol._new(*ACT_NAMES)
    pol(dev(obs), deterministic=deterministic, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_target(pol, b, ent_coef=None) -> dict:
    """All five outputs of one td_target call as numpy arrays."""
    out = pol.new_target_out(len(b.actions), *TARGET_NAMES)
    pol.td_target(dev_batch(b), gamma=GAMMA, ent_coef=ent_coef, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_q(pol, obs: dict, actions, target=False) -> np.ndarray:
    q0, q1 = pol.q_values(dev(obs), torch.from_numpy(np.ascontiguousarray(actions)).cuda(), target=target)
    torch.cuda.synchronize()
    return np.stack([q0.cpu().numpy(), q1.cpu().numpy()])


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a: dict, b: dict, rows=slice(None), names=None):
    for k in names or a:
        want = b[k][:, rows] if k == "next_q" else b[k][rows]
        assert np.array_equal(bits(a[k]), bits(want)), k


def ulps32(x):
    return np.spacing(np.abs(x).astype(np.float32)).astype(np.float64)


def own_u(mean, log_std, noise) -> np.ndarray:
    """The pre-squash value of float32 mean, log_std and noise as include/mcg.h forms it: in double, rounded to float32 once."""
    return isac.pre_squash(mean, log_std, noise).astype(np.float32).astype(np.float64)


@functools.lru_cache(maxsize=None)
def reference(D, A, trunk, weights_seed=3, n=N, rows=B):
    """Computed once per case and shared: the inputs, the float64 rule on their float32 roundings with the restated noise of call 0,
    and the twin's float32 errors against it, which are the bounds' yardstick."""
    act = isac.TRUNKS[trunk][2]
    twin = twin_for(D, A, trunk, weights_seed)
    sd = twin.numpy_state()
    t = lambda d: {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}
    ref, err = {"sd": sd}, {}
    # ---- the collection action
    eps = isac.noise(isac.DOMAIN_ACT, SEED, 0, n, A)
    obs = isac.conditioned_obs(sd, act, n, D, 5, eps)
    mu64, ls64, _ = isac.actor_rule(sd, isac.round32(obs), act)
    a64 = np.tanh(isac.pre_squash(mu64, ls64, eps))
    with torch.no_grad():
        a, lp, mu, ls, u = (x.numpy() for x in twin.action_log_prob(t(obs), torch.from_numpy(eps)))
    err["act"] = {"mean": np.abs(mu - mu64).max(), "log_std": np.abs(ls - ls64).max(), "action": np.abs(a - a64).max(),
                  "log_prob": np.abs(lp - isac.log_prob(eps, ls64, np.tanh(u.astype(np.float64)))).max()}
    ref.update(obs=obs, eps=eps, mean=mu64, log_std=ls64, action=a64, log_prob=isac.log_prob(eps, ls64, a64))
    # ---- the critics and the target line
    eps8 = isac.noise(isac.DOMAIN_TARGET, SEED, 0, rows, A)
    b = isac.replay_batch(sd, act, rows, D, A, 11, eps8)
    with torch.no_grad():
        for target, name in ((False, "critic"), (True, "critic_target")):
            ref["q_" + name] = isac.q_rule(sd, name, b.observations, b.actions, act)
            err["q_" + name] = {"q": np.abs(twin.q(t(b.observations), torch.from_numpy(b.actions), target=target).numpy() - ref["q_" + name]).max()}
        got = twin.target(t(b.next_observations), torch.from_numpy(b.rewards), torch.from_numpy(b.dones), torch.from_numpy(eps8), GAMMA, ALPHA)
    ref["target"] = isac.target_rule(sd, b.next_observations, b.rewards, b.dones, eps8, GAMMA, ALPHA, act)
    err["target"] = {k: np.abs(got[k].numpy() - v).max() for k, v in ref["target"].items()}
    ref.update(batch=b, eps8=eps8, twin_err=err)
    return ref


def assert_parity(errors: dict, twin_err: dict, scale: dict, what: str):
    """errors / twin_err / scale: output -> the kernel's largest error, the twin's, the reference's largest magnitude."""
    ratios = {}
    for k, e in errors.items():
        bound = max(10.0 * twin_err[k], 2.0 ** -23 * scale[k])
        ratios[k] = e / bound
        print(f"parity {what} {k}: kernel {e:.3e}, twin {twin_err[k]:.3e}, bound {bound:.3e}, kernel / bound {ratios[k]:.3f}")
    for k, r in ratios.items():
        assert r <= 1.0, (what, k, errors[k], twin_err[k])


def act_errors(got: dict, ref: dict) -> dict:
    lp_at_own_u = isac.log_prob(got["noise"], ref["log_std"], np.tanh(own_u(got["mean"], got["log_std"], got["noise"])))
    return {"mean": np.abs(got["mean"] - ref["mean"]).max(), "log_std": np.abs(got["log_std"] - ref["log_std"]).max(),
            "action": np.abs(got["action"] - ref["action"]).max(), "log_prob": np.abs(got["log_prob"] - lp_at_own_u).max()}


def scales(ref: dict, names) -> dict:
    return {k: float(np.abs(ref[k]).max()) for k in names}


# ---------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("D,A,trunk", isac.CASES)
def test_parity_with_the_float64_rule(built, D, A, trunk):
    check_parity_with_the_float64_rule(D, A, trunk)


def check_parity_with_the_float64_rule(D, A, trunk, B=B, both_bounds=True):
    """Every output of the collection call, of q_values on both blobs and of td_target with all its intermediates.  ``both_bounds``:
    whether the case's float64 reference has rows at both clamp bounds of log_std (every case of this file has)."""
    pol, ref = policy_for(D, A, trunk), reference(D, A, trunk, rows=B)
    what = f"D={D} A={A} {trunk}" + ("" if B == 75 else f" B={B}")
    got = run_act(pol, ref["obs"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert_parity(act_errors(got, ref), ref["twin_err"]["act"], scales(ref, ("mean", "log_std", "action", "log_prob")), what + " act")
    # both clamp bounds act, and where they do the kernel's log_std is the bound itself
    if both_bounds:
        assert (got["log_std"] == 2.0).any() and (got["log_std"] == -20.0).any()
    assert np.array_equal(got["log_std"] == 2.0, ref["log_std"] == 2.0) and np.array_equal(got["log_std"] == -20.0, ref["log_std"] == -20.0)
    b = ref["batch"]
    for target, name in ((False, "q_critic"), (True, "q_critic_target")):
        q = run_q(pol, b.observations, b.actions, target=target)
        assert q.shape == (2, B) and np.isfinite(q).all()
        assert_parity({"q": np.abs(q - ref[name]).max()}, ref["twin_err"][name], {"q": float(np.abs(ref[name]).max())}, f"{what} {name}")
    got = run_target(pol, b)
    assert all(np.isfinite(v).all() for v in got.values())
    want = ref["target"]
    assert_parity({k: np.abs(got[k] - want[k]).max() for k in want}, ref["twin_err"]["target"], scales(want, want), what + " td_target")


# ----------------------------------------------------------------------------------------------------------- 2. noise
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 8, "48x32-relu-qf16"), (25, 4, "256x256-relu")])
def test_noise_squashing_and_deterministic(built, D, A, trunk):
    check_noise_squashing_and_deterministic(D, A, trunk)


def check_noise_squashing_and_deterministic(D, A, trunk, B=B):
    pol, ref = policy_for(D, A, trunk), reference(D, A, trunk, rows=B)
    got = run_act(pol, ref["obs"])
    assert pol.calls == 1 and pol.target_calls == 0
    assert np.array_equal(bits(got["noise"]), bits(ref["eps"]))                  # domain 7, bit for bit
    tgt = run_target(pol, ref["batch"])
    assert pol.calls == 1 and pol.target_calls == 1
    assert np.array_equal(bits(tgt["noise"]), bits(ref["eps8"]))                 # domain 8, bit for bit
    assert not np.array_equal(bits(tgt["noise"][:N]), bits(got["noise"][:B]))
    # the action is tanh of the pre-squash value formed from the kernel's own mean, log_std and noise, within 1 ulp; |action| <= 1
    want = np.tanh(own_u(got["mean"], got["log_std"], got["noise"]))
    assert (np.abs(got["action"].astype(np.float64) - want) <= ulps32(want)).all()
    assert np.abs(got["action"]).max() <= 1.0 and np.abs(tgt["next_action"]).max() <= 1.0
    det = run_act(pol, ref["obs"], deterministic=True)
    assert pol.calls == 1                                                        # not advanced
    assert np.array_equal(bits(det["action"]), bits(np.tanh(det["mean"].astype(np.float64)).astype(np.float32)))
    assert np.array_equal(bits(det["mean"]), bits(got["mean"])) and np.array_equal(bits(det["log_std"]), bits(got["log_std"]))
    assert not det["noise"].any() and np.abs(det["action"]).max() <= 1.0
    lp = isac.log_prob(det["noise"], det["log_std"], det["action"])
    assert (np.abs(det["log_prob"] - lp) <= ulps32(lp)).all()
    # far out the squashing saturates and stays inside [-1, 1]: a huge mean through the bias of the head mu
    sd = pol.state_dict()
    sd["actor.mu.bias"] = torch.full_like(sd["actor.mu.bias"], 40.0) * torch.tensor([1.0, -1.0] * 8, device="cuda")[:A]
    pol.load_state_dict(sd)
    far = run_act(pol, ref["obs"])
    assert np.abs(far["action"]).max() == 1.0 and np.isfinite(far["log_prob"]).all()


# ------------------------------------------------------------------------------------------------- 3. consistency
@pytest.mark.parametrize("D,A,trunk", [(25, 8, "64x64-tanh"), (10, 7, "48x32-relu-qf16"), (25, 4, "256x256-relu")])
def test_td_target_is_consistent_with_its_parts(built, D, A, trunk):
    check_td_target_is_consistent_with_its_parts(D, A, trunk)


def check_td_target_is_consistent_with_its_parts(D, A, trunk, B=B):
    pol, ref = policy_for(D, A, trunk), reference(D, A, trunk, rows=B)
    b = ref["batch"]
    got = run_target(pol, b)
    # next_q is q_values on the target blob at the action td_target drew, bit for bit (registers there, memory here)
    q = run_q(pol, b.next_observations, got["next_action"], target=True)
    assert np.array_equal(bits(q), bits(got["next_q"]))
    assert not np.array_equal(bits(run_q(pol, b.next_observations, got["next_action"], target=False)), bits(got["next_q"]))
    # target is the header's float32 expression of its own intermediates, rounding by rounding (a product of two float32 numbers is
    # exact in float64), within 1 ulp
    f64 = lambda x: np.asarray(x, np.float64)
    nq = (f64(got["next_q"].min(axis=0)) - ALPHA * f64(got["next_log_prob"])).astype(np.float32)
    coef = ((1.0 - f64(b.dones[:, 0])) * GAMMA).astype(np.float32)
    want = f64(coef) * f64(nq) + f64(b.rewards[:, 0])
    assert (np.abs(f64(got["target"]) - want) <= ulps32(want)).all()
    print("td_target rows that differ from the expression's own rounding:", int((bits(got["target"]) != bits(want.astype(np.float32))).sum()))
    ended = b.dones[:, 0] == 1.0
    assert ended.any() and np.array_equal(bits(got["target"][ended]), bits(b.rewards[ended, 0]))
    # alpha from the device's log_ent_coef and the same alpha given on the host agree (exp is evaluated in double on both sides)
    pol.target_calls = 0
    host = run_target(pol, b, ent_coef=ALPHA)
    same_bits(host, got)
    pol.target_calls = 0
    other = run_target(pol, b, ent_coef=0.0)
    assert np.array_equal(bits(other["next_q"]), bits(got["next_q"])) and (other["target"] != got["target"])[~ended].all()
    want0 = f64(coef) * f64(got["next_q"].min(axis=0)) + f64(b.rewards[:, 0])
    assert (np.abs(other["target"] - want0) <= ulps32(want0)).all()


# ---------------------------------------------------------------------------------------- 4. tile position, sharding
@pytest.mark.parametrize("D,A,trunk", [(25, 7, "64x64-tanh"), (10, 7, "256x256-relu")])
def test_a_row_depends_on_itself_and_its_id(built, D, A, trunk):
    obs = isac.random_obs(N, D, seed=5)
    whole = run_act(policy_for(D, A, trunk), obs)
    part = run_act(policy_for(D, A, trunk, n=16, env_id_offset=24), {k: v[24:] for k, v in obs.items()})
    same_bits(part, whole, slice(24, 40))                        # the global environment id, not the row
    shifted = run_act(policy_for(D, A, trunk, n=16), {k: v[24:] for k, v in obs.items()})
    assert np.array_equal(bits(shifted["mean"]), bits(whole["mean"][24:])) and (shifted["noise"] != whole["noise"][24:]).any(axis=1).all()
    for n in (1, 17):
        same_bits(run_act(policy_for(D, A, trunk, n=n), {k: v[:n] for k, v in obs.items()}), whole, slice(0, n))
    sd = twin_for(D, A, trunk).numpy_state()
    b = isac.replay_batch(sd, isac.TRUNKS[trunk][2], B, D, A, 11, isac.noise(isac.DOMAIN_TARGET, SEED, 0, B, A))
    pol = policy_for(D, A, trunk)
    full, qfull = run_target(pol, b), run_q(pol, b.observations, b.actions)
    for n in (1, 17):
        pol.target_calls = 0
        same_bits(run_target(pol, rows_of(b, slice(0, n))), full, slice(0, n))
        assert np.array_equal(bits(run_q(pol, {k: v[:n] for k, v in b.observations.items()}, b.actions[:n])), bits(qfull[:, :n]))
    # other rows' content does not reach a row: every row but 20 replaced
    rng = np.random.default_rng(2)
    noisy = lambda x: np.where((np.arange(len(x)) == 20).reshape(-1, *[1] * (x.ndim - 1)), x, rng.normal(size=x.shape).astype(np.float32))
    scrambled = isac.Batch(observations={k: noisy(v) for k, v in b.observations.items()}, actions=noisy(b.actions),
                           next_observations={k: noisy(v) for k, v in b.next_observations.items()}, dones=b.dones, rewards=noisy(b.rewards))
    pol.target_calls = 0
    same_bits(rows_of_out(run_target(pol, scrambled), 20), full, slice(20, 21))
    assert np.array_equal(bits(run_q(pol, scrambled.observations, scrambled.actions)[:, 20]), bits(qfull[:, 20]))
    # the critics are two: the rows of q differ, and target=True reads the other blob
    assert (qfull[0] != qfull[1]).all() and (run_q(pol, b.observations, b.actions, target=True) != qfull).all()


def rows_of_out(out: dict, row: int) -> dict:
    return {k: (v[:, row:row + 1] if k == "next_q" else v[row:row + 1]) for k, v in out.items()}


# ---------------------------------------------------------------------------------------------------------- 5. Polyak
@pytest.mark.parametrize("trunk", ["48x32-relu-qf16", "64x64-tanh"])
def test_polyak(built, trunk):
    D, A = 10, 7
    pol = policy_for(D, A, trunk)
    critic, before = pol._t["critic"].clone(), pol._t["critic_target"].clone()
    actor = pol._t["actor"].clone()
    assert not torch.equal(critic, before)
    pad = ((critic == 0) & (before == 0)).cpu().numpy()
    assert pad.any() and not pad.all()
    pol.polyak(tau=0.005)
    torch.cuda.synchronize()
    c, t0, t1 = critic.cpu().numpy(), before.cpu().numpy(), pol._t["critic_target"].cpu().numpy()
    want = isac.polyak_rule(c, t0, 0.005)
    assert (np.abs(t1.astype(np.float64) - want) <= ulps32(want)).all()                # within one float32 ulp of the float64 rule
    some = np.random.default_rng(0).choice(c.size, min(c.size, 2000), replace=False)
    assert np.array_equal(bits(t1[some]), bits(isac.polyak_restated(c[some], t0[some], 0.005)))      # the header's expression, bit for bit
    assert not bits(t1)[pad].any()                                                     # padding stays +0.0
    assert (t1 != t0)[~pad].mean() > 0.9
    assert torch.equal(pol._t["critic"], critic) and torch.equal(pol._t["actor"], actor)
    # the unpacked weights moved by the same rule: the blob is still a blob
    sd = pol.state_dict()
    k = "critic_target.qf1.0.weight"
    tw = twin_for(D, A, trunk).state_dict()
    moved = isac.polyak_rule(tw["critic.qf1.0.weight"].numpy(), tw[k].numpy(), 0.005)
    assert (np.abs(sd[k].cpu().numpy() - moved) <= ulps32(moved)).all()
    # tau = 1 is the copy, whatever the target held: a diverged target is repaired and a critic's -0.0 stays -0.0
    live = np.flatnonzero(~pad)[:3]
    pol._t["critic_target"][int(live[0])], pol._t["critic_target"][int(live[1])] = float("inf"), float("nan")
    pol._t["critic"][int(live[2])] = -0.0
    critic, c = pol._t["critic"].clone(), pol._t["critic"].cpu().numpy()
    assert bits(c)[live[2]] == 0x80000000
    pol.polyak(tau=1.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(pol._t["critic_target"].cpu().numpy()), bits(c))
    pol.polyak(tau=0.0)
    torch.cuda.synchronize()
    assert np.array_equal(bits(pol._t["critic_target"].cpu().numpy()), bits(c)) and torch.equal(pol._t["critic"], critic)


# ---------------------------------------------------------------------------------------------------- 6. stray writes
@pytest.mark.parametrize("n,rows", [(40, 75), (17, 1)])
def test_no_stray_writes(built, n, rows):
    """Outputs are slices of larger tensors whose borders keep a sentinel; inputs are slices of larger tensors whose guard rows are
    NaN, so a row read past the count would poison a result; outputs left out are not written."""
    D, A, trunk, G = 25, 7, "64x64-tanh", 3
    S = -77.25
    pol = policy_for(D, A, trunk, n=n)
    sd = twin_for(D, A, trunk).numpy_state()
    eps = isac.noise(isac.DOMAIN_ACT, SEED, 0, n, A)
    obs = isac.conditioned_obs(sd, "tanh", n, D, 5, eps)
    plain = run_act(policy_for(D, A, trunk, n=n), obs)

    def guarded(x):                      # [G NaN rows, x, G NaN rows] on the device -> the middle slice
        x = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        big = torch.full((len(x) + 2 * G, *x.shape[1:]), float("nan"), dtype=x.dtype, device="cuda")
        big[G:G + len(x)] = x
        return big[G:G + len(x)]

    def bordered(shape, axis=0):
        shape = list(shape)
        shape[axis] += 2 * G
        return torch.full(shape, S, device="cuda")

    def check(big, want, k, axis=0):
        v = big.cpu().numpy()
        v = np.moveaxis(v, axis, 0)
        m = v.shape[0] - 2 * G
        assert (v[:G] == S).all() and (v[G + m:] == S).all(), k
        assert np.array_equal(bits(np.moveaxis(v[G:G + m], 0, axis)), bits(want)), k

    big = {k: bordered((n,) if k == "log_prob" else (n, A)) for k in ACT_NAMES}
    pol({k: guarded(v) for k, v in obs.items()}, out={k: v[G:G + n] for k, v in big.items()})
    torch.cuda.synchronize()
    for k, v in big.items():
        check(v, plain[k], k)
    only = bordered((n, A))
    pol.calls = 0
    pol({k: guarded(v) for k, v in obs.items()}, out={"action": only[G:G + n]})          # the optional outputs left out
    torch.cuda.synchronize()
    check(only, plain["action"], "action alone")

    b = isac.replay_batch(sd, "tanh", rows, D, A, 11, isac.noise(isac.DOMAIN_TARGET, SEED, 0, rows, A))
    plain_t = run_target(policy_for(D, A, trunk, n=n), b)
    gb = isac.Batch(observations={k: guarded(v) for k, v in b.observations.items()}, actions=guarded(b.actions),
                    next_observations={k: guarded(v) for k, v in b.next_observations.items()}, dones=guarded(b.dones), rewards=guarded(b.rewards))
    shape = {"target": (rows,), "next_log_prob": (rows,), "next_action": (rows, A), "noise": (rows, A)}
    big = {k: bordered(s) for k, s in shape.items()}
    nq_all = torch.full((2 + 2 * G, rows), S, device="cuda")      # [2, B] is contiguous: its borders are the rows before and after
    out = {k: v[G:G + rows] for k, v in big.items()}
    out["next_q"] = nq_all[G:G + 2]
    pol.td_target(gb, gamma=GAMMA, out=out)
    torch.cuda.synchronize()
    for k, v in big.items():
        check(v, plain_t[k], k)
    check(nq_all, plain_t["next_q"], "next_q")
    only = bordered((rows,))
    pol.target_calls = 0
    pol.td_target(gb, gamma=GAMMA, out={"target": only[G:G + rows]})
    torch.cuda.synchronize()
    check(only, plain_t["target"], "target alone")
    qbig = torch.full((2 + 2 * G, rows), S, device="cuda")
    pol.q_values(gb.observations, gb.actions, out=qbig[G:G + 2])
    torch.cuda.synchronize()
    check(qbig, run_q(pol, b.observations, b.actions), "q")


# --------------------------------------------------------------------------------------------- 7. calls, checkpoints
def test_calls_and_checkpoints(built):
    from mycobotgym_amd import SACPolicy
    D, A, trunk = 25, 8, "64x64-tanh"
    ref = reference(D, A, trunk)
    obs, b = ref["obs"], ref["batch"]
    pol, other = policy_for(D, A, trunk), policy_for(D, A, trunk)
    first, again = run_act(pol, obs), run_act(other, obs)
    same_bits(first, again)                                      # equal (seed, calls): equal outputs
    second = run_act(pol, obs)
    assert (second["noise"] != first["noise"]).any(axis=1).all() and np.array_equal(bits(second["mean"]), bits(first["mean"]))
    assert np.array_equal(bits(second["noise"]), bits(isac.noise(isac.DOMAIN_ACT, SEED, 1, N, A)))       # the call number is the second word
    t0 = run_target(pol, b)
    t1 = run_target(pol, b)
    assert np.array_equal(bits(t1["noise"]), bits(isac.noise(isac.DOMAIN_TARGET, SEED, 1, B, A))) and (t1["noise"] != t0["noise"]).any()
    pol.polyak(0.3)
    sd = pol.state_dict()
    assert (sd["seed"], sd["calls"], sd["target_calls"]) == (SEED, 2, 2)
    assert sd["log_ent_coef"].dtype == torch.float32 and tuple(sd["log_ent_coef"].shape) == (1,)
    pi, qf, act = isac.TRUNKS[trunk]
    fresh = SACPolicy(num_envs=N, obs_dim=D, act_dim=A, hidden=dict(pi=pi, qf=qf), activation=act, seed=999)
    assert float(fresh.log_ent_coef) == 0.0                      # ln 1
    assert torch.equal(fresh._t["critic"], fresh._t["critic_target"]) and not torch.equal(fresh._t["critic"], pol._t["critic"])
    fresh.load_state_dict(sd)
    assert (fresh.seed, fresh.calls, fresh.target_calls) == (SEED, 2, 2)
    for k in ("actor", "critic", "critic_target", "log_ent_coef"):
        assert torch.equal(fresh._t[k], pol._t[k]), k
    same_bits(run_act(fresh, obs), run_act(pol, obs))            # the third collection call, on both
    same_bits(run_target(fresh, b), run_target(pol, b))          # and the third target call
    assert fresh.calls == pol.calls == 3 and fresh.target_calls == pol.target_calls == 3
    # an SB3 policy's state dict has no log_ent_coef and no host state: what is not given stays
    fresh.load_state_dict(twin_for(D, A, trunk).state_dict())
    assert (fresh.seed, fresh.calls, fresh.target_calls) == (SEED, 3, 3) and float(fresh.log_ent_coef) == np.float32(LOG_ALPHA)
    with pytest.raises(ValueError, match="does not fit"):
        fresh.load_state_dict({k: v for k, v in sd.items() if k != "critic_target.qf1.0.bias"})


def test_initial_weights(built):
    from mycobotgym_amd import SACPolicy
    pol = SACPolicy(num_envs=4, obs_dim=10, act_dim=7, hidden=(64, 64), seed=5)
    assert (pol.pi, pol.qf, pol.activation) == ((64, 64), (64, 64), "relu")
    sd = pol.state_dict()
    for k, v in sd.items():
        if k.endswith(".weight"):                                # nn.Linear's default: uniform within 1 / sqrt(fan_in), biases too
            bound = 1.0 / math.sqrt(v.shape[1])
            assert float(v.abs().max()) <= bound and float(v.abs().max()) > 0.8 * bound, k
            assert float(sd[k[:-6] + "bias"].abs().max()) <= bound and float(sd[k[:-6] + "bias"].abs().max()) > 0, k
        if k.startswith("critic."):
            assert torch.equal(v, sd[k.replace("critic.", "critic_target.", 1)]), k
    assert not torch.equal(sd["critic.qf0.0.weight"], sd["critic.qf1.0.weight"])
    again = SACPolicy(num_envs=4, obs_dim=10, act_dim=7, hidden=(64, 64), seed=5).state_dict()
    assert all(torch.equal(v, again[k]) for k, v in sd.items() if torch.is_tensor(v))


# ---------------------------------------------------------------------------------------------------- 8. on the engine
@contextlib.contextmanager
def no_sync():
    """A torch call that synchronises raises inside (the C entries are known not to: they only enqueue on the current stream)."""
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")      # (torch says once that the mode does not detect every synchronising operation)
        torch.cuda.set_sync_debug_mode("error")
    try:
        yield
    finally:
        torch.cuda.set_sync_debug_mode("default")


def test_on_the_engine_with_the_her_buffer(built):
    from mycobotgym_amd import HerBuffer, SACPolicy, make
    n, steps, batch = 64, 25, 256
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=n, max_episode_steps=10, seed=3)
    D, A = envs.obs_dim, envs.action_dim
    pol = SACPolicy(envs, hidden=(64, 64), seed=SEED)
    twin = isac.Twin(D, A, (64, 64), (64, 64), "relu")
    weights = {k: v.cpu() for k, v in pol.state_dict().items() if k in twin.state_dict()}
    twin.load_state_dict(weights)
    same = SACPolicy.from_module(twin, envs, seed=SEED)
    assert (same.pi, same.qf, same.activation, same.obs_dim, same.act_dim) == ((64, 64), (64, 64), "relu", D, A)
    assert all(torch.equal(same._t[k], pol._t[k]) for k in ("actor", "critic", "critic_target"))
    buf = HerBuffer(envs, capacity=40, n_sampled_goal=4, seed=2)
    obs, _ = envs.reset(seed=0)
    buf.start(obs)
    torch.cuda.synchronize()
    for t in range(steps):
        in_place = [x.data_ptr() for x in pol._goal_obs(obs, "obs")]
        assert in_place == [obs[k].data_ptr() for k in ("observation", "achieved_goal", "desired_goal")]      # read where they lie
        with no_sync():
            a = pol(obs)
        out = envs.step(a)
        with no_sync():
            buf.add(a, *out)
        obs = out[0]
    tout = pol.new_target_out(batch, *TARGET_NAMES)
    before = pol._t["critic_target"].clone()
    with no_sync():
        sample = buf.sample(batch, check=False)
        y = pol.td_target(sample, gamma=0.99, out=tout)
        q0, q1 = pol.q_values(sample.observations, sample.actions)
        pol.polyak(tau=0.005)
    torch.cuda.synchronize()
    assert pol.calls == steps and pol.target_calls == 1 and buf.counters()["sample_give_ups"] == 0
    assert torch.equal(pol._t["critic_target"], before)          # critic_target started as the critic's copy: the step leaves it
    got = {k: v.cpu().numpy() for k, v in tout.items()}
    assert y.data_ptr() == tout["target"].data_ptr()
    assert all(np.isfinite(v).all() for v in got.values()) and np.isfinite(q0.cpu().numpy()).all() and np.isfinite(q1.cpu().numpy()).all()
    assert np.abs(a.cpu().numpy()).max() <= 1.0
    nxt = {k: v.cpu().numpy() for k, v in sample.next_observations.items()}
    reward, done = sample.rewards.cpu().numpy(), sample.dones.cpu().numpy()
    eps = isac.noise(isac.DOMAIN_TARGET, SEED, 0, batch, A)
    assert np.array_equal(bits(got["noise"]), bits(eps))
    sd = twin.numpy_state()
    want = isac.target_rule(sd, nxt, reward, done, eps, float(np.float32(0.99)), 1.0, "relu")
    with torch.no_grad():
        t32 = twin.target({k: torch.from_numpy(v) for k, v in nxt.items()}, torch.from_numpy(reward), torch.from_numpy(done),
                          torch.from_numpy(eps), float(np.float32(0.99)), 1.0)
    assert_parity({k: np.abs(got[k] - want[k]).max() for k in want}, {k: np.abs(t32[k].numpy() - want[k]).max() for k in want},
                  scales(want, want), "engine td_target")
    envs.close()


# ------------------------------------------------------------------------------------------------------- 9. refusals
def test_refusals(built):
    from mycobotgym_amd import FrameStack, SACPolicy, _abi, make
    envs = make("MyCobotReach-Dense-joint-v1", num_envs=2)
    with pytest.raises(ValueError, match="CNN"):
        SACPolicy(envs)
    with pytest.raises(ValueError, match="CNN"):
        SACPolicy(FrameStack(envs, 2))
    envs.close()
    D, A, trunk, S = 10, 7, "16-relu", -77.25
    pol = policy_for(D, A, trunk)
    b = reference(D, A, trunk)["batch"]
    db = dev_batch(b)
    # Python's own: float64, mis-shaped, another device
    with pytest.raises(ValueError, match="expected float32"):
        pol.q_values({k: v.double() for k, v in db.observations.items()}, db.actions)
    with pytest.raises(ValueError, match="expected shape"):
        pol.q_values(db.observations, db.actions[:, :A - 1])
    with pytest.raises(ValueError, match="lives on cpu"):
        pol.q_values({k: v.cpu() for k, v in db.observations.items()}, db.actions)
    with pytest.raises(ValueError, match="lives on cpu"):
        pol.td_target(db._replace(rewards=db.rewards.cpu()))
    with pytest.raises(ValueError, match="expected float32"):
        pol.td_target(db._replace(dones=db.dones.bool()))
    with pytest.raises(ValueError, match="expected shape"):
        pol.td_target(db._replace(rewards=db.rewards[:-1]))
    with pytest.raises(ValueError, match="expected shape"):
        pol({k: v[:-1] for k, v in dev(reference(D, A, trunk)["obs"]).items()})
    # a caller's `out` tensors reach the kernel as bare pointers: float64, short, transposed, elsewhere or misnamed ones are refused
    dobs, f32 = dev(reference(D, A, trunk)["obs"]), dict(dtype=torch.float32, device="cuda")
    for bad, why in (({"action": torch.empty(N, A, dtype=torch.float64, device="cuda")}, "expected a contiguous float32"),
                     ({"action": torch.empty(N - 1, A, **f32)}, r"out\['action'\]"),
                     ({"action": torch.empty(A, N, **f32).t()}, "contiguous"),
                     ({"action": torch.empty(N, A)}, "lives on cpu"),
                     ({"log_prob": torch.empty(N, **f32)}, "'action' is required"),
                     ({"action": torch.empty(N, A, **f32), "next_q": torch.empty(2, N, **f32)}, "unknown")):
        with pytest.raises(ValueError, match=why):
            pol(dobs, out=bad)
    for bad, why in (({"target": torch.empty(B, dtype=torch.float64, device="cuda")}, "expected a contiguous float32"),
                     ({"target": torch.empty(B, **f32), "next_q": torch.empty(2, B - 1, **f32)}, r"out\['next_q'\]"),
                     ({"target": torch.empty(B, **f32), "next_action": torch.empty(A, B, **f32).t()}, "contiguous"),
                     ({"target": torch.empty(B)}, "lives on cpu"),
                     ({"next_q": torch.empty(2, B, **f32)}, "'target' is required")):
        with pytest.raises(ValueError, match=why):
            pol.td_target(db, out=bad)
    assert pol.target_calls == 0 and pol.calls == 0
    # the C side's: MCG_ERR_ARG, and nothing is launched -- the outputs keep their sentinel
    out = {k: v.fill_(S) for k, v in pol.new_target_out(B, *TARGET_NAMES).items()}
    for kw in (dict(gamma=1.5), dict(gamma=-0.1), dict(ent_coef=-1.0), dict(ent_coef=float("inf"))):
        with pytest.raises(_abi.McgError, match="code 1"):
            pol.td_target(db, **{"gamma": GAMMA, **kw}, out=out)
    for tau in (-0.5, 1.5, float("nan")):
        with pytest.raises(_abi.McgError, match="tau"):
            pol.polyak(tau)
    lib, stream = pol._lib, pol._stream()
    rows = _abi.McgSacRows(obs=db.observations["observation"].data_ptr(), achieved=db.observations["achieved_goal"].data_ptr(),
                           desired=db.observations["desired_goal"].data_ptr(), action=db.actions.data_ptr())
    q = torch.full((2, B), S, device="cuda")
    assert lib.mcg_sac_q(C.byref(pol._cbuf), 2, C.byref(rows), B, q.data_ptr(), stream) == _abi.MCG_ERR_ARG
    assert lib.mcg_sac_q(C.byref(pol._cbuf), 0, C.byref(rows), 0, q.data_ptr(), stream) == _abi.MCG_ERR_ARG
    assert lib.mcg_sac_q(C.byref(pol._cbuf), 0, C.byref(_abi.McgSacRows(obs=rows.obs)), B, q.data_ptr(), stream) == _abi.MCG_ERR_ARG
    wrong = _abi.McgSac.from_buffer_copy(pol._cbuf)
    wrong.critic_floats += 16
    assert lib.mcg_sac_q(C.byref(wrong), 0, C.byref(rows), B, q.data_ptr(), stream) == _abi.MCG_ERR_ARG
    assert lib.mcg_sac_polyak(C.byref(wrong), 0.5, stream) == _abi.MCG_ERR_ARG
    before = pol._t["critic_target"].clone()
    torch.cuda.synchronize()
    assert all(bool((v == S).all()) for v in out.values()) and bool((q == S).all()) and torch.equal(pol._t["critic_target"], before)
    assert pol.target_calls == 0
