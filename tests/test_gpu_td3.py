"""TD3's and DDPG's gradient-free half on the GPU (mycobotgym_amd/td3_policy.py, csrc/mcg_td3.hip) against the restated rule
(tests/indep_td3.py): the collection action, the critics, the smoothed TD target, the Polyak step.

The yardstick is test_gpu_policy_update.py's ``assert_yardstick``, imported: per tensor, the kernel's max-abs error against the
float64 twin over the tensor's scale may be at most 10 x the float32 eager twin's own, floored at 2^-23.  The measured ratios are in
profiles/td3/parity.md.  N = 40 environments are two full tiles of 16 and one of 8; B = 75 four full tiles and one of 11."""
import functools
from fractions import Fraction

import numpy as np
import pytest
import torch

from tests import indep_td3 as it
from tests.test_gpu_policy_update import assert_yardstick
from tests.test_gpu_sac import bits, dev, dev_batch

pytestmark = pytest.mark.gpu

N, SEED = 40, it.NOISE_SEED
ID_OFFSET, BIG_CALL = 2 ** 33 + 7, 2 ** 32 + 5
FORWARD_CASES = [c for c in it.CASES if c[3] == 75]


@functools.lru_cache(maxsize=None)
def reference(D, A, trunk, B, nc):
    """Computed once per case and shared, and left unchanged: the twins, the batch and the clipped smoothing noise of call 0."""
    return it.case(D, A, trunk, B, nc)


def policy_of(twin, D, A, trunk, nc, **kw):
    from mycobotgym_amd import TD3Policy
    pi, qf, act = it.TRUNKS[trunk]
    pol = TD3Policy(num_envs=N, obs_dim=D, act_dim=A, hidden=dict(pi=pi, qf=qf), activation=act, seed=SEED, n_critics=nc, **kw)
    pol.load_state_dict(twin.state_dict())
    return pol


def fmaf32(a, b, c) -> np.ndarray:
    """fmaf on float32 arrays, exactly: the rational a b + c rounded to float32 once (to nearest, ties to even)."""
    out = np.empty(a.shape, np.float32)
    for j in range(a.size):
        exact = Fraction(float(a[j])) * Fraction(float(b[j])) + Fraction(float(c[j]))
        near = np.float32(float(exact))
        cands = [near, np.nextafter(near, np.float32(-np.inf)), np.nextafter(near, np.float32(np.inf))]
        best = min(cands, key=lambda x: (abs(Fraction(float(x)) - exact), int(np.float32(x).view(np.uint32)) & 1))
        out[j] = best
    return out


def host(d: dict) -> dict:
    return {k: v.detach().double().numpy() for k, v in d.items()}


# ------------------------------------------------------------------------------------------------------ 1. collection
@pytest.mark.parametrize("D,A,trunk,B,nc", FORWARD_CASES)
def test_collection_action(built, D, A, trunk, B, nc):
    check_collection_action(D, A, trunk, B, nc)


def check_collection_action(D, A, trunk, B, nc):
    """pol(obs) without and with noise under the yardstick; the noise bit for bit against the Python Philox with env_id_offset != 0 and
    a call number >= 2^32; every action inside [-1, 1]; noise_std = 0 writes +0 and still uses up a call number."""
    t32, t64, *_ = reference(D, A, trunk, B, nc)
    pol = policy_of(t64, D, A, trunk, nc, env_id_offset=ID_OFFSET)
    obs = it.random_obs(N, D, 77)
    with torch.no_grad():
        m64, m32 = t64.act(it.round32(obs)).numpy(), t32.act({k: v.astype(np.float32) for k, v in obs.items()}).double().numpy()
    what = f"act D={D} A={A} {trunk} nc={nc}"
    out = {k: torch.full((N, A), float("nan"), device="cuda") for k in ("action", "mean", "noise")}
    pol.calls = BIG_CALL
    a = pol(dev(obs), out=out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    assert a is out["action"] and pol.calls == BIG_CALL + 1
    assert not bits(got["noise"]).any()                              # +0, bit for bit
    assert np.array_equal(bits(got["action"]), bits(got["mean"]))
    assert_yardstick({"mean": got["mean"]}, {"mean": m32}, {"mean": m64}, what)
    std = 0.3
    pol(dev(obs), noise_std=std, out=out)
    got = {k: v.cpu().numpy() for k, v in out.items()}
    n = it.scaled_noise(it.DOMAIN_ACT, SEED, BIG_CALL + 1, N, A, std, None, ID_OFFSET)
    assert np.array_equal(bits(got["noise"]), bits(n))
    assert np.abs(got["action"]).max() <= 1.0 and (np.abs(m64 + n) > 1.0).any()                  # the clamp acts somewhere
    clamp = lambda m: np.clip(m + n.astype(np.float64), -1.0, 1.0)
    assert_yardstick({"action": got["action"]}, {"action": clamp(m32)}, {"action": clamp(m64)}, what + " noisy")
    own = np.clip((got["mean"] + n).astype(np.float32), np.float32(-1), np.float32(1))          # the stated line on the kernel's own mean
    assert np.array_equal(bits(got["action"]), bits(own))
    fresh = pol(dev(obs), noise_std=std)                             # another call number: another noise
    assert not torch.equal(fresh, out["action"]) and pol.calls == BIG_CALL + 3


# ------------------------------------------------------------------------------------------- 2. critics and the target
@pytest.mark.parametrize("D,A,trunk,B,nc", FORWARD_CASES)
def test_q_values_and_td_target(built, D, A, trunk, B, nc):
    check_q_values_and_td_target(D, A, trunk, B, nc)


def check_q_values_and_td_target(D, A, trunk, B, nc):
    """(The body of the test above, callable on other cases: tests/test_gpu_td3_shapes.py.)  The census of the min is the maker's and
    holds from 75 rows on."""
    t32, t64, batch, n, census = reference(D, A, trunk, B, nc)
    pol = policy_of(t64, D, A, trunk, nc)
    db = dev_batch(batch)
    what = f"D={D} A={A} {trunk} nc={nc}"
    for target in (False, True):
        q = pol.q_values(db.observations, db.actions, target=target)
        assert len(q) == nc
        with torch.no_grad():
            r64, r32 = t64.q(batch.observations, batch.actions, target).numpy(), t32.q(batch.observations, batch.actions, target).double().numpy()
        assert_yardstick({"q": torch.stack(q).cpu().numpy()}, {"q": r32}, {"q": r64}, f"q target={target} " + what)
    names = ("target", "next_action", "next_q", "noise")
    out = {k: torch.full(s, float("nan"), device="cuda") for k, s in pol._target_shapes(B).items()}
    y = pol.td_target(db, gamma=it.GAMMA, target_policy_noise=it.SIGMA, target_noise_clip=it.CLIP, out=out)
    got = {k: out[k].cpu().numpy() for k in names}
    assert y is out["target"] and pol.target_calls == 1
    r64, r32 = host(it.target(t64, batch, n)), host(it.target(t32, batch, n))
    assert_yardstick({k: got[k] for k in r64}, r32, r64, "td_target " + what)
    # bit for bit
    assert np.array_equal(bits(got["noise"]), bits(n))
    assert np.abs(got["next_action"]).max() <= 1.0
    nq = pol.q_values(db.next_observations, out["next_action"], target=True)
    assert np.array_equal(bits(torch.stack(nq).cpu().numpy()), bits(got["next_q"]))
    t = (np.float32(1.0) - batch.dones.reshape(-1)) * np.float32(it.GAMMA)
    assert t.dtype == np.float32
    assert np.array_equal(bits(got["target"]), bits(fmaf32(t, got["next_q"].min(axis=0), batch.rewards.reshape(-1))))
    if nc == 2 and B >= it.FIRST_ROWS:
        smaller = got["next_q"][1] < got["next_q"][0]
        assert 8 <= smaller[:75].sum() <= 67                          # each target critic is the min in some rows
    # a call number >= 2^32
    pol.target_calls = BIG_CALL
    pol.td_target(db, gamma=it.GAMMA, target_policy_noise=it.SIGMA, target_noise_clip=it.CLIP, out=out)
    assert np.array_equal(bits(out["noise"].cpu().numpy()), bits(it.scaled_noise(it.DOMAIN_TARGET, SEED, BIG_CALL, B, A, it.SIGMA, it.CLIP)))
    # sigma = 0: a noise of +0, the action of sigma > 0 with clip = 0, and a call number used up all the same
    pol.td_target(db, gamma=it.GAMMA, target_policy_noise=0.0, target_noise_clip=it.CLIP, out=out)
    assert not bits(out["noise"].cpu().numpy()).any() and pol.target_calls == BIG_CALL + 2
    plain = {k: out[k].clone() for k in ("next_action", "target")}
    pol.td_target(db, gamma=it.GAMMA, target_policy_noise=it.SIGMA, target_noise_clip=0.0, out=out)
    assert torch.equal(plain["next_action"].view(torch.int32), out["next_action"].view(torch.int32))
    assert torch.equal(plain["target"].view(torch.int32), out["target"].view(torch.int32))
    only = pol.td_target(db, gamma=it.GAMMA, target_policy_noise=0.0, target_noise_clip=0.0)      # no optional output
    assert torch.equal(only.view(torch.int32), plain["target"].view(torch.int32))


def test_rows_depend_on_themselves_alone(built):
    """B = 1 and B = 17 are the first rows of the B = 75 batch and give the same bits (the noise's id is the row's index)."""
    D, A, trunk, B, nc = 10, 7, "64x64-relu", 75, 2
    _, t64, batch, n, _ = reference(D, A, trunk, B, nc)
    pol = policy_of(t64, D, A, trunk, nc)
    db = dev_batch(batch)
    kw = dict(gamma=it.GAMMA, target_policy_noise=it.SIGMA, target_noise_clip=it.CLIP)
    full = pol.td_target(db, **kw).clone()
    for rows in (1, 17):
        cut = lambda d: {k: v[:rows] for k, v in d.items()}
        part = it.Batch(observations=cut(db.observations), actions=db.actions[:rows], next_observations=cut(db.next_observations),
                        dones=db.dones[:rows], rewards=db.rewards[:rows])
        pol.target_calls = 0
        assert torch.equal(pol.td_target(part, **kw).view(torch.int32), full[:rows].view(torch.int32)), rows


# -------------------------------------------------------------------------------------------------------- 3. Polyak
@pytest.mark.parametrize("nc", [1, 2])
def test_polyak_steps_both_pairs(built, nc):
    D, A, trunk = 25, 8, "48x32-tanh-qf16"
    _, t64, *_ = reference(D, A, trunk, 75, nc)
    pol = policy_of(t64, D, A, trunk, nc)
    before = {k: v.double().cpu().numpy() for k, v in pol._t.items()}
    assert all(not np.array_equal(before[k], before[k + "_target"]) for k in ("actor", "critic"))
    pol.polyak(0.25)
    for k in ("actor", "critic"):
        want = it.polyak_rule(before[k], before[k + "_target"], 0.25)
        got = pol._t[k + "_target"].double().cpu().numpy()
        assert np.abs(got - want).max() <= 2.0 ** -24 * np.abs(want).max() and not np.array_equal(got, before[k + "_target"]), k
        assert np.array_equal(pol._t[k].double().cpu().numpy(), before[k]), k
        assert not bits(pol._t[k + "_target"].cpu().numpy())[before[k] == 0.0].any(), k          # the padding stays +0
    pol.polyak(1.0)                                                  # the copy
    for k in ("actor", "critic"):
        assert torch.equal(pol._t[k].view(torch.int32), pol._t[k + "_target"].view(torch.int32)), k


# ------------------------------------------------------------------------------------------------- 4. from_module, DDPG
def test_from_module_and_the_ddpg_preset(built):
    from mycobotgym_amd import DDPGPolicy, TD3Policy
    D, A, trunk = 10, 7, "48x32-tanh-qf16"
    for nc in (1, 2):
        t32, t64, *_ = reference(D, A, trunk, 75, nc)
        pol = TD3Policy.from_module(t32, num_envs=N, obs_dim=D, act_dim=A, seed=SEED)
        assert (pol.pi, pol.qf, pol.activation, pol.n_critics) == ((48, 32), (16,), "tanh", nc)
        same = policy_of(t64, D, A, trunk, nc)
        assert all(torch.equal(pol._t[k].view(torch.int32), same._t[k].view(torch.int32)) for k in pol._t)
        sd = pol.state_dict()
        assert {k for k in sd if k not in ("seed", "calls", "target_calls")} == set(t32.state_dict())
        assert all(torch.equal(sd[k].cpu(), v) for k, v in t32.state_dict().items())
    ddpg = DDPGPolicy(num_envs=N, obs_dim=D, act_dim=A, hidden=(64, 64), seed=1)
    td3 = TD3Policy(num_envs=N, obs_dim=D, act_dim=A, hidden=(64, 64), seed=1)
    assert (ddpg.n_critics, td3.n_critics) == (1, 2) and ddpg.critic_floats * 2 == td3.critic_floats
    for p in (ddpg, td3):                                            # the targets start as copies
        assert torch.equal(p._t["actor"], p._t["actor_target"]) and torch.equal(p._t["critic"], p._t["critic_target"])
    assert torch.equal(ddpg._t["actor"], td3._t["actor"]) and ddpg._t["actor"].abs().max() > 0


# ------------------------------------------------------------------------------------------------------- 5. refusals
def test_outputs_are_checked_before_any_launch(built):
    D, A, trunk, B, nc = 10, 7, "64x64-relu", 75, 2
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol = policy_of(t64, D, A, trunk, nc)
    db = dev_batch(batch)
    obs = dev(it.random_obs(N, D, 77))
    for bad in (torch.zeros(N, A, dtype=torch.float64, device="cuda"), torch.zeros(N, A + 1, device="cuda"), torch.zeros(A, N, device="cuda").t(),
                torch.zeros(N, A)):
        with pytest.raises(ValueError, match="out"):
            pol(obs, out={"action": bad})
    for bad in (torch.zeros(B, dtype=torch.float64, device="cuda"), torch.zeros(B + 1, device="cuda"), torch.zeros(2 * B, device="cuda")[::2],
                torch.zeros(B)):
        with pytest.raises(ValueError, match="out"):
            pol.td_target(db, out={"target": bad})
    with pytest.raises(ValueError, match="unknown"):
        pol.td_target(db, out={"target": torch.zeros(B, device="cuda"), "next_log_prob": torch.zeros(B, device="cuda")})
    with pytest.raises(ValueError, match="out"):
        pol.q_values(db.observations, db.actions, out=torch.zeros(B, nc, device="cuda"))
    assert (pol.calls, pol.target_calls) == (0, 0)
