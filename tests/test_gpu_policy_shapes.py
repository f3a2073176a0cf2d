"""The actor-critic policy and the PPO / A2C update on the GPU at the shape edges of tests/policy_shape_cases.py: a third layer
(n == 3), widths 80..240 in the MT = 16 kernels with partial tiles, the policy and the value net on different sides of width 64, A in
{1, 9, 13, 16} and D in {1, 12, 45, 58}.  The module's docstring there says which path each case reaches.

The checks are the bodies of tests/test_gpu_policy.py and tests/test_gpu_policy_update.py, called on these cases, under the same
bounds (``assert_parity``: 10 x the float32 eager twin's error against float64; ``assert_yardstick``: the same per tensor, floored at
2^-23 of its scale); what is new here is the row-independence check on scrambled rows, the direct check of the padding columns, the
sentinel borders around the policy's blob as well, and the checkpoint of a three-layer policy.  The measured ratios are in
profiles/policy_shapes/parity.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import indep_policy as ip
from tests import policy_shape_cases as psc
from tests import test_gpu_policy_update as upd
from tests.test_gpu_policy import N, NAMES, SEED, assert_parity, bits, dev, policy_for, reference, run
from tests.test_gpu_policy_update import batch_for, padding_mask, samples, updater

pytestmark = pytest.mark.gpu

FORWARD = list(dict.fromkeys((D, A, t) for D, A, t, _ in psc.CASES))      # (the collection call does not read B)


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("D,A,trunk", FORWARD)
def test_parity_with_the_float64_rule(built, D, A, trunk):
    """mean, value and log_prob of the collection call (N = 40) against the float64 rule; values() gives the call's value."""
    pol, _ = policy_for(D, A, trunk)
    ref = reference(D, A, trunk)
    got = run(pol, ref["obs"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert_parity(got, ref, f"D={D} A={A} {trunk}")
    v = pol.values(dev(ref["obs"]))
    assert np.array_equal(bits(v.cpu().numpy()), bits(got["value"])) and pol.calls == 1


@pytest.mark.parametrize("D,A,trunk,B", psc.CASES)
def test_evaluate_actions_parity(built, D, A, trunk, B):
    """value and log_prob of B rows under the yardstick, the entropy, and the first 1 and 17 rows alone."""
    upd.check_evaluate_actions_parity(D, A, trunk, B)


@pytest.mark.parametrize("D,A,trunk", FORWARD)
def test_noise_action_and_deterministic(built, D, A, trunk):
    """The noise bit for bit with the Python Philox in all A columns (pairs 4..7 for A > 8; the dropped second value for an odd A);
    the action from the kernel's own mean and noise; deterministic=True gives the mean's action and the log-prob of the mean."""
    pol, _ = policy_for(D, A, trunk)
    ref = reference(D, A, trunk)
    got = run(pol, ref["obs"])
    assert pol.calls == 1 and got["noise"].shape == (N, A)
    assert np.array_equal(bits(got["noise"]), bits(ref["eps"]))
    want = ip.sample(got["mean"], ref["sd"]["log_std"], got["noise"]).astype(np.float32)
    assert (np.abs(got["action"].astype(np.float64) - want) <= upd.ulps32(want)).all()
    again = run(pol, ref["obs"])
    assert np.array_equal(bits(again["noise"]), bits(ip.noise(SEED, 1, N, A)))           # the call number is the second word
    det = run(pol, ref["obs"], deterministic=True)
    assert pol.calls == 2
    assert np.array_equal(bits(det["action"]), bits(det["mean"])) and np.array_equal(bits(det["mean"]), bits(got["mean"]))
    assert not det["noise"].any() and np.array_equal(bits(det["value"]), bits(got["value"]))
    ls = ref["sd"]["log_std"].astype(np.float64)
    lp64 = (-ls - ip.LOG_SQRT_2PI).sum()
    assert np.abs(det["log_prob"] - lp64).max() <= (A + 1) * 2.0 ** -24 * (np.abs(ls) + ip.LOG_SQRT_2PI).sum()


@pytest.mark.parametrize("D,A,trunk,B", psc.ROW_CASES)
def test_a_row_does_not_read_its_tiles_other_rows(built, D, A, trunk, B):
    """Every row but 20 (the fifth of the second tile) replaced: row 20 of the collection call and of evaluate_actions keeps its
    bits, the log-prob's sum over the four lanes included."""
    pol, _ = policy_for(D, A, trunk)
    ref = reference(D, A, trunk)
    rng = np.random.default_rng(2)
    keep = lambda x: np.where((np.arange(len(x)) == 20).reshape(-1, *[1] * (x.ndim - 1)), x, rng.normal(size=x.shape).astype(x.dtype))
    whole = run(pol, ref["obs"])
    pol.calls = 0
    other = run(pol, {k: keep(v) for k, v in ref["obs"].items()})
    for k in NAMES:
        assert np.array_equal(bits(whole[k][20]), bits(other[k][20])), k
    assert not np.array_equal(bits(whole["mean"][21]), bits(other["mean"][21]))
    batch = batch_for(D, A, trunk, B)
    mb = samples(batch)
    scrambled = samples(dict(batch, obs={k: keep(np.asarray(v, np.float32)) for k, v in batch["obs"].items()},
                             actions=keep(np.asarray(batch["actions"], np.float32))))
    a = pol.evaluate_actions(mb.observations, mb.actions)
    b = pol.evaluate_actions(scrambled.observations, scrambled.actions)
    for x, y in zip(a, b):
        assert torch.equal(x[20].view(torch.int32), y[20].view(torch.int32))
    assert not torch.equal(a[0][21], b[0][21]) and not torch.equal(a[1][21], b[1][21])


# ------------------------------------------------------------------------------------------------------------- update
def padding_columns(pol):
    """-> the blob positions of both first layers' feature columns >= D + 6."""
    from mycobotgym_amd.policy import pack
    D, A = pol.obs_dim, pol.act_dim
    F, Fp = D + 6, (D + 6 + 3) // 4 * 4
    zeros = {k: torch.zeros_like(v).cpu() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    fn = lambda sd: pack(sd, D, A, pol.pi, pol.vf)
    mask = psc.padding_columns(fn, zeros, "mlp_extractor.policy_net.0.weight", slice(0, F), Fp)
    mask |= psc.padding_columns(fn, zeros, "mlp_extractor.value_net.0.weight", slice(0, F), Fp)
    assert int(mask.sum()) == (pol.pi[0] + pol.vf[0]) * (Fp - F)
    return mask


@pytest.mark.parametrize("D,A,trunk,B,variant", [c + ("ppo-norm-ent",) for c in psc.CASES] + [c + ("a2c",) for c in psc.THREE_LAYER_75])
def test_gradient_parity(built, D, A, trunk, B, variant):
    """Every gradient tensor and stat under the yardstick; +0.0 at every padding position of the gradient blob (the head's rows >= A
    and log_std's among them); and, directly, +0.0 in every first-layer column >= D + 6, where a missing `kb < nkb` or `cols` guard
    would show."""
    pol, opt = upd.check_gradient_parity(D, A, trunk, B, variant)
    opt.grad_blob.fill_(float("nan"))
    opt.compute_grad(samples(batch_for(D, A, trunk, B)))
    g = opt.grad_blob.cpu()
    assert torch.isfinite(g).all()
    assert not bits(g.numpy()[padding_mask(pol)]).any()
    assert not g.view(torch.int32)[padding_columns(pol)].any()
    named = opt.grad(samples(batch_for(D, A, trunk, B)))
    assert all((v != 0).any() for v in named.values())


@pytest.mark.parametrize("D,A,trunk,B", psc.BIT_CASES)
def test_determinism_and_ragged_filler(built, D, A, trunk, B):
    upd.check_determinism_and_ragged_filler(D, A, trunk, B)


@pytest.mark.parametrize("D,A,trunk,B", psc.THREE_LAYER_75)
def test_five_steps_against_the_twin(built, D, A, trunk, B):
    """Afterwards the blob, the gradient and both moments are +0.0 at every padding position and pack(unpack(blob)) gives the blob
    back: Adam touched every float of a three-layer blob and no padding."""
    from mycobotgym_amd.policy import pack, unpack
    pol, opt = upd.check_five_steps_against_the_twin(D, A, trunk, B)
    pad = padding_mask(pol)
    for name, t in (("grad", opt.grad_blob), ("m", opt.m), ("v", opt.v), ("blob", pol._blob)):
        assert not bits(t.cpu().numpy()[pad]).any(), name
    shape = (pol.obs_dim, pol.act_dim, pol.pi, pol.vf)
    assert torch.equal(pack(unpack(pol._blob, *shape), *shape, device="cuda").view(torch.int32), pol._blob.view(torch.int32))
    assert all((v != 0).any() for v in unpack(opt.v, *shape).values())                               # every tensor was stepped


@pytest.mark.parametrize("D,A,trunk,B", psc.STRAY_CASES)
def test_no_stray_writes(built, D, A, trunk, B):
    """Two PPOUpdate.step calls and an evaluate_actions call with sentinel borders around `work` (of exactly the size the C side asks
    for), the gradient, both moments, the stats, the norm, the policy's blob and the three outputs; the results are those of a run
    on plain tensors, bit for bit."""
    mb = samples(batch_for(D, A, trunk, B))
    plain_pol, plain = updater(D, A, trunk, "ppo-norm-ent")
    plain.step(mb); plain.step(mb)
    pol, opt = updater(D, A, trunk, "ppo-norm-ent")
    full = {}
    full["blob"], inner = psc.bordered(pol.blob_floats, pol._blob)
    pol._blob = inner
    pol._cbuf.blob = inner.data_ptr()
    need = int(pol._lib.mcg_policy_grad_work_floats(C.byref(pol._cbuf), C.c_int64(B)))
    assert need > 0
    for name, n, fill in (("grad_blob", pol.blob_floats, None), ("m", pol.blob_floats, 0.0), ("v", pol.blob_floats, 0.0), ("stats", 8, None),
                          ("grad_norm", 4, None), ("_work", need, None)):
        full[name], view = psc.bordered(n, fill)
        setattr(opt, name, view)
    outs = {}
    for name in ("value", "log_prob", "entropy"):
        full[name], outs[name] = psc.bordered(B)
    opt.step(mb); opt.step(mb)
    pol.evaluate_actions(mb.observations, mb.actions, out=outs)
    torch.cuda.synchronize()
    assert opt._work.numel() == need and opt._work.data_ptr() == full["_work"].data_ptr() + 4 * psc.BORDER      # not replaced
    for name, t in full.items():
        assert psc.borders_intact(t), name
    assert (opt.grad_norm[1:] == psc.SENTINEL).all()
    for x, y in ((pol._blob, plain_pol._blob), (opt.grad_blob, plain.grad_blob), (opt.m, plain.m), (opt.v, plain.v), (opt.stats, plain.stats)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    assert all(torch.isfinite(v).all() and not (v == psc.SENTINEL).any() for v in outs.values())


def test_checkpoint_continues_bit_for_bit(built):
    """state_dict after three steps, reloaded into a fresh three-layer policy and updater, continues bit for bit; the moments under
    SB3's names pack to the same blobs."""
    from mycobotgym_amd import ActorCritic, PPOUpdate
    D, A, trunk, B = 12, 13, "80x16x112-relu-96x240x16", 75
    pi, vf, act = ip.TRUNKS[trunk]
    mbs = [samples(batch_for(D, A, trunk, B, seed=5 + s)) for s in range(5)]
    pol, opt = updater(D, A, trunk, "ppo-norm-ent")
    for mb in mbs[:3]:
        opt.step(mb)
    saved_pol, saved_opt = pol.state_dict(), opt.state_dict()
    for mb in mbs[3:]:
        opt.step(mb)
    pol2 = ActorCritic(num_envs=N, obs_dim=D, act_dim=A, hidden=dict(pi=pi, vf=vf), activation=act, seed=999)
    opt2 = PPOUpdate(pol2, learning_rate=1.0, loss="a2c")
    pol2.load_state_dict(saved_pol)
    opt2.load_state_dict(saved_opt)
    assert (opt2.steps, opt2.loss, opt2.learning_rate, opt2.ent_coef) == (3, "ppo", 3e-4, 0.01)
    for mb in mbs[3:]:
        opt2.step(mb)
    for x, y in ((pol._blob, pol2._blob), (opt.m, opt2.m), (opt.v, opt2.v), (opt.grad_blob, opt2.grad_blob), (opt.stats, opt2.stats)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    named = {k: v for k, v in saved_opt.items() if k not in ("m", "v")}
    opt3 = PPOUpdate(updater(D, A, trunk)[0])
    opt3.load_state_dict(named)
    assert torch.equal(opt3.m.view(torch.int32), saved_opt["m"].view(torch.int32)) and torch.equal(opt3.v.view(torch.int32), saved_opt["v"].view(torch.int32))
    obs = dev(ip.random_obs(N, D, seed=5))
    for x, y in zip(pol(obs), pol2(obs)):                            # the same call number: the same noise on the same weights
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
