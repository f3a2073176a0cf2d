"""TD3 and DDPG on the GPU at the shape edges of tests/policy_shape_cases.py: a third layer (n == 3), widths 80..240 in the MT = 16
kernels with partial tiles, actor and critic on different sides of width 64, A in {1, 9, 13, 16} and D in {1, 12, 45, 58}.  The
module's docstring there says which path each case reaches.

The checks are the bodies of tests/test_gpu_td3.py and tests/test_gpu_td3_update.py, called on these cases, under the same
yardstick (``assert_yardstick``: 10 x the float32 eager twin's error against float64, floored at 2^-23 of the tensor's scale); what
is new here is the row-independence check on scrambled rows, the direct check of the padding columns, and the sentinel borders
around everything ``TD3Update.step`` writes.  The measured ratios are in profiles/policy_shapes/parity.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import indep_td3 as it
from tests import policy_shape_cases as psc
from tests import test_gpu_td3 as fwd
from tests import test_gpu_td3_update as upd
from tests.test_gpu_sac import bits, dev, dev_batch
from tests.test_gpu_td3 import N, policy_of, reference
from tests.test_gpu_td3_update import KW, updater

pytestmark = pytest.mark.gpu

COLLECTION = list({(D, A, t, nc): (D, A, t, B, nc) for D, A, t, B, nc in psc.TD3_CASES}.values())      # (the call does not read B)
TWO = lambda cases: [c + (2,) for c in cases]


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("D,A,trunk,B,nc", COLLECTION)
def test_collection_action(built, D, A, trunk, B, nc):
    """The mean and the clamped noisy action under the yardstick; the noise bit for bit with the Python Philox in all A columns
    (pairs 4..7 for A > 8; the dropped second value for an odd A); noise_std = 0 gives the mean's action."""
    fwd.check_collection_action(D, A, trunk, B, nc)


@pytest.mark.parametrize("D,A,trunk,B,nc", psc.TD3_CASES)
def test_q_values_and_td_target(built, D, A, trunk, B, nc):
    """q_values on both blobs and td_target with next_action, next_q and the noise, as test_gpu_td3.py checks them."""
    fwd.check_q_values_and_td_target(D, A, trunk, B, nc)


@pytest.mark.parametrize("D,A,trunk,B,nc", TWO(psc.ROW_CASES))
def test_a_row_does_not_read_its_tiles_other_rows(built, D, A, trunk, B, nc):
    """Every row but 20 (the fifth of the second tile) replaced: row 20 of the collection call, of q_values and of td_target keeps
    its bits."""
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol = policy_of(t64, D, A, trunk, nc)
    rng = np.random.default_rng(2)
    keep = lambda x: np.where((np.arange(len(x)) == 20).reshape(-1, *[1] * (x.ndim - 1)), x, rng.normal(size=x.shape).astype(np.float32))
    obs = {k: v.astype(np.float32) for k, v in it.random_obs(N, D, 77).items()}
    names = ("action", "mean", "noise")
    runs = []
    for o in (obs, {k: keep(v) for k, v in obs.items()}):
        out = {k: torch.full((N, A), float("nan"), device="cuda") for k in names}
        pol.calls = 0
        pol(dev(o), noise_std=0.3, out=out)
        runs.append({k: v.cpu().numpy() for k, v in out.items()})
    for k in names:
        assert np.array_equal(bits(runs[0][k][20]), bits(runs[1][k][20])), k
    assert not np.array_equal(bits(runs[0]["mean"][21]), bits(runs[1]["mean"][21]))
    scrambled = it.Batch(observations={k: keep(v) for k, v in batch.observations.items()}, actions=keep(batch.actions),
                         next_observations={k: keep(v) for k, v in batch.next_observations.items()}, dones=batch.dones, rewards=keep(batch.rewards))
    runs = []
    for b in (batch, scrambled):
        db = dev_batch(b)
        out = {k: torch.full(s, float("nan"), device="cuda") for k, s in pol._target_shapes(B).items()}
        pol.target_calls = 0
        pol.td_target(db, out=out, **KW)
        got = {k: v.cpu().numpy() for k, v in out.items()}
        got["q"] = torch.stack(pol.q_values(db.observations, db.actions)).cpu().numpy()
        runs.append(got)
    for k, v in runs[0].items():
        row = (lambda x: x[:, 20]) if k in ("q", "next_q") else (lambda x: x[20])
        assert np.array_equal(bits(row(v)), bits(row(runs[1][k]))), k
    assert not np.array_equal(bits(runs[0]["target"][21]), bits(runs[1]["target"][21]))


# ------------------------------------------------------------------------------------------------------------- update
def padding_columns(pol):
    """-> the positions, per gradient blob, of the first layers' feature columns >= D + 6 and of the critics' action columns >= A."""
    from mycobotgym_amd import td3_policy as tp
    D, A, nc = pol.obs_dim, pol.act_dim, pol.n_critics
    F, Fp = D + 6, (D + 6 + 3) // 4 * 4
    zeros = {k: torch.zeros_like(v).cpu() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    actor = psc.padding_columns(lambda sd: tp.pack_actor(sd, D, A, pol.pi, "actor"), zeros, "actor.mu.0.weight", slice(0, F), Fp)
    critic = torch.zeros(pol.critic_floats, dtype=torch.bool)
    for q in range(nc):
        pack = lambda sd: tp.pack_critic(sd, D, A, pol.qf, "critic", nc)
        critic |= psc.padding_columns(pack, zeros, f"critic.qf{q}.0.weight", slice(0, F), Fp)
        critic |= psc.padding_columns(pack, zeros, f"critic.qf{q}.0.weight", slice(F, F + A), 16)
    assert int(critic.sum()) == nc * pol.qf[0] * (Fp - F + 16 - A) and int(actor.sum()) == pol.pi[0] * (Fp - F)
    return {"actor": actor, "critic": critic}


@pytest.mark.parametrize("D,A,trunk,B,nc", psc.TD3_CASES)
def test_gradients_stats_and_intermediates(built, D, A, trunk, B, nc):
    """Every gradient tensor, the stats and action, q_pi, dq_da, y under the yardstick; q_pi bit for bit with q_values on the action
    written; +0.0 at every padding position; and, directly, +0.0 in every first-layer column >= D + 6 and every action column >= A,
    where a missing `kb < nkb` or `cols` guard would show."""
    upd.check_gradients_stats_and_intermediates(D, A, trunk, B, nc)
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol, opt = updater(t64, D, A, trunk, nc)
    for k in opt.grad_blob:
        opt.grad_blob[k].fill_(float("nan"))
    opt.grad(dev_batch(batch))
    for k, mask in padding_columns(pol).items():
        g = opt.grad_blob[k].cpu()
        assert torch.isfinite(g).all() and not g.view(torch.int32)[mask].any(), k
        assert (g[~mask] != 0).any(), k


@pytest.mark.parametrize("D,A,trunk,B,nc", TWO(psc.BIT_CASES))
def test_equal_inputs_give_equal_bits(built, D, A, trunk, B, nc):
    upd.check_equal_inputs_give_equal_bits(D, A, trunk, B, nc)


@pytest.mark.parametrize("D,A,trunk,B,nc", TWO(psc.THREE_LAYER_75))
def test_six_steps_against_the_twin_in_sb3s_order(built, D, A, trunk, B, nc):
    """policy_delay = 2, Adam's eps as test_gpu_td3_update.py documents it; afterwards pack(unpack(.)) gives each of the four blobs
    back: Adam and the Polyak step touched every float of a three-layer blob and no padding."""
    upd.check_six_steps_against_the_twin_in_sb3s_order(D, A, trunk, B, nc, 2)


@pytest.mark.parametrize("D,A,trunk,B,nc", TWO(psc.STRAY_CASES))
def test_no_stray_writes(built, D, A, trunk, B, nc):
    """Two TD3Update.step calls (policy_delay = 2: a critic step, then a critic and an actor step with the Polyak step) with sentinel
    borders around `work` (of exactly the size the C side asks for), both gradient blobs, the four moments, the four policy blobs, y,
    the stats and the actor entry's three outputs; the results are those of a run on plain tensors, bit for bit."""
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    db = dev_batch(batch)
    plain_pol, plain = updater(t64, D, A, trunk, nc, policy_delay=2)
    plain.step(db); plain.step(db)
    pol, opt = updater(t64, D, A, trunk, nc, policy_delay=2)
    full = {}
    for k in list(pol._t):
        full["blob " + k], inner = psc.bordered(pol._t[k].numel(), pol._t[k])
        pol._t[k] = inner
        setattr(pol._cbuf, k, inner.data_ptr())
    for k in ("critic", "actor"):
        full["grad " + k], opt.grad_blob[k] = psc.bordered(opt.grad_blob[k].numel())
        full["m " + k], opt.m[k] = psc.bordered(opt.m[k].numel(), 0.0)
        full["v " + k], opt.v[k] = psc.bordered(opt.v[k].numel(), 0.0)
    need = int(pol._lib.mcg_td3_grad_work_floats(C.byref(pol._cbuf), C.c_int64(B)))
    assert need > 0
    full["work"], opt._work = psc.bordered(need)
    full["stats"], opt.stats = psc.bordered(8, 0.0)
    full["y"], y = psc.bordered(B)
    opt._rows = {B: y}
    out = {}
    for k, shape in (("action", (B, A)), ("q_pi", (B,)), ("dq_da", (B, A))):
        full[k], inner = psc.bordered(int(np.prod(shape)))
        out[k] = inner.view(shape)
    opt.step(db); opt.step(db, out=out)
    torch.cuda.synchronize()
    assert opt._work.numel() == need and opt._work.data_ptr() == full["work"].data_ptr() + 4 * psc.BORDER      # not replaced
    for name, t in full.items():
        assert psc.borders_intact(t), name
    for k in pol._t:
        assert torch.equal(pol._t[k].view(torch.int32), plain_pol._t[k].view(torch.int32)), k
    for k in opt.grad_blob:
        assert torch.equal(opt.grad_blob[k].view(torch.int32), plain.grad_blob[k].view(torch.int32)), k
        assert torch.equal(opt.m[k].view(torch.int32), plain.m[k].view(torch.int32)) and torch.equal(opt.v[k].view(torch.int32), plain.v[k].view(torch.int32))
    assert torch.equal(opt.stats.view(torch.int32), plain.stats.view(torch.int32))
    for k, v in out.items():
        assert torch.isfinite(v).all() and not (v == psc.SENTINEL).any(), k
    upd.valid_blobs(pol)


def test_checkpoint_continues_bit_for_bit(built):
    upd.check_checkpoint_continues_bit_for_bit(12, 13, "80x16x112-relu-96x240x16", 75, 2)
