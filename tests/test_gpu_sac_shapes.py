"""SAC on the GPU at the shape edges of tests/policy_shape_cases.py: a third layer (n == 3), widths 80..240 in the MT = 16 kernels
with partial tiles, actor and critic on different sides of width 64, A in {1, 9, 13, 16} and D in {1, 12, 45, 58}.  The module's
docstring there says which path each case reaches.

The checks are the bodies of tests/test_gpu_sac.py and tests/test_gpu_sac_update.py, called on these cases, under the same bounds
(``assert_parity`` and ``assert_yardstick``: 10 x the float32 eager twin's error against float64, floored at 2^-23 of the output's
scale); what is new here is the row-independence check on scrambled rows, the direct check of the padding columns, and the sentinel
borders around everything ``SACUpdate.step`` writes.  The measured ratios are in profiles/policy_shapes/parity.md."""
import ctypes as C

import numpy as np
import pytest
import torch

from tests import indep_sac as isac
from tests import policy_shape_cases as psc
from tests import test_gpu_sac as fwd
from tests import test_gpu_sac_update as upd
from tests.test_gpu_sac import bits, dev_batch, policy_for, reference, run_act, run_q, run_target
from tests.test_gpu_sac_update import updater

pytestmark = pytest.mark.gpu


# ------------------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("D,A,trunk,B", psc.CASES)
def test_parity_with_the_float64_rule(built, D, A, trunk, B):
    """Every output of the collection call (N = 40), of q_values on both blobs and of td_target with all its intermediates (B rows).
    Both clamp bounds of log_std act in the float64 reference of every case with A >= 9, and there the kernel's must too; the
    clamp masks are equal at every case."""
    ref = reference(D, A, trunk, rows=B)
    both = bool((ref["log_std"] == 2.0).any() and (ref["log_std"] == -20.0).any())
    assert both or A < 9
    fwd.check_parity_with_the_float64_rule(D, A, trunk, B, both_bounds=both)


@pytest.mark.parametrize("D,A,trunk,B", psc.CASES)
def test_noise_squashing_and_deterministic(built, D, A, trunk, B):
    """The noise of both domains bit for bit with the Python Philox in all A columns (pairs 4..7 for A > 8; the dropped second value
    for an odd A); the action is tanh of the kernel's own pre-squash value; deterministic=True gives tanh of the mean."""
    fwd.check_noise_squashing_and_deterministic(D, A, trunk, B)


@pytest.mark.parametrize("D,A,trunk,B", psc.ROW_CASES)
def test_a_row_does_not_read_its_tiles_other_rows(built, D, A, trunk, B):
    """Every row but 20 (the fifth of the second tile) replaced: row 20 of the collection call, of q_values and of td_target keeps
    its bits, the log-prob's sum over the four lanes included."""
    ref = reference(D, A, trunk, rows=B)
    pol = policy_for(D, A, trunk)
    rng = np.random.default_rng(2)
    keep = lambda x: np.where((np.arange(len(x)) == 20).reshape(-1, *[1] * (x.ndim - 1)), x, rng.normal(size=x.shape).astype(x.dtype))
    whole = run_act(pol, ref["obs"])
    pol.calls = 0
    other = run_act(pol, {k: keep(v) for k, v in ref["obs"].items()})
    for k in whole:
        assert np.array_equal(bits(whole[k][20]), bits(other[k][20])), k
    assert not np.array_equal(bits(whole["mean"][21]), bits(other["mean"][21]))
    b = ref["batch"]
    scrambled = isac.Batch(observations={k: keep(v) for k, v in b.observations.items()}, actions=keep(b.actions),
                           next_observations={k: keep(v) for k, v in b.next_observations.items()}, dones=b.dones, rewards=keep(b.rewards))
    full, qfull = run_target(pol, b), run_q(pol, b.observations, b.actions)
    pol.target_calls = 0
    fwd.same_bits(fwd.rows_of_out(run_target(pol, scrambled), 20), full, slice(20, 21))
    q = run_q(pol, scrambled.observations, scrambled.actions)
    assert np.array_equal(bits(q[:, 20]), bits(qfull[:, 20])) and not np.array_equal(bits(q[:, 21]), bits(qfull[:, 21]))


# ------------------------------------------------------------------------------------------------------------- update
def padding_columns(pol):
    """-> the positions, per gradient blob, of the first layers' feature columns >= D + 6 and of the critics' action columns >= A."""
    from mycobotgym_amd import sac_policy as sp
    D, A = pol.obs_dim, pol.act_dim
    F, Fp = D + 6, (D + 6 + 3) // 4 * 4
    zeros = {k: torch.zeros_like(v).cpu() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    actor = psc.padding_columns(lambda sd: sp.pack_actor(sd, D, A, pol.pi), zeros, "actor.latent_pi.0.weight", slice(0, F), Fp)
    critic = torch.zeros(pol.critic_floats, dtype=torch.bool)
    pack = lambda sd: sp.pack_critic(sd, D, A, pol.qf, "critic")
    for q in range(2):
        critic |= psc.padding_columns(pack, zeros, f"critic.qf{q}.0.weight", slice(0, F), Fp)
        critic |= psc.padding_columns(pack, zeros, f"critic.qf{q}.0.weight", slice(F, F + A), 16)
    assert int(critic.sum()) == 2 * pol.qf[0] * (Fp - F + 16 - A) and int(actor.sum()) == pol.pi[0] * (Fp - F)
    return {"actor": actor, "critic": critic}


@pytest.mark.parametrize("D,A,trunk,B", psc.CASES)
def test_gradients_stats_and_intermediates(built, D, A, trunk, B):
    """The three gradients per tensor, the stats and action, q_pi, dq_da, logp, y under the yardstick; the noise bit for bit; q_pi bit
    for bit with q_values on the action written; +0.0 at every padding position; and, directly, +0.0 in every first-layer column
    >= D + 6 and every action column >= A, where a missing `kb < nkb` or `cols` guard would show."""
    upd.check_gradients_stats_and_intermediates(D, A, trunk, B)
    _, t64, batch, *_ = upd.reference(D, A, trunk, B, True)
    pol, opt = updater(t64, D, A, trunk)
    for k in ("actor", "critic"):
        opt.grad_blob[k].fill_(float("nan"))
    opt.grad(dev_batch(batch))
    for k, mask in padding_columns(pol).items():
        g = opt.grad_blob[k].cpu()
        assert torch.isfinite(g).all() and not g.view(torch.int32)[mask].any(), k
        assert (g[~mask] != 0).any(), k


@pytest.mark.parametrize("D,A,trunk,B", psc.BIT_CASES)
def test_equal_inputs_give_equal_bits(built, D, A, trunk, B):
    upd.check_equal_inputs_give_equal_bits(D, A, trunk, B)


@pytest.mark.parametrize("D,A,trunk,B", psc.THREE_LAYER_75)
def test_five_steps_against_the_twin_in_sb3s_order(built, D, A, trunk, B):
    """Afterwards pack(unpack(.)) gives each blob back: Adam and the Polyak step touched every float of a three-layer blob and no
    padding."""
    upd.check_five_steps_against_the_twin_in_sb3s_order(D, A, trunk, B)


@pytest.mark.parametrize("D,A,trunk,B", psc.STRAY_CASES)
def test_no_stray_writes(built, D, A, trunk, B):
    """Two SACUpdate.step calls with sentinel borders around `work` (of exactly the size the C side asks for), the three gradients,
    the six moments, the three policy blobs and log_ent_coef, y, logp, the stats and the actor entry's four outputs; the results are
    those of a run on plain tensors, bit for bit."""
    _, t64, batch, *_ = upd.reference(D, A, trunk, B, True)
    db = dev_batch(batch)
    plain_pol, plain = updater(t64, D, A, trunk)
    plain.step(db); plain.step(db)
    pol, opt = updater(t64, D, A, trunk)
    full = {}
    for k in list(pol._t):
        full["blob " + k], inner = psc.bordered(pol._t[k].numel(), pol._t[k])
        pol._t[k] = inner
        if k != "log_ent_coef":
            setattr(pol._cbuf, k, inner.data_ptr())
    for k in ("critic", "actor", "log_ent_coef"):
        full["grad " + k], opt.grad_blob[k] = psc.bordered(opt.grad_blob[k].numel())
        full["m " + k], opt.m[k] = psc.bordered(opt.m[k].numel(), 0.0)
        full["v " + k], opt.v[k] = psc.bordered(opt.v[k].numel(), 0.0)
    need = int(pol._lib.mcg_sac_grad_work_floats(C.byref(pol._cbuf), C.c_int64(B)))
    assert need > 0
    full["work"], opt._work = psc.bordered(need)
    full["stats"], opt.stats = psc.bordered(8, 0.0)
    full["y"], y = psc.bordered(B)
    full["logp"], logp = psc.bordered(B)
    opt._rows = {B: (y, logp)}
    out = {}
    for k, shape in (("action", (B, A)), ("noise", (B, A)), ("q_pi", (2, B)), ("dq_da", (B, A))):
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
    upd.check_checkpoint_continues_bit_for_bit(12, 9, "32x48x16-tanh-16x48x32", 75)
