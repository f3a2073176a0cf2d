"""SAC's update on the GPU (mycobotgym_amd/sac_update.py, csrc/mcg_sac_grad.hip) against the restated losses with autograd in float64
(tests/indep_sac_update.py).

The yardstick is test_gpu_policy_update.py's ``assert_yardstick``, imported: per tensor, the kernel's max-abs error against float64
over the tensor's scale may be at most 10 x the float32 eager twin's own, floored at 2^-23.  The measured ratios are in
profiles/sac_update/parity.md.  B = 75 is four full tiles of 16 samples and one of 11; B = 600 is 38 tiles in parts of unequal length
(13 parts of 3 tiles and a last one of 2 up to width 64, 4 parts of 10 with a last one of 8 above); B = 1 is one sample.

The actor-loss draw cannot be compared bit for bit with ``pol(obs)`` or ``td_target``: their noise is of other Philox domains (7, 8),
and no existing entry takes the noise from the caller.  Its action and log-prob are compared under the yardstick, its noise with the
Python Philox bit for bit, and its Q-values bit for bit with ``q_values`` on the action it wrote."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import indep_sac as isac
from tests import indep_sac_update as su
from tests.test_gpu_policy_update import assert_yardstick, host
from tests.test_gpu_sac import ALPHA, GAMMA, LOG_ALPHA, SEED, bits, dev_batch, no_sync, ulps32

pytestmark = pytest.mark.gpu

N = 40
MID = ("action", "noise", "q_pi", "dq_da")
assert SEED == su.NOISE_SEED


@functools.lru_cache(maxsize=None)
def reference(D, A, trunk, B, auto=True):
    """Computed once per case and shared, and left unchanged: the twins, the batch, the float64 gradients and the float32 twin's."""
    t32, t64, batch, eps_t, eps_a, census = su.case(D, A, trunk, B)
    kw = dict(log_alpha=LOG_ALPHA, target_entropy=-float(A)) if auto else dict(alpha=ALPHA)
    return t32, t64, batch, eps_t, eps_a, su.grads(t64, batch, eps_t, eps_a, GAMMA, **kw), su.grads(t32, batch, eps_t, eps_a, GAMMA, **kw)


def policy_of(twin, D, A, trunk, **kw):
    from mycobotgym_amd import SACPolicy
    pi, qf, act = su.TRUNKS[trunk]
    pol = SACPolicy(num_envs=N, obs_dim=D, act_dim=A, hidden=dict(pi=pi, qf=qf), activation=act, seed=SEED, **kw)
    pol.load_state_dict(twin.state_dict())
    pol.log_ent_coef.fill_(LOG_ALPHA)
    return pol


def updater(twin, D, A, trunk, auto=True, **kw):
    from mycobotgym_amd import SACUpdate
    pol = policy_of(twin, D, A, trunk)
    return pol, SACUpdate(pol, gamma=GAMMA, ent_coef="auto" if auto else ALPHA, **kw)


def mid_out(B, A):
    shapes = {"action": (B, A), "noise": (B, A), "q_pi": (2, B), "dq_da": (B, A)}
    return {k: torch.full(shapes[k], float("nan"), device="cuda") for k in MID}


def valid_blobs(pol):
    from mycobotgym_amd import sac_policy as sp
    D, A = pol.obs_dim, pol.act_dim
    for name in ("critic", "critic_target"):
        again = sp.pack_critic(sp.unpack_critic(pol._t[name], D, A, pol.qf, name), D, A, pol.qf, name, device="cuda")
        assert torch.equal(again.view(torch.int32), pol._t[name].view(torch.int32)), name
    again = sp.pack_actor(sp.unpack_actor(pol._t["actor"], D, A, pol.pi), D, A, pol.pi, device="cuda")
    assert torch.equal(again.view(torch.int32), pol._t["actor"].view(torch.int32))


def padding_is_plus_zero(opt):
    """pack(unpack(grad)) writes +0.0 at every padding position and the gradient's own bits elsewhere."""
    from mycobotgym_amd import sac_policy as sp
    pol = opt.policy
    D, A = pol.obs_dim, pol.act_dim
    g = opt.grad_blob
    again = sp.pack_critic(sp.unpack_critic(g["critic"], D, A, pol.qf, "critic"), D, A, pol.qf, "critic", device="cuda")
    assert torch.equal(again.view(torch.int32), g["critic"].view(torch.int32))
    again = sp.pack_actor(sp.unpack_actor(g["actor"], D, A, pol.pi), D, A, pol.pi, device="cuda")
    assert torch.equal(again.view(torch.int32), g["actor"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("D,A,trunk,B,auto", [c + (True,) for c in su.GRAD_CASES] + [(10, 7, "64x64-relu", 75, False),
                                                                                       (25, 8, "48x32-tanh-qf16", 75, False)])
def test_gradients_stats_and_intermediates(built, D, A, trunk, B, auto):
    check_gradients_stats_and_intermediates(D, A, trunk, B, auto)


def check_gradients_stats_and_intermediates(D, A, trunk, B, auto=True):
    """The three gradients per parameter tensor, the stats and q_pi, dq_da, logp, action under the yardstick, with alpha from the
    device (auto) and from the host.  The batches have rows where each clamp acts (the maker's census).  Bit for bit: the noise, q_pi
    against q_values on the action written, +0.0 at every padding position of both gradients."""
    t32, t64, batch, eps_t, eps_a, r64, r32 = reference(D, A, trunk, B, auto)
    pol, opt = updater(t64, D, A, trunk, auto)
    out = mid_out(B, A)
    db = dev_batch(batch)
    got = host(opt.grad(db, out=out))
    torch.cuda.synchronize()
    assert (pol.target_calls, opt.actor_calls, opt.steps) == (0, 0, 0)
    what = f"D={D} A={A} {trunk} B={B} {'auto' if auto else 'host-alpha'}"
    assert set(got) == set(r64["grad"])
    assert_yardstick(got, r32["grad"], r64["grad"], "grad " + what)
    stats = dict(zip(su.STATS, opt.stats.cpu().numpy()[:7].astype(np.float64)))
    assert opt.stats[7].item() == 0.0
    names = [k for k in su.STATS if auto or k != "ent_coef_loss"]
    assert_yardstick(stats, r32["stats"], {k: r64["stats"][k] for k in names}, "stats " + what)
    mid = {"q_pi": out["q_pi"].cpu().numpy(), "dq_da": out["dq_da"].cpu().numpy(), "logp": opt._rows[B][1].cpu().numpy(),
           "action": out["action"].cpu().numpy(), "y": opt._rows[B][0].cpu().numpy()}
    assert_yardstick(mid, r32["mid"], r64["mid"], "mid " + what)
    assert np.array_equal(bits(out["noise"].cpu().numpy()), bits(eps_a))
    q0, q1 = pol.q_values(db.observations, out["action"])
    assert np.array_equal(bits(np.stack([q0.cpu().numpy(), q1.cpu().numpy()])), bits(mid["q_pi"]))
    padding_is_plus_zero(opt)


# ---------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("D,A,trunk,B", [(10, 7, "64x64-relu", 75), (25, 4, "256x256-relu", 75), (25, 8, "48x32-tanh-qf16", 600)])
def test_equal_inputs_give_equal_bits(built, D, A, trunk, B):
    check_equal_inputs_give_equal_bits(D, A, trunk, B)


def check_equal_inputs_give_equal_bits(D, A, trunk, B):
    """Across two calls, and with NaN garbage in `work` and in the rows behind the batch (the tensors are views of the first B rows
    of storage of 16 more rows, which a ragged tile's extra lanes must not read into the result)."""
    _, t64, batch, *_ = reference(D, A, trunk, B)
    pol, opt = updater(t64, D, A, trunk)
    db = dev_batch(batch)
    opt.grad(db)
    first = {k: v.clone() for k, v in opt.grad_blob.items()}
    stats = opt.stats.clone()
    opt._work.fill_(float("nan"))
    opt.grad(db)
    assert all(torch.equal(first[k].view(torch.int32), opt.grad_blob[k].view(torch.int32)) for k in first)

    def behind(x):
        full = torch.full((x.shape[0] + 16,) + tuple(x.shape[1:]), float("nan"), device="cuda")
        full[:x.shape[0]] = x
        return full[:x.shape[0]]
    wide = isac.Batch(observations={k: behind(v) for k, v in db.observations.items()}, actions=behind(db.actions),
                      next_observations={k: behind(v) for k, v in db.next_observations.items()}, dones=behind(db.dones), rewards=behind(db.rewards))
    opt._work.fill_(float("nan"))
    opt.grad_blob["critic"].fill_(7.0); opt.grad_blob["actor"].fill_(7.0)
    opt.grad(wide)
    assert all(torch.equal(first[k].view(torch.int32), opt.grad_blob[k].view(torch.int32)) for k in first)
    assert torch.equal(stats.view(torch.int32), opt.stats.view(torch.int32))


# ------------------------------------------------------------------------------------------------- 3. the min's choice
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-relu"), (25, 4, "256x256-relu")])
def test_the_min_picks_one_critic_per_row(built, D, A, trunk):
    """qf1's head bias raised by 10 max|q|: the actor gradient is bit for bit that with qf1 absent from the min (qf1 := qf0: a tie
    picks qf0).  Likewise with qf0 raised and qf0 := qf1.  And in the batch as it is, a row's dq_da is the chosen critic's alone."""
    B = 75
    _, t64, batch, *_ = reference(D, A, trunk, B)
    db = dev_batch(batch)
    pol, opt = updater(t64, D, A, trunk)
    out = mid_out(B, A)
    opt.grad(db, out=out)
    q = out["q_pi"].cpu().numpy()
    chosen, own = (q[1] < q[0]), out["dq_da"].cpu().numpy()
    assert 8 <= chosen.sum() <= B - 8
    big = 10.0 * float(np.abs(q).max())
    half = pol.critic_floats // 2
    base = pol._t["critic"].clone()
    head_bias = half - 16                                           # the last 16 floats of a critic: its head's bias, row 0 first
    forced = {}
    for k in (0, 1):                                                # k: the critic that stays in the min
        pol._t["critic"].copy_(base)
        pol._t["critic"][(1 - k) * half + head_bias] += big
        o = mid_out(B, A)
        opt.grad(db, out=o)
        raised = opt.grad_blob["actor"].clone()
        assert ((o["q_pi"][1] < o["q_pi"][0]).cpu().numpy() == bool(k)).all()
        pol._t["critic"].copy_(base)
        pol._t["critic"][(1 - k) * half:(2 - k) * half] = base[k * half:(k + 1) * half]
        opt.grad(db)
        assert torch.equal(raised.view(torch.int32), opt.grad_blob["actor"].view(torch.int32)), k
        forced[k] = o["dq_da"].cpu().numpy()
    for k in (0, 1):
        rows = chosen == bool(k)
        assert np.array_equal(bits(own[rows]), bits(forced[k][rows])), k


# ------------------------------------------------------------------------------------------------------------ 4. Adam
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-relu"), (25, 8, "48x32-tanh-qf16")])
def test_adam_on_the_kernels_own_gradient(built, D, A, trunk):
    """One step, then a second with the moments of the first, on both blobs and the scalar against the float64 rule: within one ulp
    of the parameter plus 1e-5 of the step (lr)."""
    B, lr = 75, 3e-4
    _, t64, batch, *_ = reference(D, A, trunk, B)
    pol, opt = updater(t64, D, A, trunk, learning_rate=lr)
    opt.grad(dev_batch(batch))
    state = {}
    for step in (1, 2):
        opt.steps = step
        for k in ("critic", "actor", "log_ent_coef"):
            p = pol._t[k]
            before, g = p.cpu().numpy().astype(np.float64), opt.grad_blob[k].cpu().numpy()
            m, v = state.get(k, (np.zeros_like(before), np.zeros_like(before)))
            want, m, v = su.adam_step(before, g, m, v, step, lr=lr)
            state[k] = (m, v)
            if k == "log_ent_coef":
                opt._alpha_step(opt._rows[B][1], B, lr)
            else:
                opt._adam(k)
            got = p.cpu().numpy().astype(np.float64)
            assert (np.abs(got - want) <= ulps32(want) + 1e-5 * lr).all(), (k, step, np.abs(got - want).max())
            assert (got[g == 0.0] == before[g == 0.0]).all() and np.abs(got - before).max() > 0.5 * lr
            assert np.allclose(opt.m[k].cpu().numpy(), m, rtol=1e-5, atol=1e-12) and np.allclose(opt.v[k].cpu().numpy(), v, rtol=1e-5, atol=1e-20)
    valid_blobs(pol)


# ---------------------------------------------------------------------------------------------------- 5. five steps
def run_twin(twin, batch, A, steps, **kw):
    state = {"log_ent_coef": LOG_ALPHA}
    before = {k: v.detach().clone().double().numpy() for k, v in twin.state_dict().items()}
    stats = []
    for s in range(steps):
        eps_t, eps_a = isac.noise(isac.DOMAIN_TARGET, SEED, s, len(batch.actions), A), isac.noise(su.DOMAIN_ACTOR_LOSS, SEED, s, len(batch.actions), A)
        stats.append(su.twin_step(twin, state, batch, eps_t, eps_a, s + 1, gamma=GAMMA, target_entropy=-float(A), **kw))
    delta = {k: v.detach().double().numpy() - before[k] for k, v in twin.state_dict().items()}
    delta["log_ent_coef"] = np.array([state["log_ent_coef"] - LOG_ALPHA])
    return delta, stats


@pytest.mark.parametrize("D,A,trunk,B", [(10, 7, "64x64-relu", 75), (25, 8, "48x32-tanh-qf16", 75), (25, 4, "256x256-relu", 75),
                                         (25, 4, "16-tanh", 600)])
def test_five_steps_against_the_twin_in_sb3s_order(built, D, A, trunk, B):
    check_five_steps_against_the_twin_in_sb3s_order(D, A, trunk, B)


def check_five_steps_against_the_twin_in_sb3s_order(D, A, trunk, B):
    """Each parameter's change over five opt.step calls (the three blobs and log_ent_coef) against the float64 twin stepped in SB3's
    order, under the yardstick with the float32 twin's own five-step error.  A wrong sequence (the actor loss on the old critic, the
    target after the alpha step, alpha's loss on a stale logp) changes the later steps' gradients by parts in a thousand."""
    import copy
    t32, t64, batch, *_ = reference(D, A, trunk, B)
    t32, t64 = copy.deepcopy(t32), copy.deepcopy(t64)
    pol, opt = updater(t64, D, A, trunk)
    before = {k: v.clone() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    db = dev_batch(batch)
    with no_sync():
        opt.step(db)                     # (the first call allocates the scratch)
    for _ in range(4):
        with no_sync():
            opt.step(db)
    torch.cuda.synchronize()
    assert (pol.target_calls, opt.actor_calls, opt.steps) == (5, 5, 5)
    got = {k: v.double().cpu().numpy() - before[k].double().cpu().numpy() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    d64, s64 = run_twin(t64, batch, A, 5)
    d32, s32 = run_twin(t32, batch, A, 5)
    assert set(got) == set(d64)
    assert_yardstick(got, d32, d64, f"five steps D={D} A={A} {trunk} B={B}")
    stats = dict(zip(su.STATS, opt.stats.cpu().numpy()[:7].astype(np.float64)))
    assert_yardstick(stats, s32[-1], s64[-1], f"five steps' last stats D={D} A={A} {trunk} B={B}")
    valid_blobs(pol)


# --------------------------------------------------------------------------------- 6. the target's interval, fixed alpha
def test_target_update_interval_and_fixed_ent_coef(built):
    D, A, trunk, B = 10, 7, "64x64-relu", 75
    _, t64, batch, *_ = reference(D, A, trunk, B)
    db = dev_batch(batch)
    pol, opt = updater(t64, D, A, trunk, target_update_interval=2)
    changed = []
    for _ in range(4):
        held = pol._t["critic_target"].clone()
        opt.step(db)
        changed.append(not torch.equal(held.view(torch.int32), pol._t["critic_target"].view(torch.int32)))
    assert changed == [False, True, False, True]                    # after the second and the fourth step
    assert pol.log_ent_coef.item() != np.float32(LOG_ALPHA)
    pol, opt = updater(t64, D, A, trunk, auto=False)
    held = {k: pol._t[k].clone() for k in ("actor", "critic", "critic_target")}
    for _ in range(2):
        opt.step(db)
    assert bits(pol.log_ent_coef.cpu().numpy())[0] == bits(np.float32(LOG_ALPHA).reshape(1))[0]
    stats = opt.stats.cpu().numpy()
    assert stats[3] == np.float32(ALPHA) and stats[2] == 0.0 and np.isfinite(stats).all()
    assert all(not torch.equal(held[k], pol._t[k]) for k in held)
    assert not opt.m["log_ent_coef"].any() and not opt.v["log_ent_coef"].any()


# ------------------------------------------------------------------------------------------------------ 7. stray writes
@pytest.mark.parametrize("B", [75, 1])
def test_no_stray_writes(built, B):
    """Sentinel borders around grad, work, logp_out, the moments and the three blobs; critic_target and critic are untouched by the
    actor entry, actor by the critic entry, and every blob by both."""
    from mycobotgym_amd import _abi
    D, A, trunk = 25, 8, "48x32-tanh-qf16"
    _, t64, batch, *_ = reference(D, A, trunk, 75)
    pol = policy_of(t64, D, A, trunk)
    L, PAD, S = _abi.load(), 64, 1234.5

    def bordered(n, fill=None):
        full = torch.full((n + 2 * PAD,), S, device="cuda")
        if fill is not None:
            full[PAD:PAD + n] = fill
        return full, full[PAD:PAD + n]
    blobs = {k: bordered(pol._t[k].numel(), pol._t[k]) for k in ("actor", "critic", "critic_target")}
    sac = _abi.McgSac.from_buffer_copy(pol._cbuf)
    for k, (_, inner) in blobs.items():
        setattr(sac, k, inner.data_ptr())
    need = L.mcg_sac_grad_work_floats(C.byref(sac), B)
    assert need > 0
    bufs = {"work": bordered(need), "gc": bordered(pol.critic_floats), "ga": bordered(pol.actor_floats), "logp": bordered(B), "y": bordered(B, 0.25),
            "stats": bordered(8), "mc": bordered(pol.critic_floats, 0.0), "vc": bordered(pol.critic_floats, 0.0), "lec": bordered(1, LOG_ALPHA),
            "m1": bordered(4, 0.0), "v1": bordered(4, 0.0), "g1": bordered(4)}
    mid = {"action": bordered(B * A), "noise": bordered(B * A), "q_pi": bordered(2 * B), "dq_da": bordered(B * A)}
    db = dev_batch(batch)
    keep = [db.observations[k][:B].contiguous() for k in ("observation", "achieved_goal", "desired_goal")] + [db.actions[:B].contiguous()]
    rows = _abi.McgSacRows(**{k: t.data_ptr() for k, t in zip(("obs", "achieved", "desired", "action"), keep)})
    p = lambda name, src=bufs: C.c_void_p(src[name][1].data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    held = {k: full.clone() for k, (full, _) in blobs.items()}
    assert L.mcg_sac_critic_grad(C.byref(sac), C.byref(rows), p("y"), B, p("work"), need, p("gc"), p("stats"), stream) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(held[k], blobs[k][0]) for k in held)
    cout = _abi.McgSacActorGradOut(**{k: mid[k][1].data_ptr() for k in mid})
    assert L.mcg_sac_actor_grad(C.byref(sac), C.byref(rows), B, SEED, 0, 0.0, p("lec"), p("work"), need, p("ga"), p("logp"), p("stats"),
                                C.byref(cout), stream) == 0
    torch.cuda.synchronize()
    assert all(torch.equal(held[k], blobs[k][0]) for k in held)
    assert L.mcg_sac_alpha_step(p("lec"), p("logp"), B, -float(A), p("m1"), p("v1"), 1, 3e-4, 0.9, 0.999, 1e-8, p("g1"), p("stats"), stream) == 0
    assert L.mcg_sac_adam(C.c_void_p(blobs["critic"][1].data_ptr()), p("gc"), p("mc"), p("vc"), pol.critic_floats, 1, 3e-4, 0.9, 0.999, 1e-8,
                          stream) == 0
    torch.cuda.synchronize()
    assert torch.equal(held["actor"], blobs["actor"][0]) and torch.equal(held["critic_target"], blobs["critic_target"][0])
    assert not torch.equal(held["critic"], blobs["critic"][0])
    for name, (full, inner) in list(bufs.items()) + list(mid.items()) + list(blobs.items()):
        assert (full[:PAD] == S).all() and (full[PAD + inner.numel():] == S).all(), name
    for name in ("gc", "ga", "logp", "stats", "action", "noise", "q_pi", "dq_da"):
        inner = (bufs.get(name) or mid.get(name))[1]
        assert torch.isfinite(inner).all() and not (inner == S).all(), name
    assert (bufs["m1"][1][1:] == 0).all() and bufs["m1"][1][0] != 0 and (bufs["g1"][1][1:] == S).all() and bufs["lec"][1][0] != np.float32(LOG_ALPHA)


# --------------------------------------------------------------------------------------------------------- 8. checkpoint
def test_checkpoint_continues_bit_for_bit(built):
    check_checkpoint_continues_bit_for_bit(25, 8, "48x32-tanh-qf16", 75)


def check_checkpoint_continues_bit_for_bit(D, A, trunk, B):
    from mycobotgym_amd import SACUpdate
    _, t64, batch, *_ = reference(D, A, trunk, B)
    db = dev_batch(batch)
    pol, opt = updater(t64, D, A, trunk, target_update_interval=2)
    for _ in range(3):
        opt.step(db)
    saved_pol, saved_opt = pol.state_dict(), opt.state_dict()
    for _ in range(2):
        opt.step(db)
    pol2 = policy_of(t64, D, A, trunk)
    opt2 = SACUpdate(pol2)
    pol2.load_state_dict(saved_pol)
    opt2.load_state_dict(saved_opt)
    assert (opt2.steps, opt2.actor_calls, opt2.target_update_interval, opt2.gamma, pol2.target_calls) == (3, 3, 2, GAMMA, 3)
    for _ in range(2):
        opt2.step(db)
    for k in ("actor", "critic", "critic_target", "log_ent_coef"):
        assert torch.equal(pol._t[k].view(torch.int32), pol2._t[k].view(torch.int32)), k
    for k in opt.m:
        assert torch.equal(opt.m[k].view(torch.int32), opt2.m[k].view(torch.int32)) and torch.equal(opt.v[k].view(torch.int32), opt2.v[k].view(torch.int32))
    assert torch.equal(opt.stats.view(torch.int32), opt2.stats.view(torch.int32))
    named = dict(saved_opt)
    del named["m"], named["v"]
    opt3 = SACUpdate(policy_of(t64, D, A, trunk))
    opt3.load_state_dict(named)                                      # the moments under SB3's names pack to the same blobs
    assert all(torch.equal(opt3.m[k], saved_opt["m"][k]) and torch.equal(opt3.v[k], saved_opt["v"][k]) for k in opt3.m)


# ------------------------------------------------------------------------------------------------------ 9. on the engine
def test_on_the_engine_with_the_her_buffer(built):
    from mycobotgym_amd import HerBuffer, SACPolicy, SACUpdate, make
    n = 64
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=n, max_episode_steps=10, seed=3)
    pol = SACPolicy(envs, hidden=(64, 64), seed=SEED)
    opt = SACUpdate(pol)
    buf = HerBuffer(envs, capacity=40, n_sampled_goal=4, seed=2)
    obs, _ = envs.reset(seed=0)
    buf.start(obs)
    for _ in range(20):
        a = pol(obs)
        out = envs.step(a)
        buf.add(a, *out)
        obs = out[0]
    opt.step(buf.sample(256, check=False))                          # (allocates the scratch)
    stats = [opt.stats.clone()]
    with no_sync():
        for _ in range(4):
            opt.step(buf.sample(256, check=False))
            stats.append(opt.stats.clone())                         # (a device copy: the one PyTorch op here, and the test's own)
        a = pol(obs)
    torch.cuda.synchronize()
    stats = torch.stack(stats).cpu().numpy()
    assert np.isfinite(stats).all() and len(set(stats[:, 0].tolist())) == 5, stats
    assert all(torch.isfinite(pol._t[k]).all() for k in pol._t) and torch.isfinite(a).all()
    assert (opt.steps, opt.actor_calls, pol.target_calls, buf.counters()["sample_give_ups"]) == (5, 5, 5, 0)
    valid_blobs(pol)
    envs.close()


# --------------------------------------------------------------------------------------------------------- 10. refusals
def test_refusals_on_the_device(built):
    from mycobotgym_amd import _abi
    D, A, trunk, B = 10, 7, "64x64-relu", 75
    _, t64, batch, *_ = reference(D, A, trunk, B)
    pol, opt = updater(t64, D, A, trunk)
    db = dev_batch(batch)
    held = {k: v.clone() for k, v in pol._t.items()}

    def refused(fragment, b, **kw):
        with pytest.raises(ValueError, match=fragment):
            opt.step(b, **kw)
    refused("lives on cpu", db._replace(actions=db.actions.cpu()))
    refused("expected float32", db._replace(actions=db.actions.double()))
    refused("expected shape", db._replace(actions=db.actions[:, :A - 1]))
    refused("expected shape", db._replace(rewards=db.rewards[:B - 1]))
    refused("another number of rows", db._replace(next_observations={k: v[:B - 1] for k, v in db.next_observations.items()}))
    refused("picture", db._replace(observations=torch.zeros(B, 3, 8, 8, dtype=torch.uint8, device="cuda")))
    refused("out", db, out={"q_pi": torch.zeros(B, 2, device="cuda")})
    refused("unknown", db, out={"logp": torch.zeros(B, device="cuda")})
    opt.learning_rate = 0.0
    refused("learning_rate", db)
    opt.learning_rate = 3e-4
    assert (opt.steps, opt.actor_calls, pol.target_calls) == (0, 0, 0) and all(torch.equal(held[k], pol._t[k]) for k in held)
    L = _abi.load()
    work, g = torch.empty(1024, device="cuda"), torch.empty(pol.critic_floats, device="cuda")
    rows = _abi.McgSacRows(obs=db.observations["observation"].data_ptr(), achieved=db.observations["achieved_goal"].data_ptr(),
                           desired=db.observations["desired_goal"].data_ptr(), action=db.actions.data_ptr())
    code = L.mcg_sac_critic_grad(C.byref(pol._cbuf), C.byref(rows), work.data_ptr(), B, work.data_ptr(), work.numel(), g.data_ptr(),
                                 opt.stats.data_ptr(), None)
    assert code == _abi.MCG_ERR_ARG and b"work_floats" in L.mcg_last_error()
