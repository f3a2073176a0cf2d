"""TD3's and DDPG's update on the GPU (mycobotgym_amd/td3_update.py, csrc/mcg_td3_grad.hip) against the restated losses with autograd
in float64 (tests/indep_td3.py).

The yardstick is test_gpu_policy_update.py's ``assert_yardstick``, imported: per tensor, the kernel's max-abs error against float64
over the tensor's scale may be at most 10 x the float32 eager twin's own, floored at 2^-23.  The measured ratios are in
profiles/td3/parity.md.  B = 75 is four full tiles of 16 samples and one of 11; B = 600 is 38 tiles in parts of unequal length; B = 1
is one sample."""
import copy

import numpy as np
import pytest
import torch

from tests import indep_td3 as it
from tests.test_gpu_policy_update import assert_yardstick, host
from tests.test_gpu_sac import bits, dev_batch, no_sync
from tests.test_gpu_td3 import SEED, policy_of, reference

pytestmark = pytest.mark.gpu

MID = ("action", "q_pi", "dq_da")
KW = dict(gamma=it.GAMMA, target_policy_noise=it.SIGMA, target_noise_clip=it.CLIP)


def updater(twin, D, A, trunk, nc, **kw):
    from mycobotgym_amd import TD3Update
    pol = policy_of(twin, D, A, trunk, nc)
    return pol, TD3Update(pol, **{**KW, **kw})


def mid_out(B, A):
    shapes = {"action": (B, A), "q_pi": (B,), "dq_da": (B, A)}
    return {k: torch.full(shapes[k], float("nan"), device="cuda") for k in MID}


def blob_bits(pol):
    return {k: v.clone().view(torch.int32) for k, v in pol._t.items()}


def padding_is_plus_zero(opt):
    """pack(unpack(grad)) writes +0.0 at every padding position and the gradient's own bits elsewhere."""
    from mycobotgym_amd import td3_policy as tp
    pol = opt.policy
    D, A, nc = pol.obs_dim, pol.act_dim, pol.n_critics
    g = opt.grad_blob
    again = tp.pack_critic(tp.unpack_critic(g["critic"], D, A, pol.qf, "critic", nc), D, A, pol.qf, "critic", nc, device="cuda")
    assert torch.equal(again.view(torch.int32), g["critic"].view(torch.int32))
    again = tp.pack_actor(tp.unpack_actor(g["actor"], D, A, pol.pi), D, A, pol.pi, device="cuda")
    assert torch.equal(again.view(torch.int32), g["actor"].view(torch.int32))


def valid_blobs(pol):
    """pack(unpack(blob)) is the blob, bit for bit, for all four: the padding is +0.0 and nothing else moved."""
    from mycobotgym_amd import td3_policy as tp
    D, A, nc = pol.obs_dim, pol.act_dim, pol.n_critics
    for name in ("critic", "critic_target"):
        again = tp.pack_critic(tp.unpack_critic(pol._t[name], D, A, pol.qf, name, nc), D, A, pol.qf, name, nc, device="cuda")
        assert torch.equal(again.view(torch.int32), pol._t[name].view(torch.int32)), name
    for name in ("actor", "actor_target"):
        again = tp.pack_actor(tp.unpack_actor(pol._t[name], D, A, pol.pi, name), D, A, pol.pi, name, device="cuda")
        assert torch.equal(again.view(torch.int32), pol._t[name].view(torch.int32)), name


def stats_of(opt) -> dict:
    s = opt.stats.cpu().numpy().astype(np.float64)
    assert not s[5:].any()
    return dict(zip(it.STATS, s[:5]))


# ---------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("D,A,trunk,B,nc", it.CASES)
def test_gradients_stats_and_intermediates(built, D, A, trunk, B, nc):
    check_gradients_stats_and_intermediates(D, A, trunk, B, nc)


def check_gradients_stats_and_intermediates(D, A, trunk, B, nc):
    """Both gradients per parameter tensor, the stats and q_pi, dq_da, action, y under the yardstick.  Bit for bit: q_pi against
    q_values' row 0 on the action written, +0.0 at every padding position of both gradients, and, with two critics, the actor
    gradient with qf1's weights perturbed: the actor loss goes through qf0 alone."""
    t32, t64, batch, n, _ = reference(D, A, trunk, B, nc)
    r64, r32 = it.grads(t64, batch, n), it.grads(t32, batch, n)
    pol, opt = updater(t64, D, A, trunk, nc)
    out = mid_out(B, A)
    db = dev_batch(batch)
    got = host(opt.grad(db, out=out))
    torch.cuda.synchronize()
    assert (pol.target_calls, opt.steps, opt.actor_steps) == (0, 0, 0)
    what = f"D={D} A={A} {trunk} B={B} nc={nc}"
    assert set(got) == set(r64["grad"])
    assert_yardstick(got, r32["grad"], r64["grad"], "grad " + what)
    assert_yardstick(stats_of(opt), r32["stats"], r64["stats"], "stats " + what)
    if nc == 1:
        assert opt.stats[3].item() == 0.0
    mid = {"q_pi": out["q_pi"].cpu().numpy(), "dq_da": out["dq_da"].cpu().numpy(), "action": out["action"].cpu().numpy(),
           "y": opt._rows[B].cpu().numpy()}
    assert_yardstick(mid, r32["mid"], r64["mid"], "mid " + what)
    q = pol.q_values(db.observations, out["action"])
    assert np.array_equal(bits(q[0].cpu().numpy()), bits(mid["q_pi"]))
    padding_is_plus_zero(opt)
    if nc == 2:
        actor = opt.grad_blob["actor"].clone()
        half = pol.critic_floats // 2
        pol._t["critic"][half:] *= 1.7
        opt.grad(db)
        assert torch.equal(actor.view(torch.int32), opt.grad_blob["actor"].view(torch.int32))


# ---------------------------------------------------------------------------------------------------- 2. determinism
@pytest.mark.parametrize("D,A,trunk,B,nc", [(10, 7, "64x64-relu", 75, 2), (25, 4, "256x256-relu", 75, 1), (25, 8, "48x32-tanh-qf16", 600, 1)])
def test_equal_inputs_give_equal_bits(built, D, A, trunk, B, nc):
    check_equal_inputs_give_equal_bits(D, A, trunk, B, nc)


def check_equal_inputs_give_equal_bits(D, A, trunk, B, nc):
    """Across two calls, and with NaN garbage in `work`, in the gradient blobs and in the rows behind the batch (the tensors are views
    of the first B rows of storage of 16 more rows, which a ragged tile's extra lanes must not read into the result)."""
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol, opt = updater(t64, D, A, trunk, nc)
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
    wide = it.Batch(observations={k: behind(v) for k, v in db.observations.items()}, actions=behind(db.actions),
                    next_observations={k: behind(v) for k, v in db.next_observations.items()}, dones=behind(db.dones), rewards=behind(db.rewards))
    opt._work.fill_(float("nan"))
    opt.grad_blob["critic"].fill_(7.0); opt.grad_blob["actor"].fill_(float("nan"))
    opt.grad(wide)
    assert all(torch.equal(first[k].view(torch.int32), opt.grad_blob[k].view(torch.int32)) for k in first)
    assert torch.equal(stats.view(torch.int32), opt.stats.view(torch.int32))
    assert torch.isfinite(opt.stats).all()


# ------------------------------------------------------------------------------------------------------ 3. six steps
def run_twin(twin, batch, A, steps, sigma, clip, **kw):
    """-> per step: every parameter's change since the start, and the stats."""
    before = {k: v.detach().clone().double().numpy() for k, v in twin.state_dict().items()}
    state, deltas, stats = {}, [], []
    for s in range(steps):
        n = it.scaled_noise(it.DOMAIN_TARGET, SEED, s, len(batch.actions), A, sigma, clip)
        stats.append(it.twin_step(twin, state, batch, n, **kw))
        deltas.append({k: v.detach().double().numpy() - before[k] for k, v in twin.state_dict().items()})
    return deltas, stats, state


@pytest.mark.parametrize("D,A,trunk,B,nc,delay", [(10, 7, "64x64-relu", 75, 2, 2), (25, 8, "48x32-tanh-qf16", 75, 2, 3),
                                                  (25, 4, "256x256-relu", 75, 2, 2), (25, 4, "16-tanh", 600, 2, 3),
                                                  (10, 7, "64x64-relu", 75, 1, "ddpg"), (25, 8, "48x32-tanh-qf16", 600, 1, "ddpg")])
def test_six_steps_against_the_twin_in_sb3s_order(built, D, A, trunk, B, nc, delay):
    check_six_steps_against_the_twin_in_sb3s_order(D, A, trunk, B, nc, delay)


def check_six_steps_against_the_twin_in_sb3s_order(D, A, trunk, B, nc, delay):
    """After every one of six opt.step calls, each parameter's change since the start (all four blobs) against the float64 twin stepped
    in SB3's order, under the yardstick with the float32 twin's own error.  On the steps without an actor update, actor, actor_target
    and critic_target keep their bits.  policy_delay 2 and 3, and DDPG's preset (one critic, no delay, no smoothing).

    Adam's eps here is the float64 twin's largest gradient magnitude at the start, not 1e-8.  Adam's early steps are
    lr g / (|g| + eps) per element, whose derivative in g at small |g| is lr / eps: a float32 gradient with an error of 2^-23 of the
    tensor's largest element moves an element with |g| near 1e-8 by about 2^-23 max|g| / 1e-8 of the step, parts in a thousand, in
    any float32 implementation, the eager twin included (its own error there is 1e-3), and which of the two is hit harder is chance.
    With eps >= max|g| the derivative is at most lr / max|g| and the step is as well conditioned as the gradient, so the comparison
    measures the code.  The step counts still matter in full: the bias correction 1 - beta1^step scales every element.
    test_the_actors_adam_counts_actor_updates and the engine test run with the default eps."""
    from mycobotgym_amd import DDPGUpdate
    t32, t64, batch, n0, _ = reference(D, A, trunk, B, nc)
    adam_eps = float(np.float32(max(np.abs(g).max() for g in it.grads(t64, batch, n0)["grad"].values())))
    t32, t64 = copy.deepcopy(t32), copy.deepcopy(t64)
    if delay == "ddpg":
        pol = policy_of(t64, D, A, trunk, nc)
        opt = DDPGUpdate(pol, gamma=it.GAMMA, eps=adam_eps)
        assert (opt.policy_delay, opt.target_policy_noise, opt.target_noise_clip, opt.learning_rate, opt.tau) == (1, 0.0, 0.0, 1e-3, 0.005)
        delay, sigma, clip = 1, 0.0, 0.0
    else:
        pol, opt = updater(t64, D, A, trunk, nc, policy_delay=delay, eps=adam_eps)
        sigma, clip = it.SIGMA, it.CLIP
    before = {k: v.double().cpu().numpy() for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    db = dev_batch(batch)
    opt._buffers(B)                                                  # (allocates the scratch)
    d64, s64, state = run_twin(t64, batch, A, 6, sigma, clip, policy_delay=delay, eps=adam_eps)
    d32, s32, _ = run_twin(t32, batch, A, 6, sigma, clip, policy_delay=delay, eps=adam_eps)
    for s in range(6):
        held = blob_bits(pol)
        with no_sync():
            opt.step(db)
        torch.cuda.synchronize()
        now = blob_bits(pol)
        acted = (s + 1) % delay == 0
        assert not torch.equal(held["critic"], now["critic"])
        for k in ("actor", "actor_target", "critic_target"):
            assert torch.equal(held[k], now[k]) != acted, (s, k)
        assert (opt.steps, opt.actor_steps, pol.target_calls) == (s + 1, (s + 1) // delay, s + 1)
        got = {k: v.double().cpu().numpy() - before[k] for k, v in pol.state_dict().items() if torch.is_tensor(v)}
        assert set(got) == set(d64[s])
        what = f"step {s + 1} D={D} A={A} {trunk} B={B} nc={nc} delay={delay}"
        assert_yardstick(got, d32[s], d64[s], what)
        if (s + 1) >= delay:
            assert_yardstick(stats_of(opt), s32[s], s64[s], "stats " + what)
    assert state["actor_steps"] == opt.actor_steps == 6 // delay
    valid_blobs(pol)
    pol.polyak(1.0)
    assert torch.equal(pol._t["actor"].view(torch.int32), pol._t["actor_target"].view(torch.int32))
    assert torch.equal(pol._t["critic"].view(torch.int32), pol._t["critic_target"].view(torch.int32))


def test_the_actors_adam_counts_actor_updates(built):
    """With policy_delay = 2 the first actor update is Adam's step 1: the change is lr sign(g) wherever |g| is well above eps."""
    D, A, trunk, B, nc = 10, 7, "64x64-relu", 75, 2
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol, opt = updater(t64, D, A, trunk, nc, policy_delay=2)
    db = dev_batch(batch)
    before = pol._t["actor"].clone()
    opt.step(db); opt.step(db)
    g = opt.grad_blob["actor"]
    assert g.abs().max() > 1e-5
    big = g.abs() > 1e-2 * g.abs().max()                            # (|g| >= 1e-7 = 10 eps: the quotient is within a tenth of 1)
    change = (pol._t["actor"] - before)[big]
    assert big.sum() > 100 and torch.allclose(change, -1e-3 * torch.sign(g[big]), rtol=0.12, atol=1e-7)


# --------------------------------------------------------------------------------------------------------- 4. checkpoint
def test_checkpoint_continues_bit_for_bit(built):
    check_checkpoint_continues_bit_for_bit(25, 8, "48x32-tanh-qf16", 75, 2)


def check_checkpoint_continues_bit_for_bit(D, A, trunk, B, nc):
    from mycobotgym_amd import TD3Update
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    db = dev_batch(batch)
    pol, opt = updater(t64, D, A, trunk, nc, policy_delay=2)
    for _ in range(3):
        opt.step(db)
    saved_pol, saved_opt = pol.state_dict(), opt.state_dict()
    for _ in range(3):
        opt.step(db)
    pol2 = policy_of(t64, D, A, trunk, nc)
    opt2 = TD3Update(pol2)
    pol2.load_state_dict(saved_pol)
    opt2.load_state_dict(saved_opt)
    assert (opt2.steps, opt2.actor_steps, opt2.policy_delay, opt2.gamma, opt2.target_policy_noise, pol2.target_calls) == (3, 1, 2, it.GAMMA, it.SIGMA, 3)
    for _ in range(3):
        opt2.step(db)
    for k in pol._t:
        assert torch.equal(pol._t[k].view(torch.int32), pol2._t[k].view(torch.int32)), k
    for k in opt.m:
        assert torch.equal(opt.m[k].view(torch.int32), opt2.m[k].view(torch.int32)) and torch.equal(opt.v[k].view(torch.int32), opt2.v[k].view(torch.int32))
    assert torch.equal(opt.stats.view(torch.int32), opt2.stats.view(torch.int32)) and (opt2.steps, opt2.actor_steps) == (6, 3)
    named = dict(saved_opt)
    del named["m"], named["v"]
    opt3 = TD3Update(policy_of(t64, D, A, trunk, nc))
    opt3.load_state_dict(named)                                      # the moments under SB3's names pack to the same blobs
    assert all(torch.equal(opt3.m[k], saved_opt["m"][k]) and torch.equal(opt3.v[k], saved_opt["v"][k]) for k in opt3.m)


# ------------------------------------------------------------------------------------------------------- 5. refusals
def test_refusals_on_the_device(built):
    from mycobotgym_amd import _abi
    import ctypes as C
    D, A, trunk, B, nc = 10, 7, "64x64-relu", 75, 2
    _, t64, batch, *_ = reference(D, A, trunk, B, nc)
    pol, opt = updater(t64, D, A, trunk, nc)
    db = dev_batch(batch)
    held = blob_bits(pol)

    def refused(fragment, b, **kw):
        for call in (opt.step, opt.grad):
            with pytest.raises(ValueError, match=fragment):
                call(b, **kw)
    refused("lives on cpu", db._replace(actions=db.actions.cpu()))
    refused("expected float32", db._replace(actions=db.actions.double()))
    refused("expected shape", db._replace(actions=db.actions[:, :A - 1]))
    refused("expected shape", db._replace(rewards=db.rewards[:B - 1]))
    refused("another number of rows", db._replace(next_observations={k: v[:B - 1] for k, v in db.next_observations.items()}))
    refused("picture", db._replace(observations=torch.zeros(B, 3, 8, 8, dtype=torch.uint8, device="cuda")))
    refused("out", db, out={"q_pi": torch.zeros(2, B, device="cuda")})                         # shape
    refused("out", db, out={"q_pi": torch.zeros(B, dtype=torch.float64, device="cuda")})      # dtype
    refused("out", db, out={"dq_da": torch.zeros(A, B, device="cuda").t()})                    # layout
    refused("out", db, out={"action": torch.zeros(B, A)})                                      # device
    refused("unknown", db, out={"noise": torch.zeros(B, A, device="cuda")})
    opt.learning_rate = 0.0
    refused("learning_rate", db)
    opt.learning_rate = 1e-3
    assert (opt.steps, opt.actor_steps, pol.target_calls) == (0, 0, 0) and all(torch.equal(held[k], v) for k, v in blob_bits(pol).items())
    L = _abi.load()
    work, g = torch.empty(1024, device="cuda"), torch.empty(pol.critic_floats, device="cuda")
    rows = _abi.McgSacRows(obs=db.observations["observation"].data_ptr(), achieved=db.observations["achieved_goal"].data_ptr(),
                           desired=db.observations["desired_goal"].data_ptr(), action=db.actions.data_ptr())
    code = L.mcg_td3_critic_grad(C.byref(pol._cbuf), C.byref(rows), work.data_ptr(), B, work.data_ptr(), work.numel(), g.data_ptr(),
                                 opt.stats.data_ptr(), None)
    assert code == _abi.MCG_ERR_ARG and b"work_floats" in L.mcg_last_error()


# ---------------------------------------------------------------------------------------------------- 6. on the engine
def test_on_the_engine_with_the_her_buffer(built):
    from mycobotgym_amd import DDPGPolicy, DDPGUpdate, HerBuffer, TD3Policy, TD3Update, make
    n = 64
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=n, max_episode_steps=10, seed=3)
    for Policy, Update in ((TD3Policy, TD3Update), (DDPGPolicy, DDPGUpdate)):
        pol = Policy(envs, hidden=(64, 64), seed=SEED)
        opt = Update(pol)
        buf = HerBuffer(envs, capacity=40, n_sampled_goal=4, seed=2)
        obs, _ = envs.reset(seed=0)
        buf.start(obs)
        for _ in range(20):
            a = pol(obs, noise_std=0.1)
            out = envs.step(a)
            buf.add(a, *out)
            obs = out[0]
        opt.step(buf.sample(256, check=False))                      # (allocates the scratch)
        stats = [opt.stats.clone()]
        with no_sync():
            for _ in range(5):
                opt.step(buf.sample(256, check=False))
                stats.append(opt.stats.clone())                     # (a device copy: the one PyTorch op here, and the test's own)
            a = pol(obs)
        torch.cuda.synchronize()
        stats = torch.stack(stats).cpu().numpy()
        assert np.isfinite(stats).all() and len(set(stats[:, 0].tolist())) == 6, stats
        assert all(torch.isfinite(pol._t[k]).all() for k in pol._t) and torch.isfinite(a).all() and a.abs().max() <= 1.0
        assert (opt.steps, opt.actor_steps, pol.target_calls) == (6, 6 // opt.policy_delay, 6)
    envs.close()
