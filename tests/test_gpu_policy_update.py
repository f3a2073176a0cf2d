"""The policy update on the GPU (mycobotgym_amd/policy_update.py, csrc/mcg_policy_grad.hip) against the restated loss with autograd in
float64 (tests/indep_ppo.py).

The yardstick is test_gpu_policy.py's: the kernel's error against float64 may be at most 10 x the error of the float32 eager twin on
the same inputs -- here per parameter tensor (and per stat), as max-abs error over the float64 tensor's max-abs, the twin's error
floored at 2^-23 (a float32 result cannot be asked for better than an ulp of its own scale).  The measured ratios are in
profiles/policy_update/parity.md.

B = 75 is four full tiles of 16 samples and one of 11 (5 parts of one tile); B = 600 is 38 tiles: 13 parts of 3 tiles with a last one
of 2 where the widest layer has at most 64 units, 4 parts of 10 with a last one of 8 above; B = 1 skips the normalisation."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

from tests import indep_policy as ip
from tests import indep_ppo as pp
from tests.test_gpu_policy import bits, dev, policy_for, ulps32

pytestmark = pytest.mark.gpu

FLOOR = 2.0 ** -23
SHAPES = [(D, A, name) for (D, A) in ip.DIMS for name in ("64x64-tanh", "48x32-relu-vf16", "16-tanh")] + [(25, 4, "256x256-relu")]
VARIANTS = {"ppo-norm": dict(loss="ppo", normalize_advantage=True, ent_coef=0.0), "ppo": dict(loss="ppo", normalize_advantage=False, ent_coef=0.0),
            "ppo-norm-ent": dict(loss="ppo", normalize_advantage=True, ent_coef=0.01), "a2c": dict(loss="a2c", normalize_advantage=True, ent_coef=0.01)}
GRAD_CASES = ([(D, A, t, 75, "ppo-norm") for D, A, t in SHAPES]
              + [(10, 7, t, 75, v) for t in ("64x64-tanh", "48x32-relu-vf16") for v in ("ppo", "ppo-norm-ent", "a2c")]
              + [(25, 4, "256x256-relu", 75, "a2c"), (25, 4, "256x256-relu", 75, "ppo-norm-ent")]
              + [(D, A, t, B, "ppo-norm-ent") for (D, A, t) in ((10, 7, "64x64-tanh"), (25, 8, "48x32-relu-vf16"), (25, 4, "256x256-relu"))
                 for B in (600, 1)])


def twins(D, A, trunk, weights_seed=3):
    pi, vf, act = ip.TRUNKS[trunk]
    return ip.Twin(D, A, pi, vf, act).randomize(weights_seed), ip.Twin(D, A, pi, vf, act).randomize(weights_seed).double()


@functools.lru_cache(maxsize=None)
def batch_for(D, A, trunk, B, seed=5):
    _, twin64 = twins(D, A, trunk)
    return pp.make_batch(twin64, D, A, B, seed=seed, relu=ip.TRUNKS[trunk][2] == "relu")[0]


@functools.lru_cache(maxsize=None)
def reference(D, A, trunk, B, variant, seed=5):
    """Computed once per case and shared: the float64 gradient and stats, and the float32 twin's."""
    twin32, twin64 = twins(D, A, trunk)
    batch = batch_for(D, A, trunk, B, seed)
    g64, s64 = pp.grad_and_stats(twin64, batch, **VARIANTS[variant])
    g32, s32 = pp.grad_and_stats(twin32, batch, **VARIANTS[variant])
    return g64, s64, g32, s32


def samples(batch, rows=None, fill=0.0):
    """The batch as RolloutBuffer.get yields it, on the device; ``rows``: the tensors are views of the first B rows of storage of
    that many rows, the others hold ``fill``."""
    from mycobotgym_amd import RolloutSamples
    B = len(batch["actions"])
    def put(x):
        x = np.asarray(x, np.float32)
        full = np.full((rows or B,) + x.shape[1:], fill, np.float32)
        full[:B] = x
        return torch.from_numpy(full).cuda()[:B]
    return RolloutSamples(observations={k: put(v) for k, v in batch["obs"].items()}, actions=put(batch["actions"]),
                          old_values=put(np.zeros(B)), old_log_prob=put(batch["old_log_prob"]), advantages=put(batch["advantages"]),
                          returns=put(batch["returns"]), index=torch.zeros(B, dtype=torch.int32, device="cuda"))


def updater(D, A, trunk, variant="ppo-norm", **kw):
    from mycobotgym_amd import PPOUpdate
    pol, _ = policy_for(D, A, trunk)
    return pol, PPOUpdate(pol, **dict(VARIANTS[variant], **kw))


def rel(x, ref):
    scale = np.abs(ref).max()
    return np.abs(np.asarray(x, np.float64) - ref).max() / scale if scale > 0 else np.abs(np.asarray(x, np.float64)).max()


def assert_yardstick(got: dict, twin: dict, ref: dict, what):
    lines, bad = [], []
    for k, r in ref.items():
        r = np.asarray(r, np.float64)
        ke, te = rel(got[k], r), max(rel(twin[k], r), FLOOR)
        lines.append(f"parity {what} {k}: kernel {ke:.3e}, twin {te:.3e}, ratio {ke / te:.2f}")
        if not ke <= 10.0 * te:
            bad.append(lines[-1])
    print("\n".join(lines))
    assert not bad, bad


def host(sd: dict) -> dict:
    return {k: v.detach().cpu().numpy() for k, v in sd.items() if torch.is_tensor(v)}


# ------------------------------------------------------------------------------------------------- 1. evaluate_actions
@pytest.mark.parametrize("D,A,trunk", SHAPES)
def test_evaluate_actions_parity(built, D, A, trunk):
    check_evaluate_actions_parity(D, A, trunk)


def check_evaluate_actions_parity(D, A, trunk, B=75):
    """B = 75 under the yardstick (the twin's error is the maximum over the batch's rows, as test_gpu_policy.py takes it: one row's
    error alone can be anything down to 0).  B = 1 and B = 17 are the first rows of the same batch and give the same bits: a row
    depends on itself alone."""
    pol, twin32 = policy_for(D, A, trunk)
    _, twin64 = twins(D, A, trunk)
    batch = batch_for(D, A, trunk, B)
    mb = samples(batch)
    value, log_prob, entropy = (x.cpu().numpy() for x in pol.evaluate_actions(mb.observations, mb.actions))
    with torch.no_grad():
        t = lambda tw, x: torch.as_tensor(np.asarray(x)).to(tw.log_std.dtype)
        r64 = [x.numpy() for x in twin64.evaluate_actions({k: t(twin64, v) for k, v in batch["obs"].items()}, t(twin64, batch["actions"]))]
        r32 = [x.numpy() for x in twin32.evaluate_actions({k: t(twin32, v) for k, v in batch["obs"].items()}, t(twin32, batch["actions"]))]
    assert value.shape == log_prob.shape == entropy.shape == (B,)
    assert_yardstick({"value": value, "log_prob": log_prob}, {"value": r32[0], "log_prob": r32[1]}, {"value": r64[0], "log_prob": r64[1]},
                     f"evaluate D={D} A={A} {trunk} B={B}")
    assert (np.abs(entropy.astype(np.float64) - r64[2]) <= 2 * ulps32(r64[2])).all()
    only = {"entropy": torch.empty(B, device="cuda")}
    pol.evaluate_actions(mb.observations, mb.actions, out=only)
    assert np.array_equal(bits(only["entropy"].cpu().numpy()), bits(entropy))
    for rows in (r for r in (1, 17) if r <= B):
        part = pol.evaluate_actions({k: v[:rows] for k, v in mb.observations.items()}, mb.actions[:rows])
        for x, whole in zip(part, (value, log_prob, entropy)):
            assert tuple(x.shape) == (rows,) and np.array_equal(bits(x.cpu().numpy()), bits(whole[:rows]))


@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 8, "48x32-relu-vf16"), (25, 4, "256x256-relu")])
def test_evaluate_agrees_with_the_forwards_log_prob(built, D, A, trunk):
    """Observations and actions of a pol(obs) call, evaluated with the same weights: the ratio of the first epoch is 1 up to rounding."""
    pol, twin32 = policy_for(D, A, trunk)
    _, twin64 = twins(D, A, trunk)
    obs = ip.round32(ip.random_obs(40, D, seed=5))
    action, value, logp = pol(dev(obs))
    obs32 = {k: torch.from_numpy(v.astype(np.float32)).cuda() for k, v in obs.items()}
    v2, lp2, _ = pol.evaluate_actions(obs32, action)
    with torch.no_grad():
        a = action.cpu()
        lp64 = twin64.evaluate_actions({k: torch.from_numpy(v) for k, v in obs.items()}, a.double())[1].numpy()
        lp32 = twin32.evaluate_actions({k: torch.from_numpy(v).float() for k, v in obs.items()}, a)[1].numpy()
    bound = 10.0 * max(rel(lp32, lp64), FLOOR) * np.abs(lp64).max()
    gap = np.abs(lp2.cpu().numpy().astype(np.float64) - logp.cpu().numpy()).max()
    print(f"evaluate vs forward log_prob: gap {gap:.3e}, bound {bound:.3e}")
    assert gap <= bound
    assert np.array_equal(bits(v2.cpu().numpy()), bits(value.cpu().numpy()))       # the same products in the same order


# ------------------------------------------------------------------------------------------------------- 2. gradient
@pytest.mark.parametrize("D,A,trunk,B,variant", GRAD_CASES)
def test_gradient_parity(built, D, A, trunk, B, variant):
    check_gradient_parity(D, A, trunk, B, variant)


def check_gradient_parity(D, A, trunk, B, variant):
    g64, s64, g32, s32 = reference(D, A, trunk, B, variant)
    pol, opt = updater(D, A, trunk, variant)
    got = host(opt.grad(samples(batch_for(D, A, trunk, B))))
    stats = opt.stats.cpu().numpy()
    assert set(got) == set(g64) and all(np.isfinite(v).all() for v in got.values()) and np.isfinite(stats).all()
    what = f"D={D} A={A} {trunk} B={B} {variant}"
    assert_yardstick(got, g32, g64, "grad " + what)
    assert_yardstick({k: stats[j] for j, k in enumerate(pp.STATS)}, s32, s64, "stats " + what)
    assert round(float(stats[5]) * B) == round(s64["clip_fraction"] * B)          # the same samples are clipped
    assert stats[6] == 0.0 and stats[7] == 0.0
    return pol, opt


# ------------------------------------------------------------------------------------------------ 3. clipped samples
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 4, "256x256-relu")])
def test_clipped_samples_contribute_nothing(built, D, A, trunk):
    batch = dict(batch_for(D, A, trunk, 75))
    pol, opt = updater(D, A, trunk, "ppo", ent_coef=0.01)
    mb = samples(batch)
    lp = pol.evaluate_actions(mb.observations, mb.actions)[1]
    ones = opt.grad(mb._replace(old_log_prob=lp.clone()))                        # every ratio is 1
    ones = host(ones)
    ratio = torch.where(mb.advantages > 0, torch.full_like(lp, 1.5), torch.full_like(lp, 0.6))
    got = host(opt.grad(mb._replace(old_log_prob=lp - torch.log(ratio))))
    assert round(opt.stats[5].item() * 75) == 75               # every sample is clipped
    for k, v in got.items():
        if k.startswith("mlp_extractor.policy_net") or k.startswith("action_net"):
            assert not bits(v).any(), k                          # +0.0 everywhere
            assert np.abs(ones[k]).max() > 0, k
        elif k == "log_std":
            want = np.full(A, -0.01, np.float32)
            assert (np.abs(v.astype(np.float64) - want) <= ulps32(want)).all()
        else:
            assert np.array_equal(bits(v), bits(ones[k])), k


# --------------------------------------------------------------------------------------------- 4. layout and padding
def padding_mask(pol):
    """True at the blob's padding positions: where pack() puts a zero whatever the weights."""
    from mycobotgym_amd.policy import pack
    ones = {k: torch.ones_like(v) for k, v in pol.state_dict().items() if torch.is_tensor(v)}
    return (pack(ones, pol.obs_dim, pol.act_dim, pol.pi, pol.vf, device="cuda") == 0).cpu().numpy()


@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 8, "48x32-relu-vf16"), (25, 4, "256x256-relu")])
def test_layout_and_padding(built, D, A, trunk):
    from mycobotgym_amd.policy import pack, unpack
    pol, opt = updater(D, A, trunk, "ppo-norm-ent")
    pad = padding_mask(pol)
    assert pad.any() and not pad.all()
    for s in range(3):
        opt.step(samples(batch_for(D, A, trunk, 75, seed=5 + s)))
    for name, t in (("grad", opt.grad_blob), ("m", opt.m), ("v", opt.v), ("blob", pol._blob)):
        x = t.cpu().numpy()
        assert not bits(x[pad]).any(), name                      # +0.0 bit for bit
        assert (x[~pad] != 0).mean() > 0.5, name
    shape = (pol.obs_dim, pol.act_dim, pol.pi, pol.vf)
    assert torch.equal(pack(unpack(pol._blob, *shape), *shape, device="cuda").view(torch.int32), pol._blob.view(torch.int32))
    mb = samples(batch_for(D, A, trunk, 75))
    named = opt.grad(mb)
    for k, v in unpack(opt.grad_blob, *shape).items():
        assert torch.equal(v.view(torch.int32), named[k].view(torch.int32)), k


# ----------------------------------------------------------------------------------------------------- 5. determinism
@pytest.mark.parametrize("D,A,trunk,B", [(10, 7, "64x64-tanh", 75), (25, 4, "256x256-relu", 75), (25, 8, "48x32-relu-vf16", 600)])
def test_determinism_and_ragged_filler(built, D, A, trunk, B):
    check_determinism_and_ragged_filler(D, A, trunk, B)


def check_determinism_and_ragged_filler(D, A, trunk, B):
    batch = batch_for(D, A, trunk, B)
    runs = []
    for fill in (0.0, 0.0, float("nan")):
        pol, opt = updater(D, A, trunk, "ppo-norm-ent")
        opt.step(samples(batch, rows=B + 5, fill=fill))
        runs.append([x.cpu().numpy().copy() for x in (opt.grad_blob, opt.stats, pol._blob, opt.grad_norm)])
    assert np.isfinite(runs[0][0]).all()
    for other in runs[1:]:
        for x, y in zip(runs[0], other):
            assert np.array_equal(bits(x), bits(y))


# ------------------------------------------------------------------------------------------------ 6. Adam and clipping
@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 8, "48x32-relu-vf16"), (25, 4, "256x256-relu")])
@pytest.mark.parametrize("max_norm", [0.5, 1e-3, 0.0])
def test_adam_step_on_the_kernels_gradient(built, D, A, trunk, max_norm):
    twin32, _ = twins(D, A, trunk)
    pol, opt = updater(D, A, trunk, "ppo-norm-ent", max_grad_norm=max_norm)
    grad = host(opt.grad(samples(batch_for(D, A, trunk, 75))))
    before = host(pol.state_dict())
    opt.apply()
    after, m = host(pol.state_dict()), host(opt.state_dict()["exp_avg"])
    norm64 = pp.global_norm(grad)
    coef = pp.clip_coef(norm64, max_norm)
    assert coef < 0.1 if max_norm == 1e-3 else coef == 1.0 if max_norm == 0.0 else coef <= 1.0
    ref = {k: pp.adam_step(before[k], coef * grad[k].astype(np.float64), 0.0, 0.0, 1)[0] for k in grad}
    params = dict(twin32.named_parameters())
    for k, p in params.items():
        p.grad = torch.from_numpy(grad[k].copy())
    norm32 = float(torch.nn.utils.clip_grad_norm_(list(params.values()), max_norm)) if max_norm > 0 else \
        float(torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in params.values()])))
    torch.optim.Adam(list(params.values()), lr=3e-4, betas=(0.9, 0.999), eps=1e-5).step()
    assert_yardstick(after, {k: p.detach().numpy() for k, p in params.items()}, ref, f"adam D={D} A={A} {trunk} max_norm={max_norm}")
    kn = float(opt.grad_norm.item())
    print(f"norm: kernel {kn!r}, float64 {norm64!r}, twin {norm32!r}")
    assert abs(kn - norm64) <= 10.0 * max(abs(norm32 - norm64), FLOOR * norm64)
    for k in grad:                                               # the first moment is (1 - beta1) coef g: the update shrank by coef
        want = 0.1 * coef * grad[k].astype(np.float64)
        assert np.abs(m[k] - want).max() <= 8 * FLOOR * np.abs(want).max(), k
        assert (after[k] != before[k]).any(), k


@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-tanh"), (25, 4, "256x256-relu")])
def test_five_steps_against_the_twin(built, D, A, trunk):
    check_five_steps_against_the_twin(D, A, trunk)


def check_five_steps_against_the_twin(D, A, trunk, B=75):
    twin32, twin64 = twins(D, A, trunk)
    pol, opt = updater(D, A, trunk, "ppo-norm-ent")
    opt32 = torch.optim.Adam(twin32.parameters(), lr=3e-4, betas=(0.9, 0.999), eps=1e-5)
    state64 = {}
    for s in range(5):
        batch = batch_for(D, A, trunk, B, seed=5 + s)
        opt.step(samples(batch))
        pp.twin_update(twin64, state64, batch, s + 1, **VARIANTS["ppo-norm-ent"])
        opt32.zero_grad()
        pp.loss_terms(twin32, batch, **VARIANTS["ppo-norm-ent"])["loss"].backward()
        torch.nn.utils.clip_grad_norm_(twin32.parameters(), 0.5)
        opt32.step()
    assert opt.steps == 5
    assert_yardstick(host(pol.state_dict()), twin32.numpy_state(), {k: v for k, v in twin64.numpy_state().items()},
                     f"five steps {trunk}" + ("" if (D, A, B) in ((10, 7, 75), (25, 4, 75)) else f" D={D} A={A} B={B}"))
    # the forward sees the new weights at once: equal to a fresh policy loaded with them
    from mycobotgym_amd import ActorCritic
    pi, vf, act = ip.TRUNKS[trunk]
    fresh = ActorCritic(num_envs=40, obs_dim=D, act_dim=A, hidden=dict(pi=pi, vf=vf), activation=act)
    fresh.load_state_dict(pol.state_dict())
    obs = dev(ip.random_obs(40, D, seed=5))
    for x, y in zip(pol(obs, deterministic=True), fresh(obs, deterministic=True)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    return pol, opt


# --------------------------------------------------------------------------------------------------- 7. stray writes
def guarded(n, G=4):
    big = torch.full((n + 2 * G,), -77.25, device="cuda")
    return big, big[G:G + n]


@pytest.mark.parametrize("B", [75, 1])
def test_no_stray_writes(built, B):
    D, A, trunk = 25, 7, "64x64-tanh"
    pol, opt = updater(D, A, trunk, "ppo-norm-ent")
    mb = samples(batch_for(D, A, trunk, B))
    need = int(pol._lib.mcg_policy_grad_work_floats(C.byref(pol._cbuf), C.c_int64(B)))
    assert need > 0
    big = {}
    for name, n in (("grad_blob", pol.blob_floats), ("m", pol.blob_floats), ("v", pol.blob_floats), ("stats", 8), ("grad_norm", 4), ("_work", need)):
        big[name], view = guarded(n)
        if name in ("m", "v"):
            view.zero_()
        setattr(opt, name, view)
    outs = {}
    for name in ("value", "log_prob", "entropy"):
        big[name], outs[name] = guarded(B)
    pol.evaluate_actions(mb.observations, mb.actions, out=outs)
    opt.step(mb)
    torch.cuda.synchronize()
    assert opt._work.numel() == need                             # not replaced: exactly the size the C side asked for
    for name, t in big.items():
        x = t.cpu().numpy()
        assert (x[:4] == -77.25).all() and (x[-4:] == -77.25).all(), name
    assert (big["grad_norm"].cpu().numpy()[5:] == -77.25).all()
    plain_pol, plain = updater(D, A, trunk, "ppo-norm-ent")
    plain.step(mb)
    assert torch.equal(plain.grad_blob.view(torch.int32), opt.grad_blob.view(torch.int32))
    assert torch.equal(plain_pol._blob.view(torch.int32), pol._blob.view(torch.int32))
    # work of one float fewer is refused
    from mycobotgym_amd import _abi
    batch, _, _keep = pol._minibatch(mb.observations, mb.actions, "test", advantage=mb.advantages, returns=mb.returns, old_log_prob=mb.old_log_prob)
    hyper = _abi.McgPolicyHyper(loss_kind=0, normalize_advantage=1, clip_range=0.2, ent_coef=0.0, vf_coef=0.5)
    with pytest.raises(_abi.McgError, match="work_floats"):
        pol._call("mcg_policy_grad", C.byref(batch), C.c_int64(B), C.byref(hyper), C.c_void_p(opt._work.data_ptr()), C.c_int64(need - 1),
                  C.c_void_p(opt.grad_blob.data_ptr()), C.c_void_p(opt.stats.data_ptr()))


# ------------------------------------------------------------------------------------------------- 8. C-side refusals
def test_c_side_refusals(built):
    from mycobotgym_amd import _abi
    D, A, trunk, B = 10, 7, "64x64-tanh", 20
    pol, opt = updater(D, A, trunk)
    mb = samples(batch_for(D, A, trunk, B))
    batch, _, _keep = pol._minibatch(mb.observations, mb.actions, "test", advantage=mb.advantages, returns=mb.returns, old_log_prob=mb.old_log_prob)
    work = opt._work_for(B)
    p = lambda t, off=0: C.c_void_p(t.data_ptr() + off)
    def hyper(**kw):
        return _abi.McgPolicyHyper(**dict(dict(loss_kind=0, normalize_advantage=1, clip_range=0.2, ent_coef=0.0, vf_coef=0.5), **kw))
    def grad(pol_struct=None, batch=batch, B=B, hyper=hyper(), work=p(work), grad=p(opt.grad_blob), stats=p(opt.stats)):
        h = C.byref(hyper) if hyper is not None else None
        b = C.byref(batch) if batch is not None else None
        _abi.check(pol._lib.mcg_policy_grad(C.byref(pol_struct or pol._cbuf), b, C.c_int64(B), h, work, C.c_int64(opt._work.numel()), grad, stats,
                                            pol._stream()), "mcg_policy_grad")
    def adam(grad=p(opt.grad_blob), m=p(opt.m), v=p(opt.v), step=1, norm=p(opt.grad_norm)):
        _abi.check(pol._lib.mcg_policy_adam(C.byref(pol._cbuf), grad, m, v, C.c_int64(step), 3e-4, 0.9, 0.999, 1e-5, 0.5, norm, pol._stream()),
                   "mcg_policy_adam")
    def evaluate(batch=batch, B=B, out=None):
        o = _abi.McgPolicyEvalOut(**(out or {}))
        _abi.check(pol._lib.mcg_policy_evaluate(C.byref(pol._cbuf), C.byref(batch) if batch is not None else None, C.c_int64(B), C.byref(o),
                                                pol._stream()), "mcg_policy_evaluate")
    grad()                                                        # the arguments are good as they stand
    adam()
    no_adv = _abi.McgRolloutBatch(obs=batch.obs, achieved=batch.achieved, desired=batch.desired, action=batch.action, returns=batch.returns,
                                  old_log_prob=batch.old_log_prob)
    no_obs = _abi.McgRolloutBatch(achieved=batch.achieved, desired=batch.desired, action=batch.action)
    stale = _abi.McgPolicy.from_buffer_copy(pol._cbuf)
    stale.blob_floats += 16
    for call, match in ((lambda: grad(batch=None), "null mcg_rollout_batch"), (lambda: grad(batch=no_obs), "obs, achieved, desired and action"),
                        (lambda: grad(batch=no_adv), "advantage and returns"), (lambda: grad(B=0), "B must be >= 1"),
                        (lambda: grad(hyper=None), "null mcg_policy_hyper"), (lambda: grad(hyper=hyper(loss_kind=2)), "loss_kind must be"),
                        (lambda: grad(hyper=hyper(clip_range=0.0)), "clip_range must be > 0"),
                        (lambda: grad(hyper=hyper(clip_range=-0.2)), "clip_range must be > 0"),
                        (lambda: grad(work=None), "work is null"), (lambda: grad(grad=None), "grad is null"), (lambda: grad(stats=None), "stats is null"),
                        (lambda: grad(grad=p(opt.grad_blob, 4)), "grad is not 16-byte aligned"), (lambda: grad(pol_struct=stale), "blob_floats is"),
                        (lambda: adam(step=0), "step must be >= 1"), (lambda: adam(grad=None), "grad is null"), (lambda: adam(m=None), "m is null"),
                        (lambda: adam(v=None), "v is null"), (lambda: adam(norm=None), "norm_out is null"),
                        (lambda: adam(grad=p(opt.grad_blob, 4)), "grad is not 16-byte aligned"), (lambda: adam(m=p(opt.m, 8)), "m is not 16-byte aligned"),
                        (lambda: adam(v=p(opt.v, 4)), "v is not 16-byte aligned"),
                        (lambda: evaluate(out={}), "all outputs are null"), (lambda: evaluate(B=0, out=dict(value=opt.stats.data_ptr())), "B must be >= 1"),
                        (lambda: evaluate(batch=None, out=dict(value=opt.stats.data_ptr())), "null mcg_rollout_batch")):
        with pytest.raises(_abi.McgError, match=match):
            call()
    grad(hyper=hyper(loss_kind=1, clip_range=0.0))                # A2C does not read clip_range
    assert int(pol._lib.mcg_policy_grad_work_floats(C.byref(pol._cbuf), C.c_int64(0))) == 0
    torch.cuda.synchronize()


# ---------------------------------------------------------------------------------------------------- 9. on the engine
def test_on_the_engine(built):
    from mycobotgym_amd import ActorCritic, PPOUpdate, RolloutBuffer, make
    n, T = 64, 8
    envs = make("MyCobotReach-Dense-joint-v0", num_envs=n)
    pol = ActorCritic(envs, hidden=(64, 64), seed=21)
    opt = PPOUpdate(pol)
    buf = RolloutBuffer(envs, n_steps=T, seed=0)
    obs, _ = envs.reset(seed=0)
    buf.start(obs)
    for _ in range(T):
        a, v, logp = pol(obs)
        obs, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, obs, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
    buf.finish(last_values=pol.values(obs))
    blob0 = pol._blob.clone()

    def epoch(pol, opt, buf):
        out = []
        for mb in buf.get(100):
            opt.step(mb)
            out.append((len(mb.actions), opt.stats.clone(), opt.grad_norm.clone()))
        return out

    first = epoch(pol, opt, buf)
    assert [b for b, _, _ in first] == [100] * 5 + [12]           # the last minibatch is short: B changes
    assert all(torch.isfinite(s).all() and torch.isfinite(g).all() for _, s, g in first)
    assert float(first[0][1][4]) < 1e-5 and float(first[0][1][5]) == 0.0          # the first minibatch: ratio = 1 up to rounding
    assert not torch.equal(pol._blob, blob0)
    saved = pol.state_dict(), opt.state_dict(), buf.state_dict()
    pol2 = ActorCritic(envs, hidden=(64, 64), seed=999)
    opt2 = PPOUpdate(pol2, learning_rate=1.0, loss="a2c")
    buf2 = RolloutBuffer(envs, n_steps=T, seed=5)
    pol2.load_state_dict(saved[0]); opt2.load_state_dict(saved[1]); buf2.load_state_dict(saved[2])
    assert (opt2.steps, opt2.loss, opt2.learning_rate) == (6, "ppo", 3e-4)
    second, again = epoch(pol, opt, buf), epoch(pol2, opt2, buf2)
    for (_, s, g), (_, s2, g2) in zip(second, again):
        assert torch.equal(s.view(torch.int32), s2.view(torch.int32)) and torch.equal(g.view(torch.int32), g2.view(torch.int32))
    for x, y in ((pol._blob, pol2._blob), (opt.m, opt2.m), (opt.v, opt2.v), (opt.grad_blob, opt2.grad_blob)):
        assert torch.equal(x.view(torch.int32), y.view(torch.int32))
    envs.close()


def test_python_side_refusals_on_the_device(built):
    D, A, trunk = 10, 7, "64x64-tanh"
    pol, opt = updater(D, A, trunk)
    mb = samples(batch_for(D, A, trunk, 20))
    with pytest.raises(ValueError, match="picture buffers"):
        opt.step(mb._replace(observations=torch.zeros(20, 3, 8, 8, dtype=torch.uint8, device="cuda")))
    with pytest.raises(ValueError, match="lives on"):
        opt.step(mb._replace(actions=mb.actions.cpu()))
    with pytest.raises(ValueError, match="expected float32"):
        pol.evaluate_actions({k: v.double() for k, v in mb.observations.items()}, mb.actions)
    opt.step(mb)
    opt.learning_rate, opt.clip_range = 1e-4, 0.1                 # settable between steps
    opt.step(mb)
    assert opt.steps == 2 and torch.isfinite(opt.stats).all()
