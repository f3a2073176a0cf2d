"""SAC's update without a GPU: the restated rule against autograd, the batch maker's conditions, the noise domain, Adam's restatement,
the structs' layout, and every host-side refusal of the new C entries and of ``SACUpdate`` (none of which dereferences a pointer)."""
import ctypes as C
import math
import os
import subprocess
from types import SimpleNamespace

import numpy as np
import pytest
import torch

from mycobotgym_amd import sac_update as upd
from tests import indep_sac as isac
from tests import indep_sac_update as su

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOG_ALPHA = float(np.float32(math.log(0.3)))


@pytest.mark.parametrize("D,A,trunk", [(10, 7, "64x64-relu"), (25, 8, "48x32-tanh-qf16"), (25, 4, "16-tanh")])
def test_head_derivative_is_autograds(D, A, trunk):
    """The formulas of include/mcg.h in numpy float64 against autograd through the float64 twin's squash, log-prob and critics: the
    derivative of the actor loss with respect to the two heads' outputs, to 1e-10 of each one's scale; the clamp's zero included."""
    B = 75
    _, t64, batch, _, eps_a, census = su.case(D, A, trunk, B)
    assert census["lower_clamp_rows"] > 0 and census["upper_clamp_rows"] > 0
    alpha = math.exp(LOG_ALPHA)
    obs = {k: torch.from_numpy(v).double() for k, v in batch.observations.items()}
    h = t64.actor.latent_pi(t64._features(obs))
    mu, raw = t64.actor.mu(h).detach().requires_grad_(True), t64.actor.log_std(h).detach().requires_grad_(True)
    eps = torch.from_numpy(eps_a).double()
    log_std = torch.clamp(raw, isac.LOG_STD_MIN, isac.LOG_STD_MAX)
    a = torch.tanh(mu + log_std.exp() * eps)
    logp = (-0.5 * eps ** 2 - log_std - isac.LOG_SQRT_2PI).sum(-1) - torch.log(1.0 - a ** 2 + isac.EPSILON).sum(-1)
    loss = (alpha * logp - torch.min(t64.q(obs, a), dim=0).values).mean()
    dmu, draw = torch.autograd.grad(loss, [mu, raw])
    a2 = a.detach().clone().requires_grad_(True)
    dq_da = torch.autograd.grad(torch.min(t64.q(obs, a2), dim=0).values.sum(), a2)[0]
    got_mu, got_raw = su.head_derivative(a.detach().numpy(), raw.detach().numpy(), eps_a, alpha, dq_da.numpy(), B)
    for got, want in ((got_mu, dmu.numpy()), (got_raw, draw.numpy())):
        assert np.abs(got - want).max() <= 1e-10 * np.abs(want).max()
    clamped = (raw.detach().numpy() < isac.LOG_STD_MIN) | (raw.detach().numpy() > isac.LOG_STD_MAX)
    assert clamped.any() and (got_raw[clamped] == 0.0).all() and (draw.numpy()[clamped] == 0.0).all() and (got_raw[~clamped] != 0.0).all()


@pytest.mark.parametrize("D,A,trunk,B", su.GRAD_CASES)
def test_the_maker_meets_its_conditions(D, A, trunk, B):
    """For every case the GPU tests use: all B rows pass every condition in the float64 rule (none is left out), the next observations
    pass indep_sac's under the target's noise, both clamps act (B >= 75), and each critic is the smaller one in at least 8 of the first
    75 rows."""
    t32, t64, batch, eps_t, eps_a, census = su.case(D, A, trunk, B)
    print(census)
    assert all(len(v) == B for v in batch.observations.values()) and len(batch.actions) == B
    ok, second = su.row_conditions(t64, batch.observations, batch.actions, eps_a)
    assert set(ok) == {"squash_and_clamp_margin", "q_gap"} | ({"relu_margin"} if t64.activation == "relu" else set())
    assert all(v.shape == (B,) and v.all() for v in ok.values())
    assert isac.conditions(t64.numpy_state(), batch.next_observations, eps_t, t64.activation).all()
    assert all(v.dtype == np.float32 for v in batch.observations.values()) and batch.actions.dtype == np.float32
    assert np.array_equal(batch.observations["desired_goal"], batch.next_observations["desired_goal"])
    if B >= su.FIRST_ROWS:
        n1 = int(second[:su.FIRST_ROWS].sum())
        assert su.MIN_EACH <= n1 <= su.FIRST_ROWS - su.MIN_EACH
        assert census["lower_clamp_rows"] > 0 and census["upper_clamp_rows"] > 0
    assert all(torch.equal(v, t64.state_dict()[k].float()) and torch.equal(v.double(), t64.state_dict()[k]) for k, v in t32.state_dict().items())


def test_domain_9_shares_no_block_with_domains_0_to_8():
    from tests import indep_policy as ip
    assert su.DOMAIN_ACTOR_LOSS == 9 and {isac.DOMAIN_ACT, isac.DOMAIN_TARGET, ip.DOMAIN} == {6, 7, 8}
    N, A, calls, seed = 40, 8, 16, 0
    mine = {tuple(isac.block(su.DOMAIN_ACTOR_LOSS, seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
    assert len(mine) == N * calls * (A // 2)
    for dom in range(9):
        theirs = {tuple(isac.block(dom, seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
        assert not mine & theirs, dom
    assert not mine & {tuple(ip.block(seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
    assert isac.counter(9, 2 ** 32 + 5, 2 ** 32 * 7 + 9, 3) == [5, 9, 3 ^ (7 << 8), 9 ^ (1 << 8)]
    assert not np.array_equal(isac.noise(9, seed, 3, 40, 8), isac.noise(8, seed, 3, 40, 8))


def test_adam_restatement_is_torchs():
    rng = np.random.default_rng(3)
    p0 = rng.normal(size=(5, 7))
    p = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([p], lr=3e-4, betas=(0.9, 0.999), eps=1e-8)
    mine, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in range(1, 6):
        g = rng.normal(size=p0.shape) * 10.0 ** rng.integers(-9, 1, size=p0.shape)
        p.grad = torch.from_numpy(g.copy())
        opt.step()
        mine, m, v = su.adam_step(mine, g, m, v, step)
        assert np.abs(mine - p.detach().numpy()).max() <= 1e-15, step
    assert np.abs(mine - p0).max() > 1e-4


def test_structs_match_the_header_and_the_entries_are_exported(built, tmp_path):
    from mycobotgym_amd import _abi
    cls = _abi.McgSacActorGradOut
    exprs = ["MCG_ABI_VERSION", "sizeof(mcg_sac_actor_grad_out)"] + [f"offsetof(mcg_sac_actor_grad_out,{n})" for n, _ in cls._fields_]
    want = [8, C.sizeof(cls)] + [getattr(cls, n).offset for n, _ in cls._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    L = _abi.load()
    assert _abi.ABI_VERSION == 8 and L.mcg_abi_version() == 8          # additive: the version stays
    for name in ("mcg_sac_grad_work_floats", "mcg_sac_critic_grad", "mcg_sac_actor_grad", "mcg_sac_alpha_step", "mcg_sac_adam"):
        assert name in _abi.EXPORTS and hasattr(L, name)
    import mycobotgym_amd
    assert mycobotgym_amd.SACUpdate is upd.SACUpdate


def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0] * 3)[:3])


def _sac(_abi, L, **over):
    p = C.c_void_p(0x1000)
    kw = dict(actor=p, critic=p, critic_target=C.c_void_p(0x2000), n_envs=40, obs_dim=25, act_dim=7, n_pi=2, pi_width=_arr((64, 64)), n_qf=2,
              qf_width=_arr((64, 64)), activation=_abi.POLICY_RELU)
    kw.update(over)
    fa, fc = C.c_int64(0), C.c_int64(0)
    L.mcg_sac_blob_floats(kw["obs_dim"], kw["act_dim"], kw["n_pi"], kw["pi_width"], kw["n_qf"], kw["qf_width"], C.byref(fa), C.byref(fc))
    kw.setdefault("actor_floats", fa.value)
    kw.setdefault("critic_floats", fc.value)
    return _abi.McgSac(**kw)


def test_c_side_refusals_without_a_gpu(built):
    """Every argument check of the new entries: the code and a fragment of the message that names the field (the refusals come before
    any HIP call, so the pointers are never dereferenced)."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p, odd, B = 0x1000, 0x1004, 75
    ref = lambda x: None if x is None else C.byref(x)
    good = _sac(_abi, L)
    rows = _abi.McgSacRows(obs=p, achieved=p, desired=p, action=p)
    need = L.mcg_sac_grad_work_floats(C.byref(good), B)
    assert need > 0 and L.mcg_sac_grad_work_floats(C.byref(good), 600) > need
    assert L.mcg_sac_grad_work_floats(None, B) == 0 and L.mcg_sac_grad_work_floats(C.byref(good), 0) == 0
    assert L.mcg_sac_grad_work_floats(C.byref(good), 2 ** 27) == 0 and L.mcg_sac_grad_work_floats(C.byref(_sac(_abi, L, act_dim=17)), B) == 0

    def critic(s=good, r=rows, y=p, B=B, work=p, wf=need, grad=p, stats=p):
        return L.mcg_sac_critic_grad(ref(s), ref(r), y, B, work, wf, grad, stats, None)

    def actor(s=good, r=rows, B=B, ent=0.2, lec=p, work=p, wf=need, grad=p, logp=p, stats=p):
        return L.mcg_sac_actor_grad(ref(s), ref(r), B, 0, 0, ent, lec, work, wf, grad, logp, stats, None, None)

    def alpha(lec=p, logp=p, B=B, te=-7.0, m=p, v=p, step=1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8):
        return L.mcg_sac_alpha_step(lec, logp, B, te, m, v, step, lr, b1, b2, eps, None, None, None)

    def adam(blob=p, grad=p, m=p, v=p, floats=1024, step=1, lr=3e-4, b1=0.9, b2=0.999, eps=1e-8):
        return L.mcg_sac_adam(blob, grad, m, v, floats, step, lr, b1, b2, eps, None)

    no_action = _abi.McgSacRows(obs=p, achieved=p, desired=p)
    cases = [
        (lambda: critic(s=None), "null mcg_sac"), (lambda: critic(s=_sac(_abi, L, critic=None)), "critic is null"),
        (lambda: critic(s=_sac(_abi, L, critic=C.c_void_p(odd))), "not 16-byte aligned"), (lambda: critic(s=_sac(_abi, L, n_qf=4)), "n_qf"),
        (lambda: critic(s=_sac(_abi, L, qf_width=_arr((64, 300)))), "qf_width[1]"), (lambda: critic(s=_sac(_abi, L, activation=5)), "activation"),
        (lambda: critic(s=_sac(_abi, L, critic_floats=64)), "critic_floats"), (lambda: critic(B=0), "B must be >= 1"),
        (lambda: critic(B=2 ** 27), "below 2^27"), (lambda: critic(r=None), "null mcg_sac_rows"), (lambda: critic(r=no_action), "action"),
        (lambda: critic(y=None), "y is null"), (lambda: critic(stats=None), "stats is null"), (lambda: critic(grad=None), "grad is null"),
        (lambda: critic(grad=odd), "grad is not 16-byte aligned"), (lambda: critic(work=None), "work is null"),
        (lambda: critic(work=odd), "work is not 16-byte aligned"), (lambda: critic(wf=need // 8), "work_floats"),
        (lambda: actor(s=None), "null mcg_sac"), (lambda: actor(s=_sac(_abi, L, actor=None)), "actor is null"),
        (lambda: actor(s=_sac(_abi, L, critic=None)), "critic is null"), (lambda: actor(s=_sac(_abi, L, act_dim=17)), "act_dim"),
        (lambda: actor(B=0), "B must be >= 1"), (lambda: actor(B=2 ** 27), "below 2^27"), (lambda: actor(r=None), "null mcg_sac_rows"),
        (lambda: actor(r=_abi.McgSacRows(obs=p, achieved=p)), "desired"), (lambda: actor(lec=None, ent=-0.1), "ent_coef"),
        (lambda: actor(lec=None, ent=float("inf")), "ent_coef"), (lambda: actor(lec=None, ent=float("nan")), "ent_coef"),
        (lambda: actor(logp=None), "logp_out is null"), (lambda: actor(stats=None), "stats is null"), (lambda: actor(grad=None), "grad is null"),
        (lambda: actor(grad=odd), "grad is not 16-byte aligned"), (lambda: actor(work=None), "work is null"), (lambda: actor(work=odd), "work is not"),
        (lambda: actor(wf=16), "work_floats"),
        (lambda: alpha(lec=None), "log_ent_coef is null"), (lambda: alpha(logp=None), "logp is null"), (lambda: alpha(B=0), "B must be >= 1"),
        (lambda: alpha(B=2 ** 27), "below 2^27"), (lambda: alpha(te=float("nan")), "target_entropy"), (lambda: alpha(step=0), "step must be >= 1"),
        (lambda: alpha(lr=-1.0), "lr"), (lambda: alpha(lr=float("inf")), "lr"), (lambda: alpha(b1=1.0), "beta1"), (lambda: alpha(b2=-0.1), "beta1"),
        (lambda: alpha(eps=-1e-8), "eps"), (lambda: alpha(m=None), "m and v"), (lambda: alpha(v=None), "m and v"),
        (lambda: adam(blob=None), "blob is null"), (lambda: adam(blob=odd), "blob is not 16-byte aligned"), (lambda: adam(grad=None), "grad is null"),
        (lambda: adam(grad=odd), "grad is not"), (lambda: adam(m=None), "m is null"), (lambda: adam(m=odd), "m is not"), (lambda: adam(v=None), "v is null"),
        (lambda: adam(v=odd), "v is not"), (lambda: adam(floats=0), "floats"), (lambda: adam(floats=2 ** 31), "floats"),
        (lambda: adam(step=0), "step must be >= 1"), (lambda: adam(lr=float("nan")), "lr"), (lambda: adam(lr=-3e-4), "lr"),
        (lambda: adam(b1=1.5), "beta1"), (lambda: adam(b2=1.0), "beta2"), (lambda: adam(eps=float("inf")), "eps"),
    ]
    for call, fragment in cases:
        assert call() == _abi.MCG_ERR_ARG, fragment
        assert fragment.encode() in L.mcg_last_error(), (fragment, L.mcg_last_error())


def _batch(B=8, D=10, A=7, **over):
    f = lambda *s: torch.zeros(*s)
    obs = lambda: {"observation": f(B, D), "achieved_goal": f(B, 3), "desired_goal": f(B, 3)}
    kw = dict(observations=obs(), actions=f(B, A), next_observations=obs(), dones=f(B, 1), rewards=f(B, 1))
    kw.update(over)
    return SimpleNamespace(**kw)


def test_python_side_refusals_need_no_gpu():
    ok = dict(learning_rate=3e-4, gamma=0.99, tau=0.005, ent_coef="auto", target_entropy="auto", target_update_interval=1, betas=(0.9, 0.999),
              eps=1e-8, unbuilt={})
    assert upd.check_hyper(**ok) == (True, None, None)
    assert upd.check_hyper(**dict(ok, ent_coef=0.2)) == (False, 0.2, None) and upd.check_hyper(**dict(ok, ent_coef="auto_0.1")) == (True, None, 0.1)
    assert upd.check_hyper(**dict(ok, ent_coef=0.0, tau=1.0, target_entropy=-3.5, unbuilt=dict(use_sde=False))) == (False, 0.0, None)
    bad = [(dict(learning_rate=lambda f: 3e-4 * f), "schedule"), (dict(learning_rate=0.0), "learning_rate"), (dict(learning_rate=-1e-3), "learning_rate"),
           (dict(learning_rate=float("nan")), "learning_rate"), (dict(learning_rate="3e-4"), "learning_rate"),
           (dict(tau=0.0), "tau"), (dict(tau=1.5), "tau"), (dict(tau=float("nan")), "tau"), (dict(gamma=1.01), "gamma"), (dict(gamma=-0.1), "gamma"),
           (dict(target_update_interval=0), "target_update_interval"), (dict(target_update_interval=1.5), "target_update_interval"),
           (dict(ent_coef=-0.1), "ent_coef"), (dict(ent_coef=float("inf")), "ent_coef"), (dict(ent_coef=float("nan")), "ent_coef"),
           (dict(ent_coef="automatic"), "ent_coef"), (dict(ent_coef="auto_-1"), "ent_coef"), (dict(ent_coef="auto_x"), "ent_coef"),
           (dict(target_entropy="big"), "target_entropy"), (dict(target_entropy=float("inf")), "target_entropy"),
           (dict(betas=(0.9,)), "betas"), (dict(betas=(0.9, 1.0)), "betas"), (dict(eps=-1.0), "eps"),
           (dict(unbuilt=dict(use_sde=True)), "gSDE"), (dict(unbuilt=dict(sde_sample_freq=4)), "gSDE"), (dict(unbuilt=dict(max_grad_norm=0.5)), "clips no"),
           (dict(unbuilt=dict(n_critics=3)), "n_critics"), (dict(unbuilt=dict(optimizer_class=torch.optim.SGD)), "optimizer_class"),
           (dict(unbuilt=dict(action_noise=object())), "action_noise")]
    for over, fragment in bad:
        with pytest.raises(ValueError, match=fragment):
            upd.check_hyper(**dict(ok, **over))
    with pytest.raises(TypeError, match="train_freq"):
        upd.check_hyper(**dict(ok, unbuilt=dict(train_freq=1)))
    with pytest.raises(ValueError, match="needs an SACPolicy"):
        upd.SACUpdate(object())
    with pytest.raises(ValueError, match="schedule"):
        upd.SACUpdate(object(), learning_rate=lambda f: f)            # (the hyper-parameters are checked first)
    assert upd.check_batch(_batch(), 10, 7) == 8
    pictures = _batch(observations=torch.zeros(8, 3, 84, 84, dtype=torch.uint8), next_observations=torch.zeros(8, 3, 84, 84, dtype=torch.uint8))
    wrong = [(pictures, "picture"), (_batch(actions=torch.zeros(8, 7, dtype=torch.float64)), "expected float32"),
             (_batch(actions=torch.zeros(8, 6)), "expected shape"), (_batch(rewards=torch.zeros(7, 1)), "expected shape"),
             (_batch(dones=torch.zeros(8, dtype=torch.bool)), "expected float32"), (_batch(next_observations=_batch(B=7).observations), "another number"),
             (_batch(B=0), "empty"), (SimpleNamespace(observations={}, actions=None), "no field"),
             (_batch(observations={"observation": torch.zeros(8, 10), "achieved_goal": torch.zeros(8, 3)}), "lacks")]
    for b, fragment in wrong:
        with pytest.raises(ValueError, match=fragment):
            upd.check_batch(b, 10, 7)
    with pytest.raises(ValueError, match="lives on"):
        upd.check_batch(_batch(), 10, 7, device=torch.device("cuda:0"))


def test_checkpoint_round_trip_of_the_host_side_fields():
    """state_dict / load_state_dict on an updater whose policy is a stand-in with CPU blobs: the moments by blob and by SB3's names, the
    step count, the noise's call number and the hyper-parameters come back; a bad moment or hyper-parameter is refused."""
    from mycobotgym_amd import sac_policy as sp
    D, A, pi, qf = 10, 7, (32, 16), (16,)
    twin = isac.Twin(D, A, pi, qf, "tanh")
    sd = twin.state_dict()
    blobs = {"actor": sp.pack_actor(sd, D, A, pi), "critic": sp.pack_critic(sd, D, A, qf), "critic_target": sp.pack_critic(sd, D, A, qf, "critic_target"),
             "log_ent_coef": torch.zeros(1)}
    pol = SimpleNamespace(_t=blobs, obs_dim=D, act_dim=A, pi=pi, qf=qf, device=torch.device("cpu"), actor_floats=blobs["actor"].numel(),
                          critic_floats=blobs["critic"].numel(), log_ent_coef=blobs["log_ent_coef"])
    opt = upd.SACUpdate(pol, learning_rate=1e-3, gamma=0.95, tau=0.01, ent_coef="auto_0.5", target_entropy=-3.0, target_update_interval=3,
                        betas=(0.8, 0.99), eps=1e-7)
    assert abs(pol.log_ent_coef.item() - math.log(0.5)) < 1e-7 and opt.target_entropy == -3.0 and opt.auto
    assert upd.SACUpdate(pol).target_entropy == -float(A)
    for k in opt.m:                      # moments that are valid blobs: packed from random named tensors
        opt.m[k].copy_(blobs[k] * 0.5 if k != "log_ent_coef" else torch.tensor([0.25]))
        opt.v[k].copy_(blobs[k] ** 2 if k != "log_ent_coef" else torch.tensor([0.125]))
    opt.steps, opt.actor_calls = 11, 12
    saved = opt.state_dict()
    assert set(saved["exp_avg"]) == {k for k in sd if not k.startswith("critic_target.")} | {"log_ent_coef"}
    for drop in ((), ("m", "v")):
        again = upd.SACUpdate(pol)
        again.load_state_dict({k: v for k, v in saved.items() if k not in drop})
        assert (again.steps, again.actor_calls, again.learning_rate, again.gamma, again.tau, again.target_update_interval, again.betas, again.eps,
                again.target_entropy, again.auto) == (11, 12, 1e-3, 0.95, 0.01, 3, (0.8, 0.99), 1e-7, -3.0, True)
        assert all(torch.equal(again.m[k], opt.m[k]) and torch.equal(again.v[k], opt.v[k]) for k in opt.m)
    with pytest.raises(ValueError, match="neither"):
        upd.SACUpdate(pol).load_state_dict({k: v for k, v in saved.items() if k not in ("m", "exp_avg")})
    with pytest.raises(ValueError, match="expected float32"):
        upd.SACUpdate(pol).load_state_dict(dict(saved, m=dict(saved["m"], actor=torch.zeros(3))))
    with pytest.raises(ValueError, match="tau"):
        upd.SACUpdate(pol).load_state_dict(dict(saved, tau=0.0))
