"""TD3 / DDPG without a GPU: the restatement's own checks (tests/indep_td3.py), the blobs' pack / unpack, the ABI's structs and exports,
and every refusal of the C entries (which come before any HIP call) and of the Python classes."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import indep_td3 as it

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------------------------------------ the restatement itself
@pytest.mark.parametrize("D,A,trunk,B,nc", it.CASES)
def test_makers_census_holds_for_every_case(D, A, trunk, B, nc):
    """The float64 twin alone meets the census with the tests' sigma, clip and head scale: among the first 75 rows at least 8 where
    the noise clip acts, at least 8 where the +-1 clamp of a' acts, and with two critics each the smaller in at least 8.  Every row is
    kept, and with relu every row has its margins."""
    t32, t64, batch, n, census = it.case(D, A, trunk, B, nc)
    assert len(batch.actions) == B and n.shape == (B, A) and n.dtype == np.float32
    assert all(v.dtype == np.float32 for v in batch.observations.values()) and batch.dones.shape == (B, 1)
    assert np.abs(n).max() <= np.float32(it.CLIP)
    if B >= it.FIRST_ROWS:
        it.assert_census(census)
        again = it.census_of(t64, batch, it.noise(it.DOMAIN_TARGET, it.NOISE_SEED, 0, B, A))
        assert all(census[k] == v for k, v in again.items())
        assert {"noise_clip_rows", "action_clamp_rows"} <= set(again) and ("qf1_smaller_rows" in again) == (nc == 2)
    if t64.activation == "relu":
        assert it.relu_margin_ok(t64, batch.observations, batch.actions).all()
    for k, v in t64.state_dict().items():                           # the float32 twin holds the same numbers
        assert torch.equal(v, t32.state_dict()[k].double()), k


def test_twins_names_are_sb3s():
    names = set(it.Twin(10, 7, (64, 64), (64,), "relu", 2).state_dict())
    want = {f"{a}.mu.{j}.{p}" for a in ("actor", "actor_target") for j in (0, 2, 4) for p in ("weight", "bias")}
    want |= {f"{c}.qf{q}.{j}.{p}" for c in ("critic", "critic_target") for q in (0, 1) for j in (0, 2) for p in ("weight", "bias")}
    assert names == want
    assert not any(".qf1." in k for k in it.Twin(10, 7, (64,), (64,), "relu", 1).state_dict())


def test_actor_gradient_at_the_head_by_hand():
    """The twin's actor gradient at the head equals -dq_da (1 - a^2) / B, formed by hand in float64: head weight = dz^T h, bias = sum dz."""
    D, A, trunk, B, nc = 25, 4, "64x64-relu", 75, 2
    _, t64, batch, n, _ = it.case(D, A, trunk, B, nc)
    r = it.grads(t64, batch, n)
    a, dq = r["mid"]["action"], r["mid"]["dq_da"]
    dz = -dq * (1.0 - a * a) / B
    with torch.no_grad():
        h = t64.actor.mu[:-2](t64._features(batch.observations)).numpy()
    assert np.allclose(r["grad"]["actor.mu.4.weight"], dz.T @ h, rtol=1e-12, atol=1e-15)
    assert np.allclose(r["grad"]["actor.mu.4.bias"], dz.sum(axis=0), rtol=1e-12, atol=1e-15)
    assert not any(k.startswith(("actor_target", "critic_target")) for k in r["grad"])
    # the actor loss goes through qf0 alone: qf1's weights do not enter it
    with torch.no_grad():
        for p in t64.critic.qf1.parameters():
            p.mul_(1.7)
    again = it.grads(t64, batch, n)
    assert all(np.array_equal(again["grad"][k], r["grad"][k]) for k in r["grad"] if k.startswith("actor."))
    assert r["stats"]["critic_loss"] != again["stats"]["critic_loss"]


def test_critic_loss_has_no_half():
    _, t64, batch, n, _ = it.case(10, 7, "16-tanh", 75, 2)
    y = it.target(t64, batch, n)["target"]
    loss, q = it.critic_loss(t64, batch, y)
    assert np.isclose(float(loss.detach()), float((((q[0] - y) ** 2).mean() + ((q[1] - y) ** 2).mean()).detach()), rtol=1e-14)
    g = torch.autograd.grad(loss, q)[0]
    assert torch.allclose(g, 2.0 * (q - y) / 75, rtol=1e-13)


def test_twins_adam_is_torch_adam_over_three_steps():
    rng = np.random.default_rng(0)
    p0 = rng.normal(size=(5, 3))
    p = torch.tensor(p0, dtype=torch.float64, requires_grad=True)
    opt = torch.optim.Adam([p], lr=1e-3, betas=(0.9, 0.999), eps=1e-8)
    mine, m, v = p0.copy(), np.zeros_like(p0), np.zeros_like(p0)
    for step in (1, 2, 3):
        g = rng.normal(size=p0.shape)
        p.grad = torch.tensor(g)
        opt.step()
        mine, m, v = it.adam_step(mine, g, m, v, step)
        assert np.allclose(mine, p.detach().numpy(), rtol=1e-13, atol=1e-15), step


def test_twin_step_delays_the_actor_and_both_targets():
    """policy_delay = 2: the critic changes every step; the actor and both targets on even steps only, with Adam counts of their own."""
    _, t64, batch, n, _ = it.case(10, 7, "16-tanh", 75, 2)
    state = {}
    for step in (1, 2, 3, 4):
        before = {k: v.clone() for k, v in t64.state_dict().items()}
        stats = it.twin_step(t64, state, batch, n, policy_delay=2)
        changed = {g: any(not torch.equal(before[k], v) for k, v in t64.state_dict().items() if k.startswith(g + "."))
                   for g in ("actor", "actor_target", "critic", "critic_target")}
        assert changed == {"actor": step % 2 == 0, "actor_target": step % 2 == 0, "critic": True, "critic_target": step % 2 == 0}, (step, changed)
        assert (state["n_updates"], state.get("actor_steps", 0)) == (step, step // 2)
        assert (stats["actor_loss"] == 0.0) == (step == 1)
    state = {}
    it.twin_step(t64, state, batch, n, policy_delay=1)
    assert state["actor_steps"] == 1


def test_scaled_noise_restatement():
    eps = it.noise(it.DOMAIN_TARGET, 21, 3, 9, 7)
    n = it.scaled_noise(it.DOMAIN_TARGET, 21, 3, 9, 7, 0.4, 0.5)
    assert np.array_equal(n, np.clip(np.float32(0.4) * eps, np.float32(-0.5), np.float32(0.5))) and (np.abs(eps) > 1.25).any()
    z = it.scaled_noise(it.DOMAIN_ACT, 21, 3, 9, 7, 0.0)
    assert not z.view(np.uint32).any()                               # +0, bit for bit
    assert not np.array_equal(it.noise(it.DOMAIN_ACT, 21, 3, 9, 7), eps)


# ------------------------------------------------------------------------------------------------------------ the blobs
def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0, 0, 0])[:3])


def _floats(L, D, A, pi, qf, nc):
    fa, fc = C.c_int64(-1), C.c_int64(-1)
    total = L.mcg_td3_blob_floats(D, A, len(pi), _arr(pi), len(qf), _arr(qf), nc, C.byref(fa), C.byref(fc))
    return total, fa.value, fc.value


@pytest.mark.parametrize("nc", [1, 2])
@pytest.mark.parametrize("D,A,trunk", it.SHAPES)
def test_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk, nc):
    from mycobotgym_amd import _abi, td3_policy as tp
    pi, qf, act = it.TRUNKS[trunk]
    sd = it.Twin(D, A, pi, qf, act, nc).randomize(11).state_dict()
    total, fa, fc = _floats(_abi.load(), D, A, pi, qf, nc)
    blobs = {"actor": tp.pack_actor(sd, D, A, pi, "actor"), "actor_target": tp.pack_actor(sd, D, A, pi, "actor_target"),
             "critic": tp.pack_critic(sd, D, A, qf, "critic", nc), "critic_target": tp.pack_critic(sd, D, A, qf, "critic_target", nc)}
    assert all(b.dtype == torch.float32 for b in blobs.values())
    assert [b.numel() for b in blobs.values()] == [fa, fa, fc, fc] and total == fa + fc and fa % 16 == 0 and fc % 16 == 0
    back = {}
    for name in ("actor", "actor_target"):
        back.update(tp.unpack_actor(blobs[name], D, A, pi, name))
    for name in ("critic", "critic_target"):
        back.update(tp.unpack_critic(blobs[name], D, A, qf, name, nc))
    assert set(back) == set(sd) == set(tp.state_names(len(pi), len(qf), nc))
    for k, v in sd.items():
        assert back[k].shape == v.shape and back[k].numpy().tobytes() == v.detach().numpy().tobytes(), k
    for name, blob in blobs.items():                                # every weight sits in its blob exactly once; the padding is +0.0
        own = [v for k, v in sd.items() if k.startswith(name + ".")]
        assert int((blob != 0).sum()) == sum(int((v != 0).sum()) for v in own), name
        assert not (blob.view(torch.int32)[blob == 0] != 0).any(), name
        again = (tp.pack_actor(back, D, A, pi, name) if name.startswith("actor") else tp.pack_critic(back, D, A, qf, name, nc))
        assert torch.equal(again.view(torch.int32), blob.view(torch.int32)), name


def test_blob_floats_by_hand_and_refused_shapes(built):
    from mycobotgym_amd import _abi
    L = _abi.load()
    # D = 25, A = 7, [64, 64]: 8 feature k-blocks.  Actor: 4 x 8 x 64 + 64, 4 x 16 x 64 + 64, one head of 16 x 64 + 16.
    actor = (4 * 8 * 64 + 64) + (4 * 16 * 64 + 64) + (16 * 64 + 16)
    one = (4 * 12 * 64 + 64) + (4 * 16 * 64 + 64) + (16 * 64 + 16)
    assert _floats(L, 25, 7, (64, 64), (64, 64), 2) == (actor + 2 * one, actor, 2 * one)
    assert _floats(L, 25, 7, (64, 64), (64, 64), 1) == (actor + one, actor, one)
    for D, A, pi, qf, nc in ((0, 7, (64,), (64,), 2), (25, 17, (64,), (64,), 2), (25, 7, (400, 300), (64,), 2), (25, 7, (64,), (400, 300), 1),
                             (25, 7, (64,), (64,), 0), (25, 7, (64,), (64,), 3), (25, 7, (), (64,), 2)):
        assert _floats(L, D, A, pi, qf, nc) == (0, 0, 0), (D, A, pi, qf, nc)


def test_td3_structs_match_header_layout_and_exports(built, tmp_path):
    from mycobotgym_amd import _abi
    structs = (("mcg_td3", _abi.McgTd3), ("mcg_td3_act_out", _abi.McgTd3ActOut), ("mcg_td3_target_out", _abi.McgTd3TargetOut),
               ("mcg_td3_actor_grad_out", _abi.McgTd3ActorGradOut))
    exprs = ["MCG_TD3_CRITIC", "MCG_TD3_CRITIC_TARGET", "MCG_ABI_VERSION"]
    want = [_abi.TD3_CRITIC, _abi.TD3_CRITIC_TARGET, 8]
    for cname, cls in structs:
        exprs.append(f"sizeof({cname})")
        want.append(C.sizeof(cls))
        for n, _ in cls._fields_:
            exprs.append(f"offsetof({cname},{n})")
            want.append(getattr(cls, n).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    L = _abi.load()
    assert _abi.ABI_VERSION == 8 and L.mcg_abi_version() == 8          # additive: the version stays
    for name in ("mcg_td3_blob_floats", "mcg_td3_act", "mcg_td3_q", "mcg_td3_target", "mcg_td3_polyak", "mcg_td3_grad_work_floats",
                 "mcg_td3_critic_grad", "mcg_td3_actor_grad"):
        assert name in _abi.EXPORTS and hasattr(L, name), name
    import mycobotgym_amd as m
    assert m.TD3Policy is m.td3_policy.TD3Policy and m.TD3Update is m.td3_update.TD3Update
    assert issubclass(m.DDPGPolicy, m.TD3Policy) and issubclass(m.DDPGUpdate, m.TD3Update)


# --------------------------------------------------------------------------------------------------- the C side's refusals
def _td3(_abi, L, **over):
    kw = dict(actor=C.c_void_p(0x1000), actor_target=C.c_void_p(0x3000), critic=C.c_void_p(0x1000), critic_target=C.c_void_p(0x2000), n_envs=40,
              obs_dim=25, act_dim=7, n_pi=2, pi_width=_arr((64, 64)), n_qf=2, qf_width=_arr((64, 64)), activation=_abi.POLICY_RELU, n_critics=2)
    kw.update(over)
    fa, fc = C.c_int64(0), C.c_int64(0)
    L.mcg_td3_blob_floats(kw["obs_dim"], kw["act_dim"], kw["n_pi"], kw["pi_width"], kw["n_qf"], kw["qf_width"], kw["n_critics"], C.byref(fa),
                          C.byref(fc))
    kw.setdefault("actor_floats", fa.value)
    kw.setdefault("critic_floats", fc.value)
    return _abi.McgTd3(**kw)


def test_td3_host_refusals_without_a_gpu(built):
    """Every argument check of the eight entries: the code and a fragment of its message that names the field, with no GPU in the
    machine (the pointers are never dereferenced: the refusals come before any HIP call)."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = 0x1000
    ref = lambda x: None if x is None else C.byref(x)
    obs = _abi.McgStepOut(obs=p, achieved_goal=p, desired_goal=p)
    aout = _abi.McgTd3ActOut(action=p)
    rows = _abi.McgSacRows(obs=p, achieved=p, desired=p, action=p)
    batch = _abi.McgHerBatch(next_obs=p, next_achieved=p, desired=p, reward=p, done=p)
    tout = _abi.McgTd3TargetOut(target=p)
    BIG = 1 << 40

    def act(s, o=obs, q=aout, std=0.1):
        return L.mcg_td3_act(ref(s), ref(o), 0, 0, 0, std, ref(q), None)

    def qv(s, which=0, r=rows, B=8, q=p):
        return L.mcg_td3_q(ref(s), which, ref(r), B, q, None)

    def tgt(s, b=batch, B=8, gamma=0.99, sigma=0.2, clip=0.5, o=tout):
        return L.mcg_td3_target(ref(s), ref(b), B, 0, 0, gamma, sigma, clip, ref(o), None)

    def pk(s, tau=0.005):
        return L.mcg_td3_polyak(ref(s), tau, None)

    def cg(s, r=rows, y=p, B=8, work=p, wf=BIG, grad=p, stats=p):
        return L.mcg_td3_critic_grad(ref(s), ref(r), y, B, work, wf, grad, stats, None)

    def ag(s, r=rows, B=8, work=p, wf=BIG, grad=p, stats=p):
        return L.mcg_td3_actor_grad(ref(s), ref(r), B, work, wf, grad, stats, None, None)

    def refused(code, text):
        assert code == _abi.MCG_ERR_ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    # what all six share
    for entry in (act, qv, tgt, pk, cg, ag):
        refused(entry(None), "null mcg_td3")
        for name in ("obs_dim", "act_dim"):
            for bad in (0, -3):
                refused(entry(_td3(_abi, L, **{name: bad})), name)
        refused(entry(_td3(_abi, L, act_dim=17)), "act_dim must be <= 16")
        refused(entry(_td3(_abi, L, obs_dim=4097)), "obs_dim must be <= 4096")
        for name in ("n_pi", "n_qf"):
            for bad in (0, 4, -1):
                refused(entry(_td3(_abi, L, **{name: bad})), name + " must be in [1, 3]")
        for name in ("pi_width", "qf_width"):
            for bad in ((400, 300), (64, 24), (8, 64), (272, 64), (64, 0), (-16, 64)):
                which = 0 if bad[0] != 64 else 1
                refused(entry(_td3(_abi, L, **{name: _arr(bad)})), f"{name}[{which}] must be a multiple of 16")
        for bad in (0, 3, -1):
            refused(entry(_td3(_abi, L, n_critics=bad, actor_floats=16, critic_floats=16)), "n_critics must be 1 or 2")
        for bad in (2, -1):
            refused(entry(_td3(_abi, L, activation=bad)), "activation")
        good = _td3(_abi, L)
        refused(entry(_td3(_abi, L, actor_floats=good.actor_floats + 16)), "actor_floats")
        refused(entry(_td3(_abi, L, critic_floats=good.critic_floats - 16)), "critic_floats")
        refused(entry(_td3(_abi, L, n_critics=1, critic_floats=good.critic_floats)), "critic_floats")
    good = _td3(_abi, L)
    # the blobs each entry touches: null, misaligned
    touches = {act: ("actor",), qv: ("critic",), tgt: ("actor_target", "critic_target"), pk: ("actor", "actor_target", "critic", "critic_target"),
               cg: ("critic",), ag: ("actor", "critic")}
    for entry, names in touches.items():
        for name in names:
            refused(entry(_td3(_abi, L, **{name: None})), f"{name} is null")
            refused(entry(_td3(_abi, L, **{name: C.c_void_p(0x5008)})), f"{name} is not 16-byte aligned")
    refused(qv(_td3(_abi, L, critic_target=None), which=1), "critic_target is null")
    assert qv(_td3(_abi, L, critic_target=None), B=0) == _abi.MCG_ERR_ARG and b"B must be" in L.mcg_last_error()   # (an untouched blob may be null)
    refused(pk(_td3(_abi, L, critic_target=C.c_void_p(0x1000))), "critic and critic_target are the same blob")
    refused(pk(_td3(_abi, L, actor_target=C.c_void_p(0x1000))), "actor and actor_target are the same blob")
    # mcg_td3_act
    for bad in (0, -3, 2 ** 27):
        refused(act(_td3(_abi, L, n_envs=bad)), "n_envs")
    refused(act(good, o=None), "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal"):
        refused(act(good, o=_abi.McgStepOut(**{n: (None if n == name else p) for n in ("obs", "achieved_goal", "desired_goal")})), "are required")
    for bad in (-0.1, float("nan"), float("inf")):
        refused(act(good, std=bad), "noise_std")
    refused(act(good, q=None), "null mcg_td3_act_out")
    refused(act(good, q=_abi.McgTd3ActOut(mean=p)), "action is required")
    # mcg_td3_q
    for bad in (2, -1):
        refused(qv(good, which=bad), "which")
    for bad in (0, -5, 2 ** 27):
        refused(qv(good, B=bad), "B must be")
    refused(qv(good, r=None), "null mcg_sac_rows")
    for name in ("obs", "achieved", "desired", "action"):
        refused(qv(good, r=_abi.McgSacRows(**{n: (None if n == name else p) for n in ("obs", "achieved", "desired", "action")})), "are required")
    refused(qv(good, q=None), "q is null")
    # mcg_td3_target
    for bad in (0, -5, 2 ** 27):
        refused(tgt(good, B=bad), "B must be")
    refused(tgt(good, b=None), "null mcg_her_batch")
    names = ("next_obs", "next_achieved", "desired", "reward", "done")
    for name in names:
        refused(tgt(good, b=_abi.McgHerBatch(**{n: (None if n == name else p) for n in names})), "are required")
    for bad in (-0.1, 1.5, float("nan")):
        refused(tgt(good, gamma=bad), "gamma")
    for bad in (-0.1, float("nan"), float("inf")):
        refused(tgt(good, sigma=bad), "sigma")
        refused(tgt(good, clip=bad), "clip")
    refused(tgt(good, o=None), "null mcg_td3_target_out")
    refused(tgt(good, o=_abi.McgTd3TargetOut(next_q=p)), "target is required")
    # mcg_td3_polyak
    for bad in (-0.1, 1.5, float("nan")):
        refused(pk(good, tau=bad), "tau")
    # the gradient entries
    assert L.mcg_td3_grad_work_floats(None, 8) == 0 and L.mcg_td3_grad_work_floats(C.byref(good), 0) == 0
    assert L.mcg_td3_grad_work_floats(C.byref(good), 2 ** 27) == 0 and L.mcg_td3_grad_work_floats(C.byref(_td3(_abi, L, n_critics=3)), 8) == 0
    need = L.mcg_td3_grad_work_floats(C.byref(good), 75)
    assert need > 0 and L.mcg_td3_grad_work_floats(C.byref(_td3(_abi, L, n_critics=1)), 75) <= need
    for entry in (cg, ag):
        for bad in (0, -5, 2 ** 27):
            refused(entry(good, B=bad), "B must be")
        refused(entry(good, r=None), "null mcg_sac_rows")
        refused(entry(good, stats=None), "stats is null")
        refused(entry(good, grad=None), "grad is null")
        refused(entry(good, grad=0x1008), "grad is not 16-byte aligned")
        refused(entry(good, work=None), "work is null")
        refused(entry(good, work=0x1004), "work is not 16-byte aligned")
        refused(entry(good, B=75, wf=1024), "work_floats")
    refused(cg(good, B=75, wf=need - 1), "work_floats")
    refused(cg(good, y=None), "y is null")
    for name in ("obs", "achieved", "desired", "action"):
        refused(cg(good, r=_abi.McgSacRows(**{n: (None if n == name else p) for n in ("obs", "achieved", "desired", "action")})), "are required")
    for name in ("obs", "achieved", "desired"):
        refused(ag(good, r=_abi.McgSacRows(**{n: (None if n == name else p) for n in ("obs", "achieved", "desired")})), "are required")


# --------------------------------------------------------------------------------------------------- Python's refusals
def test_python_side_refusals_need_no_gpu(built):
    from mycobotgym_amd import DDPGPolicy, DDPGUpdate, TD3Policy, TD3Update, td3_policy as tp, td3_update as tu
    dims = dict(num_envs=4, obs_dim=10, act_dim=7)
    with pytest.raises(ValueError, match=r"\[400, 300\].*default"):
        TD3Policy(**dims, hidden=(400, 300))                         # SB3's own default net_arch
    with pytest.raises(ValueError, match=r"\[400, 300\]"):
        DDPGPolicy(**dims, hidden=dict(pi=(64,), qf=(400, 300)))
    for n in (3, 0, 2.5, True):
        with pytest.raises(ValueError, match="n_critics"):
            TD3Policy(**dims, n_critics=n)
    with pytest.raises(ValueError, match="gSDE"):
        TD3Policy(**dims, use_sde=True)
    for hidden in ((64, 40), (64, 64, 64, 64), (), dict(pi=(64,), qf=(8,)), (512,)):
        with pytest.raises(ValueError, match="unsupported shape"):
            TD3Policy(**dims, hidden=hidden)
    with pytest.raises(ValueError, match="'pi' and 'qf'"):
        TD3Policy(**dims, hidden=dict(pi=(64,), vf=(64,)))
    with pytest.raises(ValueError, match="activation"):
        TD3Policy(**dims, activation="gelu")
    with pytest.raises(ValueError, match="needs envs= or"):
        TD3Policy(obs_dim=10, act_dim=7)

    class Sde(torch.nn.Module):
        use_sde = True
    with pytest.raises(ValueError, match="gSDE"):
        TD3Policy.from_module(Sde())
    keys = list(it.Twin(10, 7, (64, 64)).state_dict())
    with pytest.raises(ValueError, match="features extractor with parameters"):
        tp._refuse_foreign(keys + ["actor.features_extractor.extractors.observation.0.weight"])
    with pytest.raises(ValueError, match="CNN"):
        tp._refuse_foreign(keys + ["critic.features_extractor.cnn.0.weight"])
    with pytest.raises(ValueError, match="n_critics > 2"):
        tp._refuse_foreign(keys + ["critic.qf2.0.weight"])
    with pytest.raises(ValueError, match="gSDE"):
        tp._refuse_foreign(keys + ["actor.log_std"])
    tp._refuse_foreign(keys)
    tp._refuse_foreign([k for k in keys if ".qf1." not in k])           # DDPG's single critic is served
    # the updater's hyper-parameters and unbuilt keywords
    ok = dict(learning_rate=1e-3, gamma=0.99, tau=0.005, policy_delay=2, target_policy_noise=0.2, target_noise_clip=0.5, betas=(0.9, 0.999),
              eps=1e-8, unbuilt={})
    tu.check_hyper(**ok)

    class OU:                                                        # (stands for OrnsteinUhlenbeckActionNoise)
        pass
    for kw, frag in ((dict(unbuilt={"action_noise": OU()}), "action_noise"), (dict(unbuilt={"optimizer_class": torch.optim.SGD}), "optimizer_class"),
                     (dict(unbuilt={"use_sde": True}), "gSDE"), (dict(unbuilt={"n_critics": 3}), "n_critics"),
                     (dict(learning_rate=lambda f: 1e-3 * f), "schedule"), (dict(learning_rate=0.0), "learning_rate"), (dict(gamma=1.5), "gamma"),
                     (dict(tau=0.0), "tau"), (dict(policy_delay=0), "policy_delay"), (dict(policy_delay=1.5), "policy_delay"),
                     (dict(target_policy_noise=-0.1), "target_policy_noise"), (dict(target_noise_clip=float("inf")), "target_noise_clip"),
                     (dict(betas=(0.9, 1.0)), "betas"), (dict(eps=-1.0), "eps")):
        with pytest.raises(ValueError, match=frag):
            tu.check_hyper(**{**ok, **kw})
    with pytest.raises(TypeError, match="unexpected keyword"):
        tu.check_hyper(**{**ok, "unbuilt": {"bogus": 1}})
    with pytest.raises(ValueError, match="action_noise"):
        TD3Update(object(), action_noise=OU())
    with pytest.raises(ValueError, match="needs a TD3Policy"):
        DDPGUpdate(object())
    # the collection noise: a float only
    with pytest.raises(ValueError, match="action_noise object"):
        TD3Policy.forward(object.__new__(TD3Policy), {}, noise_std=OU())
    with pytest.raises(ValueError, match="noise_std must be finite"):
        TD3Policy.forward(object.__new__(TD3Policy), {}, noise_std=-0.5)
    # the picture samples of the -v1 ids
    from mycobotgym_amd.sac_update import check_batch
    pictures = it.Batch(observations=torch.zeros(5, 3, 8, 8, dtype=torch.uint8), actions=torch.zeros(5, 7),
                        next_observations=torch.zeros(5, 3, 8, 8, dtype=torch.uint8), dones=torch.zeros(5, 1), rewards=torch.zeros(5, 1))
    with pytest.raises(ValueError, match="picture"):
        check_batch(pictures, 10, 7, None, "TD3Update")
