"""SAC's actor, critics and TD target without a GPU: the restated rule against its torch twin, the makers' conditions, the blobs'
packing, the ABI's layout, the host refusals, the restated noise's own properties and the Polyak expression (tests/indep_sac.py).

The module imports ``mycobotgym_amd.sac_policy`` at its head (importing it loads no library), so every test here, the ones that
exercise the restatement and the makers alone included, fails where the feature is absent."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from mycobotgym_amd import sac_policy as sp
from tests import indep_sac as isac

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SEED = 21


def _t(d):
    return {k: torch.from_numpy(np.ascontiguousarray(v)) for k, v in d.items()}


@pytest.mark.parametrize("D,A,trunk", isac.CASES)
def test_twin_in_float64_is_the_restated_rule(D, A, trunk):
    """The twin cast to float64 == the numpy rule to 1e-12 for the action, the log-prob, both Q pairs and the target, on weights
    whose log_std head reaches both clamp bounds: the restatement is SB3's formula."""
    pi, qf, act = isac.TRUNKS[trunk]
    twin = isac.Twin(D, A, pi, qf, act).randomize(3, D)
    sd = twin.numpy_state()
    twin = twin.double()
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith(".bias"))
    eps = isac.noise64(isac.DOMAIN_ACT, 9, 2, 40, A)
    obs = isac.conditioned_obs(sd, act, 40, D, 5, eps)
    with torch.no_grad():
        a, lp, mu, ls, u = (x.numpy() for x in twin.action_log_prob(_t(obs), torch.from_numpy(eps)))
        sb3 = twin.gaussian_terms_sb3_form(*(torch.from_numpy(x) for x in (mu, ls, u))).numpy()
        det = twin.action_log_prob(_t(obs), deterministic=True)[0].numpy()
    mu64, ls64, _ = isac.actor_rule(sd, obs, act)
    assert np.abs(mu - mu64).max() <= 1e-12 and np.abs(ls - ls64).max() <= 1e-12
    assert np.abs(a - np.tanh(isac.pre_squash(mu64, ls64, eps))).max() <= 1e-12
    assert np.abs(lp - isac.log_prob(eps, ls64, a)).max() <= 1e-12
    assert np.abs(det - np.tanh(mu64)).max() <= 1e-12
    # SB3 spells the Gaussian term Normal(mu, std).log_prob(u): the same number wherever (u - mu) / std is well-conditioned
    mild = ls64 >= -10.0
    assert mild.any() and np.abs(sb3 - (-0.5 * eps ** 2 - ls64 - isac.LOG_SQRT_2PI))[mild].max() <= 1e-8
    act_in = np.random.default_rng(1).uniform(-1, 1, (40, A))
    with torch.no_grad():
        for target, prefix in ((False, "critic"), (True, "critic_target")):
            q = twin.q(_t(obs), torch.from_numpy(act_in), target=target).numpy()
            assert q.shape == (2, 40) and np.abs(q - isac.q_rule(sd, prefix, obs, act_in, act)).max() <= 1e-12
        assert np.abs(isac.q_rule(sd, "critic", obs, act_in, act) - isac.q_rule(sd, "critic_target", obs, act_in, act)).min() > 1e-6
        eps8 = isac.noise64(isac.DOMAIN_TARGET, 9, 0, 75, A)
        b = isac.replay_batch(sd, act, 75, D, A, 11, eps8)
        got = twin.target(_t(b.next_observations), torch.from_numpy(b.rewards), torch.from_numpy(b.dones), torch.from_numpy(eps8), 0.97, 0.3)
    want = isac.target_rule(sd, b.next_observations, b.rewards, b.dones, eps8, 0.97, 0.3, act)
    for k, v in want.items():
        assert np.abs(got[k].numpy() - v).max() <= 1e-12, k


def test_concatenation_order_is_sorted_keys():
    obs = {"observation": np.full((2, 4), 3.0), "achieved_goal": np.full((2, 3), 1.0), "desired_goal": np.full((2, 3), 2.0)}
    assert isac.features(obs)[0].tolist() == [1.0] * 3 + [2.0] * 3 + [3.0] * 4
    assert list(isac.KEYS) == sorted(obs)


@pytest.mark.parametrize("D,A,trunk", isac.CASES)
def test_makers_meet_their_conditions(D, A, trunk):
    """What tests/test_gpu_sac.py relies on: in the float64 rule every |tanh(u)| <= 0.99 and every pre-clamp log_std is at least 1e-3
    from -20 and from 2, for the collection rows (N = 40, 17) and the replay batches (B = 75, 1); both clamp bounds act in some rows
    of the large shapes; `done` has both values."""
    pi, qf, act = isac.TRUNKS[trunk]
    sd = isac.Twin(D, A, pi, qf, act).randomize(3, D).numpy_state()
    for n in (40, 17):
        eps = isac.noise(isac.DOMAIN_ACT, SEED, 0, n, A)
        obs = isac.conditioned_obs(sd, act, n, D, 5, eps)
        assert isac.conditions(sd, obs, eps, act).all()
        mu, ls, raw = isac.actor_rule(sd, isac.round32(obs), act)
        assert np.abs(np.tanh(isac.pre_squash(mu, ls, eps))).max() <= isac.MAX_SQUASHED
        assert min(np.abs(raw - 2.0).min(), np.abs(raw + 20.0).min()) >= isac.CLAMP_MARGIN
        if n == 40:
            assert (raw > 2.0).any() and (raw < -20.0).any() and ((raw > -20.0) & (raw < 2.0)).any()
            assert (ls == 2.0).any() and (ls == -20.0).any()
    for B in (75, 1):
        eps = isac.noise(isac.DOMAIN_TARGET, SEED, 0, B, A)
        b = isac.replay_batch(sd, act, B, D, A, 11, eps)
        assert isac.conditions(sd, b.next_observations, eps, act).all()
        assert all(v.dtype == np.float32 for v in (*b.observations.values(), *b.next_observations.values(), b.actions, b.dones, b.rewards))
        assert b.dones.shape == b.rewards.shape == (B, 1) and np.abs(b.actions).max() <= 1.0
        if B == 75:
            raw = isac.actor_rule(sd, isac.round32(b.next_observations), act)[2]
            assert (raw > 2.0).any() and (raw < -20.0).any()
            assert set(np.unique(b.dones)) == {0.0, 1.0} and (b.rewards > 0).any() and (b.rewards < 0).any()


def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0, 0, 0])[:3])


def _floats(L, D, A, pi, qf):
    fa, fc = C.c_int64(-1), C.c_int64(-1)
    total = L.mcg_sac_blob_floats(D, A, len(pi), _arr(pi), len(qf), _arr(qf), C.byref(fa), C.byref(fc))
    return total, fa.value, fc.value


@pytest.mark.parametrize("D,A,trunk", isac.CASES)
def test_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk):
    from mycobotgym_amd import _abi, sac_policy as sp
    pi, qf, act = isac.TRUNKS[trunk]
    sd = isac.Twin(D, A, pi, qf, act).randomize(11, D).state_dict()
    total, fa, fc = _floats(_abi.load(), D, A, pi, qf)
    blobs = {"actor": sp.pack_actor(sd, D, A, pi), "critic": sp.pack_critic(sd, D, A, qf, "critic"),
             "critic_target": sp.pack_critic(sd, D, A, qf, "critic_target")}
    assert all(b.dtype == torch.float32 for b in blobs.values())
    assert (blobs["actor"].numel(), blobs["critic"].numel(), blobs["critic_target"].numel()) == (fa, fc, fc) and total == fa + fc
    assert fa % 16 == 0 and fc % 32 == 0
    back = sp.unpack_actor(blobs["actor"], D, A, pi)
    back.update(sp.unpack_critic(blobs["critic"], D, A, qf, "critic"))
    back.update(sp.unpack_critic(blobs["critic_target"], D, A, qf, "critic_target"))
    assert set(back) == set(sd) == set(sp.state_names(len(pi), len(qf)))
    for k, v in sd.items():
        assert back[k].shape == v.shape and back[k].numpy().tobytes() == v.detach().numpy().tobytes(), k
    # every weight sits in its blob exactly once, and the padding is +0.0
    for name, blob in blobs.items():
        own = [v for k, v in sd.items() if k.startswith(name + ".")]
        assert int((blob != 0).sum()) == sum(int((v != 0).sum()) for v in own), name
        assert not (blob.view(torch.int32)[blob == 0] != 0).any(), name


def test_blob_floats_by_hand_and_refused_shapes(built):
    from mycobotgym_amd import _abi
    L = _abi.load()
    # D = 25, A = 7, [64, 64]: 8 feature k-blocks.  Actor: 4 x 8 x 64 + 64, 4 x 16 x 64 + 64, two heads of 16 x 64 + 16.
    # A critic: 4 x (8 + 4) x 64 + 64, 4 x 16 x 64 + 64, head 16 x 64 + 16; two of them.
    actor = (4 * 8 * 64 + 64) + (4 * 16 * 64 + 64) + 2 * (16 * 64 + 16)
    critic = 2 * ((4 * 12 * 64 + 64) + (4 * 16 * 64 + 64) + (16 * 64 + 16))
    assert _floats(L, 25, 7, (64, 64), (64, 64)) == (actor + critic, actor, critic)
    assert L.mcg_sac_blob_floats(25, 7, 2, _arr((64, 64)), 2, _arr((64, 64)), None, None) == actor + critic
    for D, A, pi, qf in ((0, 7, (64,), (64,)), (25, 0, (64,), (64,)), (25, 17, (64,), (64,)), (4097, 7, (64,), (64,)), (25, 7, (), (64,)),
                         (25, 7, (64,), ()), (25, 7, (400, 300), (64,)), (25, 7, (64,), (400, 300)), (25, 7, (64, 40), (64,)),
                         (25, 7, (64,), (8,))):
        assert _floats(L, D, A, pi, qf) == (0, 0, 0), (D, A, pi, qf)
    assert L.mcg_sac_blob_floats(25, 7, 4, _arr((64, 64, 64)), 1, _arr((64,)), None, None) == 0
    assert L.mcg_sac_blob_floats(25, 7, 1, None, 1, _arr((64,)), None, None) == 0


def test_sac_structs_match_header_layout(built, tmp_path):
    from mycobotgym_amd import _abi
    structs = (("mcg_sac", _abi.McgSac), ("mcg_sac_act_out", _abi.McgSacActOut), ("mcg_sac_rows", _abi.McgSacRows),
               ("mcg_sac_target_out", _abi.McgSacTargetOut))
    exprs = ["MCG_SAC_CRITIC", "MCG_SAC_CRITIC_TARGET", "MCG_ABI_VERSION"]
    want = [_abi.SAC_CRITIC, _abi.SAC_CRITIC_TARGET, 8]
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
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays
    for name in ("mcg_sac_blob_floats", "mcg_sac_act", "mcg_sac_q", "mcg_sac_target", "mcg_sac_polyak"):
        assert name in _abi.EXPORTS
    import mycobotgym_amd
    assert mycobotgym_amd.SACPolicy is mycobotgym_amd.sac_policy.SACPolicy


def _sac(_abi, L, **over):
    p = C.c_void_p(0x1000)
    kw = dict(actor=p, critic=p, critic_target=C.c_void_p(0x2000), n_envs=40, obs_dim=25, act_dim=7, n_pi=2, pi_width=_arr((64, 64)), n_qf=2,
              qf_width=_arr((64, 64)), activation=_abi.POLICY_RELU)
    kw.update(over)
    _, fa, fc = 0, C.c_int64(0), C.c_int64(0)
    L.mcg_sac_blob_floats(kw["obs_dim"], kw["act_dim"], kw["n_pi"], kw["pi_width"], kw["n_qf"], kw["qf_width"], C.byref(fa), C.byref(fc))
    kw.setdefault("actor_floats", fa.value)
    kw.setdefault("critic_floats", fc.value)
    return _abi.McgSac(**kw)


def test_sac_host_refusals_without_a_gpu(built):
    """Every argument check of the four entries: the code and a fragment of its message that names the field, with no GPU in the
    machine (the pointers are never dereferenced: the refusals come before any HIP call)."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = 0x1000
    ref = lambda x: None if x is None else C.byref(x)
    obs = _abi.McgStepOut(obs=p, achieved_goal=p, desired_goal=p)
    aout = _abi.McgSacActOut(action=p)
    rows = _abi.McgSacRows(obs=p, achieved=p, desired=p, action=p)
    batch = _abi.McgHerBatch(next_obs=p, next_achieved=p, desired=p, reward=p, done=p)
    tout = _abi.McgSacTargetOut(target=p)

    def act(s, o=obs, q=aout):
        return L.mcg_sac_act(ref(s), ref(o), 0, 0, 0, 0, ref(q), None)

    def qv(s, which=0, r=rows, B=8, q=p):
        return L.mcg_sac_q(ref(s), which, ref(r), B, q, None)

    def tgt(s, b=batch, B=8, gamma=0.99, ent=0.2, lec=None, o=tout):
        return L.mcg_sac_target(ref(s), ref(b), B, 0, 0, gamma, ent, lec, ref(o), None)

    def pk(s, tau=0.005):
        return L.mcg_sac_polyak(ref(s), tau, None)

    def refused(code, text):
        assert code == _abi.MCG_ERR_ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    # what all four share
    for entry in (act, qv, tgt, pk):
        refused(entry(None), "null mcg_sac")
        for name in ("obs_dim", "act_dim"):
            for bad in (0, -3):
                refused(entry(_sac(_abi, L, **{name: bad})), name)
        refused(entry(_sac(_abi, L, act_dim=17)), "act_dim must be <= 16")
        refused(entry(_sac(_abi, L, obs_dim=4097)), "obs_dim must be <= 4096")
        for name in ("n_pi", "n_qf"):
            for bad in (0, 4, -1):
                refused(entry(_sac(_abi, L, **{name: bad})), name + " must be in [1, 3]")
        for name in ("pi_width", "qf_width"):
            for bad in ((400, 300), (64, 24), (8, 64), (272, 64), (64, 0), (-16, 64)):
                which = 0 if bad[0] != 64 else 1
                refused(entry(_sac(_abi, L, **{name: _arr(bad)})), f"{name}[{which}] must be a multiple of 16")
        for bad in (2, -1):
            refused(entry(_sac(_abi, L, activation=bad)), "activation")
        good = _sac(_abi, L)
        refused(entry(_sac(_abi, L, actor_floats=good.actor_floats + 16)), "actor_floats")
        refused(entry(_sac(_abi, L, critic_floats=good.critic_floats - 16)), "critic_floats")
    good = _sac(_abi, L)
    # the blobs each entry touches
    refused(act(_sac(_abi, L, actor=None)), "actor is null")
    refused(act(_sac(_abi, L, actor=C.c_void_p(0x1008))), "not 16-byte aligned")
    refused(qv(_sac(_abi, L, critic=None)), "critic is null")
    refused(qv(_sac(_abi, L, critic_target=None), which=1), "critic_target is null")
    refused(qv(_sac(_abi, L, critic=C.c_void_p(0x1004))), "not 16-byte aligned")
    refused(tgt(_sac(_abi, L, actor=None)), "actor is null")
    refused(tgt(_sac(_abi, L, critic_target=None)), "critic_target is null")
    refused(tgt(_sac(_abi, L, critic_target=C.c_void_p(0x2008))), "not 16-byte aligned")
    refused(pk(_sac(_abi, L, critic=None)), "critic is null")
    refused(pk(_sac(_abi, L, critic_target=None)), "critic_target is null")
    refused(pk(_sac(_abi, L, critic_target=C.c_void_p(0x1000))), "same blob")
    # mcg_sac_act
    for bad in (0, -3, 2 ** 27):
        refused(act(_sac(_abi, L, n_envs=bad)), "n_envs")
    refused(act(good, o=None), "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal"):
        refused(act(good, o=_abi.McgStepOut(**{n: (None if n == name else p) for n in ("obs", "achieved_goal", "desired_goal")})), "are required")
    refused(act(good, q=None), "null mcg_sac_act_out")
    refused(act(good, q=_abi.McgSacActOut(log_prob=p, mean=p)), "action is required")
    # mcg_sac_q
    for bad in (2, -1):
        refused(qv(good, which=bad), "which")
    for bad in (0, -5, 2 ** 27):
        refused(qv(good, B=bad), "B must be")
    refused(qv(good, r=None), "null mcg_sac_rows")
    for name in ("obs", "achieved", "desired", "action"):
        refused(qv(good, r=_abi.McgSacRows(**{n: (None if n == name else p) for n in ("obs", "achieved", "desired", "action")})), "are required")
    refused(qv(good, q=None), "q is null")
    # mcg_sac_target
    for bad in (0, -5, 2 ** 27):
        refused(tgt(good, B=bad), "B must be")
    refused(tgt(good, b=None), "null mcg_her_batch")
    names = ("next_obs", "next_achieved", "desired", "reward", "done")
    for name in names:
        refused(tgt(good, b=_abi.McgHerBatch(**{n: (None if n == name else p) for n in names})), "are required")
    for bad in (-0.1, 1.5, float("nan")):
        refused(tgt(good, gamma=bad), "gamma")
    for bad in (-0.1, float("nan"), float("inf")):
        refused(tgt(good, ent=bad), "ent_coef")
    refused(tgt(good, ent=-1.0, lec=p, o=None), "null mcg_sac_target_out")       # with log_ent_coef the host's ent_coef is not read
    refused(tgt(good, o=_abi.McgSacTargetOut(next_q=p)), "target is required")
    # mcg_sac_polyak
    for bad in (-0.1, 1.5, float("nan")):
        refused(pk(good, tau=bad), "tau")


def test_python_side_refusals_need_no_gpu(built):
    from mycobotgym_amd import SACPolicy, sac_policy as sp
    with pytest.raises(ValueError, match="gSDE"):
        SACPolicy(num_envs=4, obs_dim=10, act_dim=7, use_sde=True)
    for n in (1, 3):
        with pytest.raises(ValueError, match="n_critics != 2"):
            SACPolicy(num_envs=4, obs_dim=10, act_dim=7, n_critics=n)
    with pytest.raises(ValueError, match=r"TD3 / DDPG default net_arch \[400, 300\]"):
        SACPolicy(num_envs=4, obs_dim=10, act_dim=7, hidden=(400, 300))
    for hidden in ((64, 40), (64, 64, 64, 64), (), dict(pi=(64,), qf=(8,))):
        with pytest.raises(ValueError, match="unsupported shape"):
            SACPolicy(num_envs=4, obs_dim=10, act_dim=7, hidden=hidden)
    with pytest.raises(ValueError, match="'pi' and 'qf'"):
        SACPolicy(num_envs=4, obs_dim=10, act_dim=7, hidden=dict(pi=(64,), vf=(64,)))
    with pytest.raises(ValueError, match="activation"):
        SACPolicy(num_envs=4, obs_dim=10, act_dim=7, activation="gelu")
    with pytest.raises(ValueError, match="needs envs= or"):
        SACPolicy(obs_dim=10, act_dim=7)

    class Sde(torch.nn.Module):
        use_sde = True

    class Three(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.critic = torch.nn.Module()
            self.critic.n_critics = 3
    with pytest.raises(ValueError, match="gSDE"):
        SACPolicy.from_module(Sde())
    with pytest.raises(ValueError, match="n_critics != 2"):
        SACPolicy.from_module(Three())
    keys = list(isac.Twin(10, 7, (64, 64)).state_dict())
    with pytest.raises(ValueError, match="features extractor with parameters"):
        sp._refuse_foreign(keys + ["actor.features_extractor.extractors.observation.0.weight"])
    with pytest.raises(ValueError, match="CNN"):
        sp._refuse_foreign(keys + ["critic.features_extractor.cnn.0.weight"])
    with pytest.raises(ValueError, match="n_critics != 2"):
        sp._refuse_foreign(keys + ["critic.qf2.0.weight"])
    with pytest.raises(ValueError, match="n_critics != 2"):
        sp._refuse_foreign([k for k in keys if ".qf1." not in k])
    with pytest.raises(ValueError, match="gSDE"):
        sp._refuse_foreign(keys + ["actor.log_std"])
    sp._refuse_foreign(keys)
    # batches: float64, mis-shaped, on another device
    dev = torch.device("cuda:0")
    obs = {"observation": torch.zeros(5, 10), "achieved_goal": torch.zeros(5, 3), "desired_goal": torch.zeros(5, 3)}
    act = torch.zeros(5, 7)
    assert sp.batch_rows(obs, act, 10, 7, "q_values") == 5 and sp.batch_rows(obs, None, 10, 7, "td_target") == 5
    with pytest.raises(ValueError, match="expected float32"):
        sp.batch_rows({**obs, "observation": torch.zeros(5, 10, dtype=torch.float64)}, act, 10, 7, "q_values")
    with pytest.raises(ValueError, match="expected float32"):
        sp.batch_rows(obs, act.double(), 10, 7, "q_values")
    with pytest.raises(ValueError, match="expected shape"):
        sp.batch_rows({**obs, "achieved_goal": torch.zeros(5, 4)}, act, 10, 7, "q_values")
    with pytest.raises(ValueError, match="expected shape"):
        sp.batch_rows(obs, torch.zeros(4, 7), 10, 7, "q_values")
    with pytest.raises(ValueError, match="lacks"):
        sp.batch_rows({"observation": torch.zeros(5, 10)}, act, 10, 7, "q_values")
    with pytest.raises(ValueError, match="must be the dict"):
        sp.batch_rows(torch.zeros(5, 3, 8, 8, dtype=torch.uint8), act, 10, 7, "q_values")
    with pytest.raises(ValueError, match="empty"):
        sp.batch_rows({k: v[:0] for k, v in obs.items()}, act[:0], 10, 7, "q_values")
    with pytest.raises(ValueError, match="lives on cpu"):
        sp.batch_rows(obs, act, 10, 7, "q_values", dev)
    with pytest.raises(ValueError, match="expected shape"):
        sp._per_row(torch.zeros(5, 2), 5, "rewards", "td_target", None)
    with pytest.raises(ValueError, match="expected float32"):
        sp._per_row(torch.zeros(5, 1, dtype=torch.float64), 5, "dones", "td_target", None)
    with pytest.raises(ValueError, match="lives on cpu"):
        sp._per_row(torch.zeros(5, 1), 5, "dones", "td_target", dev)


def test_caller_owned_outputs_are_checked_before_the_kernel():
    """``forward`` and ``td_target`` hand ``out``'s tensors to the kernel as bare pointers: another dtype, a short or transposed
    tensor, a view with gaps, another device or an unknown name is refused on the host (``check_out``, which both go through)."""
    shapes = {"target": (5,), "next_log_prob": (5,), "next_q": (2, 5), "next_action": (5, 7), "noise": (5, 7)}
    good = {k: torch.zeros(s) for k, s in shapes.items()}
    assert sp.check_out(good, shapes, "target", "td_target") is good
    assert sp.check_out({"target": good["target"]}, shapes, "target", "td_target").keys() == {"target"}
    assert sp.check_out({"target": torch.zeros(9)[2:7]}, shapes, "target", "td_target")         # a contiguous slice of a larger tensor
    for bad, why in ((None, "'target' is required"), ({"next_q": good["next_q"]}, "'target' is required"),
                     ({**good, "mean": torch.zeros(5, 7)}, r"unknown \['mean'\]"),
                     ({**good, "next_q": torch.zeros(2, 5, dtype=torch.float64)}, r"out\['next_q'\]: expected a contiguous float32"),
                     ({**good, "next_q": torch.zeros(2, 4)}, r"out\['next_q'\]"),
                     ({**good, "next_q": torch.zeros(5, 2)}, r"out\['next_q'\]"),
                     ({**good, "next_action": torch.zeros(7, 5).t()}, r"out\['next_action'\]: expected a contiguous"),
                     ({**good, "noise": torch.zeros(5, 14)[:, ::2]}, r"out\['noise'\]: expected a contiguous"),
                     ({**good, "target": torch.zeros(5, 1)}, r"out\['target'\]"),
                     ({**good, "target": np.zeros(5, np.float32)}, r"out\['target'\]")):
        with pytest.raises(ValueError, match=why):
            sp.check_out(bad, shapes, "target", "td_target")
    with pytest.raises(ValueError, match=r"out\['target'\] lives on cpu"):
        sp.check_out(good, shapes, "target", "td_target", torch.device("cuda:0"))


def test_philox_restatement_and_counter_layout():
    from tests import indep_policy as ip
    rng = np.random.default_rng(1)
    for _ in range(50):
        ctr, key = rng.integers(0, 2 ** 32, 4).tolist(), rng.integers(0, 2 ** 32, 2).tolist()
        assert isac.philox4x32_10(ctr, key) == ip.philox4x32_10(ctr, key)
    assert isac.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]      # Random123
    assert isac.counter(7, 5, 9, 3) == [5, 9, 3, 7] and isac.counter(8, 5, 9, 3) == [5, 9, 3, 8]
    assert isac.counter(8, 2 ** 32 + 5, 2 ** 32 * 7 + 9, 3) == [5, 9, 3 ^ (7 << 8), 8 ^ (1 << 8)]
    # the layout is the actor-critic policy's with another domain byte; 0-6 are taken
    assert isac.counter(ip.DOMAIN, 5, 9, 3) == ip.counter(5, 9, 3)
    from tests import indep_her, indep_replay_img, indep_rollout, indep_scene_rand
    taken = {0, 1, indep_scene_rand.STREAM, indep_her.STREAM, indep_rollout.STREAM, indep_replay_img.STREAM, ip.DOMAIN}
    assert taken == set(range(7)) and not {isac.DOMAIN_ACT, isac.DOMAIN_TARGET} & taken and isac.DOMAIN_ACT != isac.DOMAIN_TARGET


def test_restated_noise_is_standard_normal_and_blocks_are_distinct():
    """Per domain 40 rows x 8 components x 64 calls, n = 20480: the mean within 4 / sqrt(n) of 0, the variance within 4 sqrt(2 / n)
    of 1; no two (domain, row, call, pair) blocks equal, domain 6's (the actor-critic policy's) included."""
    from tests import indep_policy as ip
    N, A, calls, seed = 40, 8, 64, 0
    blocks = set()
    for dom in (isac.DOMAIN_ACT, isac.DOMAIN_TARGET):
        eps = np.stack([isac.noise64(dom, seed, c, N, A) for c in range(calls)])
        n = eps.size
        assert n == 20480
        print(f"domain {dom}: mean {eps.mean():+.5f} (bound {4 / math.sqrt(n):.5f}), variance {eps.var():.5f} (1 +- {4 * math.sqrt(2 / n):.5f})")
        assert abs(eps.mean()) <= 4 / math.sqrt(n)
        assert abs(eps.var() - 1.0) <= 4 * math.sqrt(2.0 / n)
        blocks |= {tuple(isac.block(dom, seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
    blocks |= {tuple(ip.block(seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
    assert len(blocks) == 3 * N * calls * (A // 2)
    # an odd A uses the first component of its last pair; the id is what counts, not the row
    assert np.array_equal(isac.noise(7, seed, 3, 40, 7), isac.noise(7, seed, 3, 40, 8)[:, :7])
    assert np.array_equal(isac.noise(7, seed, 3, 16, 8, id_offset=24), isac.noise(7, seed, 3, 40, 8)[24:])
    assert not np.array_equal(isac.noise(7, seed, 3, 40, 8), isac.noise(8, seed, 3, 40, 8))


def test_polyak_restatement_is_within_one_ulp_of_float64():
    rng = np.random.default_rng(4)
    c = np.concatenate([rng.normal(size=3000), [0.0, 0.0, 1.0, -1.0]]).astype(np.float32)
    t = np.concatenate([rng.normal(size=3000), [0.0, 1.0, 0.0, 1.0]]).astype(np.float32)
    for tau in (0.005, 0.5, 0.999):
        got, want = isac.polyak_restated(c, t, tau), isac.polyak_rule(c, t, tau)
        ulp = np.spacing(np.abs(want).astype(np.float32)).astype(np.float64)
        assert (np.abs(got.astype(np.float64) - want) <= ulp).all(), tau
    assert np.array_equal(isac.polyak_restated(c, t, 1.0).view(np.uint32), c.view(np.uint32))
    odd_c, odd_t = np.array([-0.0, 1.5, -2.0], np.float32), np.array([0.0, np.inf, np.nan], np.float32)       # tau = 1 is a copy
    assert np.array_equal(isac.polyak_restated(odd_c, odd_t, 1.0).view(np.uint32), odd_c.view(np.uint32))
    assert np.array_equal(isac.polyak_restated(c, t, 0.0).view(np.uint32), t.view(np.uint32))
    zero = isac.polyak_restated(np.zeros(4, np.float32), np.zeros(4, np.float32), 0.005)
    assert not zero.view(np.uint32).any()                        # padding stays +0.0
