"""The actor-critic policy without a GPU: the restated rule against its torch twin, the blob's packing, the ABI's layout, the host
refusals, and the restated noise's own properties (tests/indep_policy.py)."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import indep_policy as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = [(D, A, name) for (D, A) in ip.DIMS for name in ("64x64-tanh", "48x32-relu-vf16", "16-tanh")] + [(25, 4, "256x256-relu")]


@pytest.mark.parametrize("D,A,trunk", CASES)
def test_twin_in_float64_is_the_restated_rule(D, A, trunk):
    """The twin cast to float64 == the numpy rule to 1e-12, on random weights with non-zero biases and random inputs, for the mean,
    the value, the sampled action and its log-prob: the restatement is SB3's formula."""
    pi, vf, act = ip.TRUNKS[trunk]
    twin = ip.Twin(D, A, pi, vf, act).randomize(3).double()
    sd = twin.numpy_state()
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith(".bias") or k == "log_std")
    obs = ip.random_obs(40, D, seed=5)
    eps = ip.noise64(9, 2, 40, A)
    with torch.no_grad():
        a, v, lp, m = (x.numpy() for x in twin({k: torch.from_numpy(x) for k, x in obs.items()}, noise=torch.from_numpy(eps)))
    mean, value = ip.rule(sd, obs, act)
    assert np.abs(m - mean).max() <= 1e-12 and np.abs(v - value).max() <= 1e-12
    assert np.abs(a - ip.sample(mean, sd["log_std"], eps)).max() <= 1e-12
    assert np.abs(lp - ip.log_prob(a, mean, sd["log_std"])).max() <= 1e-12
    # at the sampled action the log-prob is the noise's: the form the kernel evaluates
    assert np.abs(lp - (-0.5 * eps ** 2 - sd["log_std"] - ip.LOG_SQRT_2PI).sum(-1)).max() <= 1e-12


def test_concatenation_order_is_sorted_keys():
    obs = {"observation": np.full((2, 4), 3.0), "achieved_goal": np.full((2, 3), 1.0), "desired_goal": np.full((2, 3), 2.0)}
    assert ip.features(obs)[0].tolist() == [1.0] * 3 + [2.0] * 3 + [3.0] * 4
    assert list(ip.KEYS) == sorted(obs)


@pytest.mark.parametrize("D,A,trunk", CASES)
def test_pack_unpack_round_trip_bit_for_bit(built, D, A, trunk):
    from mycobotgym_amd import _abi, policy
    pi, vf, act = ip.TRUNKS[trunk]
    sd = ip.Twin(D, A, pi, vf, act).randomize(11).state_dict()
    blob = policy.pack(sd, D, A, pi, vf)
    arr = lambda w: (C.c_int32 * 3)(*(list(w) + [0, 0, 0])[:3])
    assert blob.dtype == torch.float32 and blob.numel() == _abi.load().mcg_policy_blob_floats(D, A, len(pi), arr(pi), len(vf), arr(vf))
    back = policy.unpack(blob, D, A, pi, vf)
    assert set(back) == set(sd) == set(policy.state_names(len(pi), len(vf)))
    for k, v in sd.items():
        assert back[k].shape == v.shape and back[k].numpy().tobytes() == v.detach().numpy().tobytes(), k
    # every weight sits in the blob exactly once, and the padding is zeros
    assert int((blob != 0).sum()) == sum(int((v != 0).sum()) for v in sd.values())


def test_policy_structs_match_header_layout(built, tmp_path):
    from mycobotgym_amd import _abi
    pf = [n for n, _ in _abi.McgPolicy._fields_]
    of = [n for n, _ in _abi.McgPolicyOut._fields_]
    exprs = (["sizeof(mcg_policy)", "sizeof(mcg_policy_out)", "MCG_POLICY_TANH", "MCG_POLICY_RELU"] + [f"offsetof(mcg_policy,{n})" for n in pf]
             + [f"offsetof(mcg_policy_out,{n})" for n in of])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_abi.McgPolicy), C.sizeof(_abi.McgPolicyOut), _abi.POLICY_TANH, _abi.POLICY_RELU]
            + [getattr(_abi.McgPolicy, n).offset for n in pf] + [getattr(_abi.McgPolicyOut, n).offset for n in of])
    assert got == want
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays
    assert "mcg_policy_blob_floats" in _abi.EXPORTS and "mcg_policy_forward" in _abi.EXPORTS
    import mycobotgym_amd
    assert mycobotgym_amd.ActorCritic is mycobotgym_amd.policy.ActorCritic


def _arr(w):
    return (C.c_int32 * 3)(*(list(w) + [0, 0, 0])[:3])


def _pol(_abi, L, **over):
    kw = dict(blob=C.c_void_p(0x1000), n_envs=40, obs_dim=25, act_dim=7, n_pi=2, n_vf=2, pi_width=_arr((64, 64)), vf_width=_arr((64, 64)),
              activation=_abi.POLICY_TANH)
    kw.update(over)
    floats = L.mcg_policy_blob_floats(kw["obs_dim"], kw["act_dim"], kw["n_pi"], kw["pi_width"], kw["n_vf"], kw["vf_width"])
    kw.setdefault("blob_floats", floats)
    return _abi.McgPolicy(**kw)


def test_policy_host_refusals_without_a_gpu(built):
    """Every argument check of mcg_policy_forward: the code and a fragment of its message that names the field, with no GPU in the
    machine (the pointers are never dereferenced: the refusals come before any HIP call)."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = 0x1000
    obs = _abi.McgStepOut(obs=p, achieved_goal=p, desired_goal=p)
    out = _abi.McgPolicyOut(action=p, value=p, log_prob=p)
    ref = lambda x: None if x is None else C.byref(x)

    def forward(pol, o=obs, q=out):
        return L.mcg_policy_forward(ref(pol), ref(o), 0, 0, 0, 0, ref(q), None)

    def refused(code, text):
        assert code == _abi.MCG_ERR_ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    refused(forward(None), "null mcg_policy")
    refused(forward(_pol(_abi, L, blob=None)), "blob is null")
    for name in ("n_envs", "obs_dim", "act_dim"):
        for bad in (0, -3):
            refused(forward(_pol(_abi, L, **{name: bad})), name)
    refused(forward(_pol(_abi, L, act_dim=17)), "act_dim must be <= 16")
    refused(forward(_pol(_abi, L, obs_dim=4097)), "obs_dim must be <= 4096")
    for name in ("n_pi", "n_vf"):
        for bad in (0, 4, -1):
            refused(forward(_pol(_abi, L, **{name: bad})), name + " must be in [1, 3]")
    for name, count in (("pi_width", "n_pi"), ("vf_width", "n_vf")):
        for bad in ((64, 24), (8, 64), (272, 64), (64, 0), (-16, 64)):
            which = 0 if bad[0] != 64 else 1
            refused(forward(_pol(_abi, L, **{name: _arr(bad)})), f"{name}[{which}] must be a multiple of 16")
        refused(forward(_pol(_abi, L, **{name: _arr((64, 64, 20)), count: 3})), f"{name}[2]")
        refused(forward(_pol(_abi, L, **{name: _arr((64, 20, 7)), count: 1}), o=None), "null mcg_step_out")      # entries past n are not read
    for bad in (2, -1):
        refused(forward(_pol(_abi, L, activation=bad)), "activation")
    good = _pol(_abi, L)
    for bad in (good.blob_floats - 1, good.blob_floats + 16, 0):
        refused(forward(_pol(_abi, L, blob_floats=bad)), "blob_floats")
    refused(forward(_pol(_abi, L, blob=C.c_void_p(0x1008))), "blob is not 16-byte aligned")
    refused(forward(good, o=None), "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal"):
        o = _abi.McgStepOut(**{n: (None if n == name else p) for n in ("obs", "achieved_goal", "desired_goal")})
        refused(forward(good, o=o), "are required")
    refused(forward(good, q=None), "null mcg_policy_out")
    refused(forward(good, q=_abi.McgPolicyOut()), "all outputs are null")


def test_blob_floats_is_zero_for_refused_shapes_and_adds_up_otherwise(built):
    from mycobotgym_amd import _abi
    f = _abi.load().mcg_policy_blob_floats
    ok = f(25, 7, 2, _arr((64, 64)), 2, _arr((64, 64)))
    # by hand: first layers 4 tiles x 8 k-blocks x 64 + 64, second 4 x 16 x 64 + 64, heads 1 x 16 x 64 + 16, twice; log_std 16
    assert ok == 2 * ((4 * 8 * 64 + 64) + (4 * 16 * 64 + 64) + (16 * 64 + 16)) + 16
    assert f(10, 7, 1, _arr((16,)), 1, _arr((16,))) == 2 * ((4 * 64 + 16) + (4 * 64 + 16)) + 16
    for args in ((0, 7, 2, _arr((64, 64)), 2, _arr((64, 64))), (25, 0, 2, _arr((64, 64)), 2, _arr((64, 64))),
                 (-1, -1, 2, _arr((64, 64)), 2, _arr((64, 64))), (25, 17, 2, _arr((64, 64)), 2, _arr((64, 64))),
                 (25, 7, 0, _arr((64, 64)), 2, _arr((64, 64))), (25, 7, 2, _arr((64, 64)), 4, _arr((64, 64))),
                 (25, 7, 2, _arr((64, 40)), 2, _arr((64, 64))), (25, 7, 2, _arr((64, 64)), 2, _arr((512, 64))),
                 (25, 7, 2, None, 2, _arr((64, 64)))):
        assert f(*args) == 0, args


def test_philox_restatement_agrees_with_another_on_common_counters():
    from tests.indep_scene_rand import philox4x32_10 as other
    from tests.indep_rollout import philox_word0
    rng = np.random.default_rng(1)
    cases = [([0, 0, 0, 0], [0, 0]), ([MASK := 0xFFFFFFFF] * 4, [MASK, MASK])] + [
        (rng.integers(0, 2 ** 32, 4).tolist(), rng.integers(0, 2 ** 32, 2).tolist()) for _ in range(50)]
    for ctr, key in cases:
        assert ip.philox4x32_10(ctr, key) == other(ctr, key)
        assert ip.philox4x32_10(ctr, key)[0] == philox_word0(ctr, key)
    # Random123's known answer for the all-ones counter and key
    assert ip.philox4x32_10([0xFFFFFFFF] * 4, [0xFFFFFFFF] * 2) == [0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD]


def test_counter_layout():
    """The four words: the global id and the call split low / high, the pair, the domain word 6, which no other layout uses."""
    assert ip.counter(5, 9, 3) == [5, 9, 3, 6]
    assert ip.counter(2 ** 32 + 5, 2 ** 32 * 7 + 9, 3) == [5, 9, 3 ^ (7 << 8), 6 ^ (1 << 8)]
    from tests import indep_her, indep_replay_img, indep_rollout, indep_scene_rand
    assert sorted({indep_scene_rand.STREAM, indep_her.STREAM, indep_rollout.STREAM, indep_replay_img.STREAM}) == [2, 3, 4, 5]
    assert ip.DOMAIN not in (0, 1, 2, 3, 4, 5)
    assert ip.block(1, 3, 0, 0) != ip.block(1, 0, 3, 0) != ip.block(1, 0, 0, 3)


def test_restated_noise_is_standard_normal_and_blocks_are_distinct():
    """40 environments x 8 components x 64 calls, n = 20480: the mean within 4 / sqrt(n) of 0, the variance within 4 sqrt(2 / n) of 1,
    no two (environment, call, pair) blocks equal."""
    N, A, calls, seed = 40, 8, 64, 0
    eps = np.stack([ip.noise64(seed, c, N, A) for c in range(calls)])
    n = eps.size
    assert n == 20480
    print(f"noise: mean {eps.mean():+.5f} (bound {4 / math.sqrt(n):.5f}), variance {eps.var():.5f} (1 +- {4 * math.sqrt(2 / n):.5f})")
    assert abs(eps.mean()) <= 4 / math.sqrt(n)
    assert abs(eps.var() - 1.0) <= 4 * math.sqrt(2.0 / n)
    blocks = {tuple(ip.block(seed, e, c, p)) for e in range(N) for c in range(calls) for p in range(A // 2)}
    assert len(blocks) == N * calls * (A // 2)
    # an odd A uses the first component of its last pair; the global id is what counts, not the row
    assert np.array_equal(ip.noise(seed, 3, 40, 7), ip.noise(seed, 3, 40, 8)[:, :7])
    assert np.array_equal(ip.noise(seed, 3, 16, 8, env_id_offset=24), ip.noise(seed, 3, 40, 8)[24:])


def test_python_side_refusals_need_no_gpu():
    from mycobotgym_amd import policy
    with pytest.raises(ValueError, match="shared layers"):
        policy._refuse_foreign(["mlp_extractor.shared_net.0.weight"])
    with pytest.raises(ValueError, match="CNN"):
        policy._refuse_foreign(["features_extractor.cnn.0.weight"])

    class Sde(torch.nn.Module):
        use_sde = True

    class Squash(torch.nn.Module):
        squash_output = True
    with pytest.raises(ValueError, match="gSDE"):
        policy.ActorCritic.from_module(Sde())
    with pytest.raises(ValueError, match="squash_output"):
        policy.ActorCritic.from_module(Squash())
    sd = ip.Twin(10, 7).state_dict()
    sd["log_std"] = torch.zeros(64, 7)          # gSDE's log_std is a matrix
    with pytest.raises(ValueError, match="log_std"):
        policy.pack(sd, 10, 7, (64, 64), (64, 64))
