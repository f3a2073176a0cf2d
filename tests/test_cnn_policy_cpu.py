"""The CNN actor-critic policy without a GPU: the restated rule against its torch twin, the blob's packing, the ABI's layout, the
counter words and every host refusal (tests/indep_cnn.py restates the rule; mycobotgym_amd/cnn_policy.py is the code under test)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import indep_cnn as ic
from tests import indep_policy as ip

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPU = torch.device("cpu")


def no_device():
    """``CnnActorCritic`` whose constructor resolves its dimensions without a GPU: it gets as far as its own refusals, and past them
    keeps its blob on the CPU (no kernel is ever launched on it)."""
    from mycobotgym_amd import _abi
    from mycobotgym_amd.cnn_policy import CnnActorCritic

    class NoDevice(CnnActorCritic):
        def _resolve(self, envs, device, given):
            self.device, self._lib = CPU, _abi.load()
            return [given[k] for k, _ in self._FROM_ENVS]
    NoDevice.__name__ = CnnActorCritic.__name__
    return lambda **kw: NoDevice(**{**dict(num_envs=4, channels=1, image_size=36, act_dim=3, features_dim=16), **kw})


# ------------------------------------------------------------------------------------------------------------ the rule
@pytest.mark.parametrize("C_,S,F,A", ic.CASES + ((2, 42, 16, 3),))
def test_twin_in_float64_is_the_restated_rule(C_, S, F, A):
    """The twin cast to float64 == the numpy rule to 1e-12 relative, on random weights with non-zero biases and random bytes, for the
    features, the mean, the value, the sampled action, its log-prob and the entropy.  S = 40, 42 and 44: where the floor drops rows and
    columns, and where it drops none."""
    n = 5
    twin = ic.Twin(C_, S, F, A).randomize(3).double()
    sd = twin.numpy_state()
    assert all(np.abs(v).min() > 0 for k, v in sd.items() if k.endswith(".bias") or k == "log_std")
    img = ic.random_pictures(n, C_, S, seed=5)
    eps = ic.noise64(9, 2, n, A)
    x = ic.preprocess(img)
    with torch.no_grad():
        a, v, lp, m, f = (t.numpy() for t in twin(torch.from_numpy(x), noise=torch.from_numpy(eps)))
        _, lp_e, ent = (t.numpy() for t in twin.evaluate_actions(torch.from_numpy(x), torch.from_numpy(a)))
    f64, mean, value = ic.rule(sd, x)
    rel = lambda got, want: np.abs(got - want).max() / max(1.0, np.abs(want).max())
    assert f64.shape == (n, F) and mean.shape == (n, A) and value.shape == (n,)
    assert rel(f, f64) <= 1e-12 and rel(m, mean) <= 1e-12 and rel(v, value) <= 1e-12
    assert rel(a, ic.sample(mean, sd["log_std"], eps)) <= 1e-12
    assert rel(lp, ic.log_prob(a, mean, sd["log_std"])) <= 1e-12 and rel(lp_e, lp) <= 1e-12
    assert rel(lp, (-0.5 * eps ** 2 - sd["log_std"] - ic.LOG_SQRT_2PI).sum(-1)) <= 1e-12      # the form the forward kernel evaluates
    assert rel(ent, ic.entropy(sd["log_std"])) <= 1e-12
    # the twin's uint8 path is x = float32(byte) / 255
    assert np.array_equal(twin.float()._x(torch.from_numpy(img)).numpy().astype(np.float64), x)


def test_sizes_and_flatten_order():
    assert ic.sizes(64) == (15, 6, 4) and 64 * 4 * 4 == 1024
    assert ic.sizes(36) == (8, 3, 1) and ic.sizes(35)[2] == 0             # 36 is the smallest S with o3 >= 1
    assert ic.sizes(40) == (9, 3, 1) and ic.sizes(44) == (10, 4, 2) and ic.sizes(96) == (23, 10, 8)
    from mycobotgym_amd.cnn_policy import conv_sizes
    for S in range(36, 97):
        assert conv_sizes(S) == ic.sizes(S)
        assert ic.conv(np.zeros((1, 1, S, S)), np.zeros((1, 1, 8, 8)), np.zeros(1), 4).shape[2] == ic.sizes(S)[0]
    # a one-hot feature map flattens to c o3^2 + y o3 + x
    x = np.zeros((1, 64, 2, 2)); x[0, 5, 1, 0] = 1.0
    assert x.reshape(1, -1).argmax() == 5 * 4 + 1 * 2 + 0


# ------------------------------------------------------------------------------------------------------------ the blob
@pytest.mark.parametrize("C_,S,F,A", ic.CASES)
def test_pack_unpack_round_trip_bit_for_bit(built, C_, S, F, A):
    from mycobotgym_amd import _abi, cnn_policy
    L = _abi.load()
    sd = ic.Twin(C_, S, F, A).randomize(11).state_dict()
    blob = cnn_policy.pack(sd, C_, S, F, A)
    assert blob.dtype == torch.float32 and blob.numel() == L.mcg_cnn_blob_floats(C_, S, F, A) == cnn_policy.blob_floats(C_, S, F, A)
    for rows in (1, 33, 8192):
        assert L.mcg_cnn_scratch_floats(C_, S, F, A, rows) == cnn_policy.scratch_floats(S, rows) == rows * 64 * ic.sizes(S)[2] ** 2
    back = cnn_policy.unpack(blob, C_, S, F, A)
    assert set(back) == set(sd) == set(cnn_policy.state_names())
    for k, v in sd.items():
        assert back[k].shape == v.shape and back[k].numpy().tobytes() == v.detach().numpy().tobytes(), k
    plain = {k: v for k, v in sd.items() if not k.startswith(("pi_", "vf_"))}
    assert set(cnn_policy.unpack(blob, C_, S, F, A, aliases=False)) == set(plain) == set(cnn_policy.state_names(aliases=False))
    # every weight sits in the blob exactly once, and the padding is zeros
    assert int((blob != 0).sum()) == sum(int((v != 0).sum()) for v in plain.values())
    # every piece starts at a multiple of 16 floats
    at = 0
    for _m, out, k, _first in cnn_policy.blob_shapes(C_, S, F, A):
        out_p = -(-out // 16) * 16
        for piece in ((16,) if k is None else (out_p * k, out_p)):
            assert at % 16 == 0 and piece % 16 == 0, (_m, at, piece)
            at += piece
    assert at == blob.numel()


def test_sizes_are_zero_for_refused_shapes(built):
    from mycobotgym_amd import _abi, cnn_policy
    L = _abi.load()
    good = (1, 64, 512, 7)
    assert L.mcg_cnn_blob_floats(*good) == 32 * 65 + 64 * 513 + 64 * 577 + 512 * 1025 + 2 * 16 * 513 + 16
    for bad in ((0, 64, 512, 7), (17, 64, 512, 7), (1, 35, 512, 7), (1, 97, 512, 7), (1, 64, 0, 7), (1, 64, 24, 7), (1, 64, 528, 7),
                (1, 64, 512, 0), (1, 64, 512, 17), (-1, -1, -1, -1)):
        assert L.mcg_cnn_blob_floats(*bad) == 0 and L.mcg_cnn_scratch_floats(*bad, 8) == 0 and not cnn_policy.accepted(*bad), bad
    for edge in ((1, 36, 16, 1), (16, 96, 512, 16)):
        assert L.mcg_cnn_blob_floats(*edge) == cnn_policy.blob_floats(*edge) > 0 and cnn_policy.accepted(*edge)
    for rows in (0, -1, 2 ** 27):
        assert L.mcg_cnn_scratch_floats(*good, rows) == 0
    assert L.mcg_cnn_scratch_floats(*good, 2 ** 27 - 1) == (2 ** 27 - 1) * 1024


# ------------------------------------------------------------------------------------------------------------- the ABI
def test_cnn_structs_match_header_layout(built, tmp_path):
    from mycobotgym_amd import _abi
    structs = (("mcg_cnn_policy", _abi.McgCnnPolicy), ("mcg_cnn_obs", _abi.McgCnnObs), ("mcg_cnn_out", _abi.McgCnnOut))
    exprs = ["MCG_CNN_UINT8", "MCG_CNN_FLOAT32"]
    want = [_abi.CNN_UINT8, _abi.CNN_FLOAT32]
    for name, cls in structs:
        exprs.append(f"sizeof({name})"); want.append(C.sizeof(cls))
        for field, _ in cls._fields_:
            exprs.append(f"offsetof({name},{field})"); want.append(getattr(cls, field).offset)
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    assert got == want
    assert [n for n, _ in _abi.McgCnnOut._fields_] == ["action", "value", "log_prob", "mean", "noise", "features"]
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays
    for name in ("mcg_cnn_blob_floats", "mcg_cnn_scratch_floats", "mcg_cnn_forward", "mcg_cnn_evaluate"):
        assert name in _abi.EXPORTS and hasattr(_abi.load(), name), name
    import mycobotgym_amd
    assert mycobotgym_amd.CnnActorCritic is mycobotgym_amd.cnn_policy.CnnActorCritic


def test_c_side_refusals_without_a_gpu(built):
    """Every argument check of mcg_cnn_forward and mcg_cnn_evaluate: the code and a fragment of its message that names the field (the
    pointers are never dereferenced: the refusals come before any HIP call)."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = 0x1000
    ref = lambda x: None if x is None else C.byref(x)

    def pol(**over):
        kw = dict(blob=p, scratch=p, n_envs=33, channels=1, image_size=64, features_dim=512, act_dim=7)
        kw.update(over)
        shape = (kw["channels"], kw["image_size"], kw["features_dim"], kw["act_dim"])
        kw.setdefault("blob_floats", L.mcg_cnn_blob_floats(*shape))
        kw.setdefault("scratch_floats", L.mcg_cnn_scratch_floats(*shape, max(kw["n_envs"], 1)))
        return _abi.McgCnnPolicy(**kw)

    obs = lambda **over: _abi.McgCnnObs(**{**dict(pixels=p, dtype=_abi.CNN_UINT8, env_stride=4096, chan_stride=4096), **over})
    out = _abi.McgCnnOut(action=p, value=p, log_prob=p)
    ev = _abi.McgPolicyEvalOut(value=p, log_prob=p, entropy=p)
    forward = lambda P, o=obs(), q=out: L.mcg_cnn_forward(ref(P), ref(o), 0, 0, 0, 0, ref(q), None)
    evaluate = lambda P, o=obs(), a=p, rows=5, q=ev: L.mcg_cnn_evaluate(ref(P), ref(o), a, rows, ref(q), None)

    def refused(code, text):
        assert code == _abi.MCG_ERR_ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    for call in (forward, evaluate):
        refused(call(None), "null mcg_cnn_policy")
        refused(call(pol(blob=None)), "blob is null")
        refused(call(pol(scratch=None)), "scratch is null")
        for bad in (0, 17):
            refused(call(pol(channels=bad)), "channels must be in [1, 16]")
            refused(call(pol(act_dim=bad)), "act_dim must be in [1, 16]")
        for bad in (35, 97):
            refused(call(pol(image_size=bad)), "image_size must be in [36, 96]")
        for bad in (0, 8, 40, 528):
            refused(call(pol(features_dim=bad)), "features_dim must be a multiple of 16 in [16, 512]")
        good = pol()
        for bad in (good.blob_floats - 1, good.blob_floats + 16, 0):
            refused(call(pol(blob_floats=bad)), "blob_floats")
        refused(call(pol(scratch_floats=5 * 1024 - 1)), "scratch_floats")
        refused(call(pol(blob=p + 8)), "blob is not 16-byte aligned")
        refused(call(pol(scratch=p + 4)), "scratch is not 16-byte aligned")
        refused(call(good, None), "null mcg_cnn_obs")
        refused(call(good, obs(pixels=None)), "pixels is null")
        refused(call(good, obs(dtype=2)), "dtype")
        refused(call(good, obs(env_stride=-1)), "env_stride")
        refused(call(pol(channels=2), obs(chan_stride=4095)), "chan_stride must be >= image_size^2")
    refused(forward(pol(n_envs=0)), "must be >= 1")
    refused(forward(pol(n_envs=2 ** 27, scratch_floats=2 ** 40)), "below 2^27")
    refused(forward(pol(), q=None), "null mcg_cnn_out")
    refused(forward(pol(), q=_abi.McgCnnOut()), "all outputs are null")
    refused(evaluate(pol(), rows=0), "must be >= 1")
    refused(evaluate(pol(), rows=34), "scratch_floats")                          # the scratch is the caller's to size for the rows
    refused(evaluate(pol(), q=None), "null mcg_policy_eval_out")
    refused(evaluate(pol(), q=_abi.McgPolicyEvalOut()), "all outputs are null")
    refused(evaluate(pol(), a=None), "actions is null")


# ----------------------------------------------------------------------------------------------------------- the noise
def test_counter_words_with_domain_12():
    assert ic.DOMAIN == 12 and ip.DOMAIN == 6
    assert ic.counter(5, 9, 3) == [5, 9, 3, 12]
    assert ic.counter(2 ** 32 + 5, 2 ** 32 * 7 + 9, 3) == [5, 9, 3 ^ (7 << 8), 12 ^ (1 << 8)]
    from tests import indep_her, indep_replay_img, indep_rollout, indep_scene_rand
    taken = {0, 1, indep_scene_rand.STREAM, indep_her.STREAM, indep_rollout.STREAM, indep_replay_img.STREAM, ip.DOMAIN, 7, 8, 9, 10, 11}
    assert taken == set(range(12)) and ic.DOMAIN not in taken
    for seed, gid, call, pair in ((1, 3, 0, 0), (21, 32, 7, 6), (2 ** 63 + 1, 2 ** 40, 2 ** 33, 1)):
        assert ic.counter(gid, call, pair)[:3] == ip.counter(gid, call, pair)[:3] and ic.counter(gid, call, pair)[3] != ip.counter(gid, call, pair)[3]
        assert ic.block(seed, gid, call, pair) != ip.block(seed, gid, call, pair)      # ActorCritic's block for equal (seed, gid, call, pair)
    assert not np.array_equal(ic.noise(21, 0, 8, 7), ip.noise(21, 0, 8, 7))
    # the global id is what counts, not the row; an odd A uses the first component of its last pair
    assert np.array_equal(ic.noise(0, 3, 16, 8, env_id_offset=24), ic.noise(0, 3, 40, 8)[24:])
    assert np.array_equal(ic.noise(0, 3, 4, 8, ids=[7, 2, 39, 0]), ic.noise(0, 3, 40, 8)[[7, 2, 39, 0]])
    assert np.array_equal(ic.noise(0, 3, 40, 7), ic.noise(0, 3, 40, 8)[:, :7])


# ------------------------------------------------------------------------------------------------------- the refusals
def test_shape_refusals(built):
    make_pol = no_device()
    for bad in (dict(channels=0), dict(channels=17), dict(image_size=35), dict(image_size=97), dict(features_dim=8), dict(features_dim=24),
                dict(features_dim=528), dict(act_dim=0), dict(act_dim=17), dict(num_envs=0)):
        with pytest.raises(ValueError, match=r"unsupported shape: .*channels 1\.\.16, image_size 36\.\.96, features_dim a multiple of 16 in "
                                             r"16\.\.512, act_dim 1\.\.16"):
            make_pol(**bad)
    from mycobotgym_amd.cnn_policy import CnnActorCritic
    with pytest.raises(ValueError, match="CnnActorCritic needs envs= or num_envs, channels, image_size, act_dim"):
        CnnActorCritic()
    pol = make_pol(channels=16, image_size=96, features_dim=512, act_dim=16)
    assert pol.blob_floats == pol._blob.numel() and (pol.seed, pol.calls, pol.env_id_offset) == (0, 0, 0)


def test_state_environments_are_refused():
    from mycobotgym_amd import MyCobotVecEnv
    from mycobotgym_amd.cnn_policy import CnnActorCritic
    envs = MyCobotVecEnv.__new__(MyCobotVecEnv)                               # a -v0 state environment (no constructor call: no device)
    envs._closed = True
    with pytest.raises(ValueError, match="the -v0 ids observe float64 states .* CnnActorCritic is the CNN policy of the -v1 picture ids"):
        CnnActorCritic(envs)


def test_foreign_state_dicts_and_modules_are_refused(built):
    from mycobotgym_amd.cnn_policy import CnnActorCritic
    C_, S, F, A = 1, 36, 16, 3
    pol = no_device()()
    twin = ic.Twin(C_, S, F, A).randomize(3)
    sd = twin.state_dict()
    pol.load_state_dict(sd)                                                   # SB3 >= 1.8's keys, aliases included
    pol.load_state_dict({k: v for k, v in sd.items() if not k.startswith(("pi_", "vf_"))})      # and SB3 < 1.8's, without them
    got = pol.state_dict()
    assert all(torch.equal(got[k], v) for k, v in sd.items()) and set(got) == set(sd) | {"seed", "calls"}
    with pytest.raises(ValueError, match=r"a non-empty net_arch \(mlp_extractor\.\* layers\) is not supported"):
        pol.load_state_dict(dict(sd, **{"mlp_extractor.policy_net.0.weight": torch.zeros(64, F), "mlp_extractor.policy_net.0.bias": torch.zeros(64)}))
    other = dict(sd)
    other["vf_features_extractor.cnn.2.bias"] = sd["vf_features_extractor.cnn.2.bias"] + 1.0
    with pytest.raises(ValueError, match="share_features_extractor=False is not supported: vf_features_extractor.cnn.2.bias differs"):
        pol.load_state_dict(other)
    with pytest.raises(ValueError, match="share_features_extractor=False is not supported: pi_features_extractor.linear.0.weight differs"):
        pol.load_state_dict(dict(sd, **{"pi_features_extractor.linear.0.weight": torch.zeros(F, 64)}))
    with pytest.raises(ValueError, match="does not fit CnnPolicy with net_arch=\\[\\]: missing \\['value_net.bias'\\]"):
        pol.load_state_dict({k: v for k, v in sd.items() if k != "value_net.bias"})
    with pytest.raises(ValueError, match=r"features_extractor.cnn.0: expected weight \(32, 1, 8, 8\)"):
        pol.load_state_dict(ic.Twin(2, S, F, A).state_dict())
    with pytest.raises(ValueError, match="log_std: expected shape .* gSDE"):
        pol.load_state_dict(dict(sd, log_std=torch.zeros(F, A)))                # gSDE's log_std is a matrix

    class Sde(torch.nn.Module):
        use_sde = True

    class Squash(torch.nn.Module):
        squash_output = True

    class Separate(torch.nn.Module):
        share_features_extractor = False
    with pytest.raises(ValueError, match="gSDE"):
        CnnActorCritic.from_module(Sde())
    with pytest.raises(ValueError, match="squash_output"):
        CnnActorCritic.from_module(Squash())
    with pytest.raises(ValueError, match="share_features_extractor=False"):
        CnnActorCritic.from_module(Separate())
    with pytest.raises(ValueError, match="no features_extractor.linear.0 layer"):
        CnnActorCritic.from_module(torch.nn.Linear(3, 3))
    with pytest.raises(ValueError, match="a non-empty net_arch"):
        CnnActorCritic.from_module(ip.Twin(10, 7))                             # the MLP policy's module


def test_wrong_pictures_are_refused():
    """The dtype, the shape and the device of the pictures, and evaluate_actions' arguments: each by its message, before any launch."""
    pol = no_device()()
    good = torch.zeros(4, 1, 36, 36, dtype=torch.uint8)
    for call in (pol.forward, pol.values):
        with pytest.raises(ValueError, match="img: expected torch.uint8 pictures, got torch.float32"):
            call(good.float())
        with pytest.raises(ValueError, match=r"img: expected shape \(4, 1, 36, 36\), got \(4, 1, 36, 35\)"):
            call(good[..., :35])
        with pytest.raises(ValueError, match=r"img: expected shape \(4, 1, 36, 36\), got \(3, 1, 36, 36\)"):
            call(good[:3])
        with pytest.raises(ValueError, match="img: expected a device tensor"):
            call({"observation": good})
        with pytest.raises(ValueError, match="img lives on meta, the policy on cpu"):
            call(good.to("meta"))
    acts = torch.zeros(5, 3)
    pics = torch.zeros(5, 1, 36, 36)
    with pytest.raises(ValueError, match="observations: expected torch.uint8 or torch.float32 pictures, got torch.float64"):
        pol.evaluate_actions(pics.double(), acts)
    with pytest.raises(ValueError, match=r"observations: expected shape \(5, 1, 36, 36\), got \(4, 1, 36, 36\)"):
        pol.evaluate_actions(pics[:4], acts)
    with pytest.raises(ValueError, match="the dict of a -v0 state id is not supported"):
        pol.evaluate_actions({"observation": pics}, acts)
    with pytest.raises(ValueError, match=r"actions: expected a float32 tensor \[B, 3\]"):
        pol.evaluate_actions(pics, torch.zeros(5, 4))
    with pytest.raises(ValueError, match=r"actions: expected a float32 tensor \[B, 3\], got torch.float64"):
        pol.evaluate_actions(pics, acts.double())
    with pytest.raises(ValueError, match="the minibatch is empty"):
        pol.evaluate_actions(pics[:0], acts[:0])
    with pytest.raises(ValueError, match="out: unknown"):
        pol.forward(good, out={"value": torch.zeros(4), "entropy": torch.zeros(4)})
    with pytest.raises(ValueError, match=r"out\['features'\]: expected a contiguous float32 tensor \(4, 16\)"):
        pol.forward(good, out={"features": torch.zeros(4, 32)})
    assert pol.calls == 0


def test_the_mlp_policies_keep_refusing_the_picture_ids():
    from mycobotgym_amd import ActorCritic, SACPolicy, TD3Policy
    for cls in (ActorCritic, SACPolicy, TD3Policy):
        assert "not supported" in cls._NO_IMAGES and "CNN" in cls._NO_IMAGES
