"""The CNN actor-critic forward on the GPU (mycobotgym_amd/cnn_policy.py, csrc/mcg_cnn.hip) against the restated rule and its torch
twin (tests/indep_cnn.py).  N = 33 is two full tiles of 16 rows and one ragged row (and, for the convolution kernel's groups of
four, three or one pictures, a ragged last group).

Bound of the parity tests, per case and per output: 10 x the largest error of the twin's CPU float32 forward against the float64 rule
on the same float32 value of byte / 255, the maximum over the case's rows (the project's "10 x a twin" margin: it covers another order
of summation).  The measured ratios are in profiles/cnn_policy/parity.md."""
import functools

import numpy as np
import pytest
import torch

from tests import indep_cnn as ic

pytestmark = pytest.mark.gpu

N, SEED = 33, 21
CASES = list(ic.CASES)
NAMES = ("action", "value", "log_prob", "mean", "noise", "features")
ENV_ID = "MyCobotReach-Sparse-joint-v1"


def policy_for(C, S, F, A, weights_seed=3, n=N, **kw):
    from mycobotgym_amd import CnnActorCritic
    twin = ic.Twin(C, S, F, A).randomize(weights_seed)
    pol = CnnActorCritic(num_envs=n, channels=C, image_size=S, act_dim=A, features_dim=F, seed=SEED, **kw)
    pol.load_state_dict(twin.state_dict())
    return pol, twin


def dev(img):
    return img if torch.is_tensor(img) else torch.from_numpy(np.ascontiguousarray(img)).cuda()


def run(pol, img, deterministic=False) -> dict:
    """All six outputs of one call as numpy arrays."""
    out = pol._new(*NAMES)
    pol.forward(dev(img), deterministic=deterministic, out=out)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def same_bits(a: dict, b: dict, rows=slice(None), names=NAMES):
    for k in names:
        assert np.array_equal(bits(a[k]), bits(b[k][rows])), k


def yardstick(twin, img, eps, what):
    """The float64 rule on the pictures ``img`` (uint8 numpy), the twin's float32 forward with the noise ``eps``, and the twin's errors."""
    sd = twin.numpy_state()
    f64, mean64, value64 = ic.rule(sd, ic.preprocess(img))
    with torch.no_grad():
        a, v, lp, m, f = (x.numpy() for x in twin(torch.from_numpy(img), noise=torch.from_numpy(eps)))
    err = {"features": np.abs(f - f64).max(), "mean": np.abs(m - mean64).max(), "value": np.abs(v - value64).max(),
           "log_prob": np.abs(lp - ic.log_prob(a, mean64, sd["log_std"])).max()}
    assert all(e > 0 for e in err.values()), (what, err)
    return {"img": img, "sd": sd, "features64": f64, "mean64": mean64, "value64": value64, "eps": eps, "twin_err": err}


@functools.lru_cache(maxsize=None)
def reference(C, S, F, A, weights_seed=3, call=0, n=N):
    """Computed once per case and shared: random bytes, the float64 rule on them, the twin's float32 forward with the restated noise
    of call `call`, and the twin's errors, which are the bounds' yardstick."""
    twin = ic.Twin(C, S, F, A).randomize(weights_seed)
    return yardstick(twin, ic.random_pictures(n, C, S, seed=5), ic.noise(SEED, call, n, A), (C, S, F, A))


def kernel_errors(got: dict, ref: dict) -> dict:
    return {"features": np.abs(got["features"] - ref["features64"]).max(), "mean": np.abs(got["mean"] - ref["mean64"]).max(),
            "value": np.abs(got["value"] - ref["value64"]).max(),
            "log_prob": np.abs(got["log_prob"] - ic.log_prob(got["action"], ref["mean64"], ref["sd"]["log_std"])).max()}


def assert_parity(got, ref, what, names=("features", "mean", "value", "log_prob")):
    err = kernel_errors(got, ref)
    for k in names:
        print(f"parity {what} {k}: kernel {err[k]:.3e}, twin {ref['twin_err'][k]:.3e}, ratio {err[k] / ref['twin_err'][k]:.2f}")
    for k in names:
        assert err[k] <= 10.0 * ref["twin_err"][k], (what, k, err[k], ref["twin_err"][k])


# ---------------------------------------------------------------------------------------------------------- 1. parity
@pytest.mark.parametrize("C,S,F,A", CASES)
def test_parity_with_the_float64_rule_on_random_bytes(built, C, S, F, A):
    """features, mean, value and log_prob against the float64 rule on the float32 value of byte / 255; log_prob is judged on the
    kernel's own action: the float64 formula at (kernel action, float64 mean, log_std)."""
    pol, _ = policy_for(C, S, F, A)
    ref = reference(C, S, F, A)
    got = run(pol, ref["img"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert_parity(got, ref, f"C={C} S={S} F={F} A={A}")


@pytest.mark.parametrize("C,S,F,A", [(1, 96, 16, 1), (16, 96, 512, 16)])
def test_parity_at_the_largest_picture(built, C, S, F, A):
    """S = 96, the end of the accepted domain: from S = 84 on one picture's activations take more than 64 KB of LDS, which the
    convolution kernel asks for by its own path.  Five pictures: a ragged tile, and five workgroups of one picture."""
    pol, _ = policy_for(C, S, F, A, n=5)
    ref = reference(C, S, F, A, n=5)
    got = run(pol, ref["img"])
    assert all(np.isfinite(v).all() for v in got.values())
    assert_parity(got, ref, f"C={C} S={S} F={F} A={A}")
    assert np.array_equal(bits(got["noise"]), bits(ref["eps"]))


def test_parity_on_real_renders(built):
    from mycobotgym_amd import CnnActorCritic, make
    envs = make(ENV_ID, num_envs=17)
    img, _ = envs.reset(seed=3)
    for _ in range(2):
        img = envs.step(torch.zeros(17, envs.action_dim, device="cuda"))[0]
    C, S, A = envs.channels, envs.image_size, envs.action_dim
    assert (C, S) == (1, 64) and (img.stride(0), img.stride(1)) == (S * S, 17 * S * S)      # the [N, C, S, S] view of [C, N, S, S] planes
    twin = ic.Twin(C, S, 512, A).randomize(3)
    pol = CnnActorCritic.from_module(twin, envs, seed=SEED)
    pictures = img.cpu().numpy()
    assert pictures.std() > 1.0                                               # a picture of something
    ref = yardstick(twin, pictures, ic.noise(SEED, 0, 17, A), "renders")
    got = run(pol, img)
    assert_parity(got, ref, "renders")
    envs.close()


# ------------------------------------------------------------------------------------------------- 2. window geometry
def _last_read(S):
    """The last row and column of the picture that conv1 reads, and the first that the floors of conv1 and conv2 together drop."""
    o1, o2, _ = ic.sizes(S)
    return 4 * (o1 - 1) + 7, 4 * (2 * (o2 - 1) + 4 - 1) + 8


@pytest.mark.parametrize("C,S,F,A", [c for c in CASES if c[0] <= 3] + [(2, 42, 16, 3)])
def test_window_geometry(built, C, S, F, A):
    """All-zero pictures with one byte set: at (0, 0), at (S - 1, S - 1), at the last row and column conv1 still reads; a fourth stays
    all zero.  Then, where the floors drop rows and columns (S = 40 and S = 64: conv2's floor drops conv1's last row and column, and so
    the picture's last four; S = 42: conv1's drops two more; S = 36 and S = 44: none, the check is empty there), changing only the
    dropped bytes leaves every output bit-identical."""
    last, first_dropped = _last_read(S)
    assert last <= S - 1 and first_dropped <= S
    assert {36: (35, 36), 40: (39, 36), 42: (39, 36), 44: (43, 44), 64: (63, 60)}[S] == (last, first_dropped)
    img = np.zeros((4, C, S, S), np.uint8)
    img[0, 0, 0, 0], img[1, C - 1, S - 1, S - 1], img[2, C - 1, last, last] = 255, 201, 77
    pol, twin = policy_for(C, S, F, A, n=4)
    ref = yardstick(twin, img, ic.noise(SEED, 0, 4, A), "one byte set")
    got = run(pol, img)
    assert_parity(got, ref, f"one byte set, S={S}", names=("features",))
    # each set byte is seen: the features differ from the all-zero picture's, unless the byte is one the floors drop
    seen = [np.abs(ref["features64"][row] - ref["features64"][3]).max() for row in range(3)]
    assert seen[0] > 1e-6
    for row, at in ((1, S - 1), (2, last)):
        assert seen[row] > 1e-6 if at < first_dropped else seen[row] < 1e-12, (row, seen)
        assert np.array_equal(bits(got["features"][row]), bits(got["features"][3])) == (at >= first_dropped)
    full = ic.random_pictures(4, C, S, seed=8)
    changed = full.copy()
    changed[:, :, first_dropped:, :] ^= 0xA5
    changed[:, :, :first_dropped, first_dropped:] ^= 0x5A
    assert bool((changed != full).any()) == (first_dropped < S)
    pol.calls = 0
    a = run(pol, full)
    pol.calls = 0
    same_bits(run(pol, changed), a)
    f_full, f_changed = ic.rule(ref["sd"], ic.preprocess(full))[0], ic.rule(ref["sd"], ic.preprocess(changed))[0]
    assert np.array_equal(f_full, f_changed)                                 # the rule agrees that those bytes are dropped


# ----------------------------------------------------------------------------------------------------------- 3. noise
@pytest.mark.parametrize("C,S,F,A", [(1, 64, 512, 7), (3, 40, 48, 13), (2, 44, 512, 16)])
def test_noise_action_and_deterministic(built, C, S, F, A):
    pol, _ = policy_for(C, S, F, A)
    ref = reference(C, S, F, A)
    got = run(pol, ref["img"])
    assert pol.calls == 1
    assert np.array_equal(bits(got["noise"]), bits(ref["eps"]))                # bit for bit, in all A columns
    want = ic.sample(got["mean"], ref["sd"]["log_std"], got["noise"]).astype(np.float32)      # in double, rounded once
    assert np.array_equal(bits(got["action"]), bits(want))
    det = run(pol, ref["img"], deterministic=True)
    assert pol.calls == 1                                                      # not advanced
    assert np.array_equal(bits(det["action"]), bits(det["mean"])) and np.array_equal(bits(det["mean"]), bits(got["mean"]))
    assert not det["noise"].any()
    assert np.array_equal(bits(det["value"]), bits(got["value"])) and np.array_equal(bits(det["features"]), bits(got["features"]))
    second = run(pol, ref["img"])
    assert pol.calls == 2
    assert np.array_equal(bits(second["noise"]), bits(ic.noise(SEED, 1, N, A)))          # the call number is the noise's second word
    assert np.array_equal(bits(second["mean"]), bits(got["mean"]))


# ------------------------------------------------------------------------------------------------- 4. value-only path
def test_values_is_the_full_calls_value(built):
    C, S, F, A = 3, 40, 48, 13
    pol, _ = policy_for(C, S, F, A)
    img = dev(reference(C, S, F, A)["img"])
    full = run(pol, img)
    calls = pol.calls
    v = pol.values(img)
    torch.cuda.synchronize()
    assert v.dtype == torch.float32 and tuple(v.shape) == (N,)
    assert np.array_equal(bits(v.cpu().numpy()), bits(full["value"]))
    assert pol.calls == calls


# ---------------------------------------------------------------------------------------------- 5. row independence
@pytest.mark.parametrize("C,S,F,A", [(1, 64, 512, 7), (3, 40, 48, 13), (2, 44, 512, 16)])
def test_a_row_depends_on_its_picture_and_its_global_id(built, C, S, F, A):
    img = reference(C, S, F, A)["img"]
    whole = run(policy_for(C, S, F, A)[0], img)
    for row in (0, 16, 32):                                                   # N = 1 with a matching env_id_offset
        same_bits(run(policy_for(C, S, F, A, n=1, env_id_offset=row)[0], img[row:row + 1]), whole, slice(row, row + 1))
    same_bits(run(policy_for(C, S, F, A, n=16)[0], img[:16]), whole, slice(0, 16))          # N = 33 against N = 16
    same_bits(run(policy_for(C, S, F, A, n=16, env_id_offset=17)[0], img[17:]), whole, slice(17, 33))
    # a permutation of the batch with the ids following: the noise is keyed by the id, so it is compared through the restatement
    perm = np.random.default_rng(2).permutation(N)
    moved = run(policy_for(C, S, F, A)[0], img[perm])
    same_bits(moved, whole, perm, names=("features", "mean", "value"))
    for row, src in enumerate(perm[:4]):                                      # row `row` now holds picture `src`: its id is `src`
        one = run(policy_for(C, S, F, A, n=1, env_id_offset=int(src))[0], img[src:src + 1])
        same_bits(one, whole, slice(src, src + 1))
        assert np.array_equal(bits(one["mean"][0]), bits(moved["mean"][row]))


# ---------------------------------------------------------------------------------------------------------- 6. layouts
def test_planes_view_and_contiguous_copy_give_equal_bits(built):
    C, S, F, A = 3, 40, 48, 13
    img = reference(C, S, F, A)["img"]
    planes = torch.from_numpy(np.ascontiguousarray(img.transpose(1, 0, 2, 3))).cuda().permute(1, 0, 2, 3)      # [N, C, S, S] of [C, N, S, S]
    assert not planes.is_contiguous() and planes.stride(0) == S * S and planes.stride(1) == N * S * S
    pol, _ = policy_for(C, S, F, A)
    cobs, kept = pol._pictures(planes, "img", N, (torch.uint8,))
    assert kept.data_ptr() == planes.data_ptr() and (cobs.env_stride, cobs.chan_stride) == (S * S, N * S * S)      # read in place
    a = run(pol, planes)
    pol.calls = 0
    b = run(pol, planes.contiguous())
    same_bits(a, b)
    same_bits(a, run(policy_for(C, S, F, A)[0], planes.clone()))              # clone() keeps the planes' layout
    single = torch.from_numpy(img[:, :1].copy()).cuda()                       # C = 1 of the same: both strides describe one layout
    one, _ = policy_for(1, S, F, A)
    same_bits(run(one, single), run(policy_for(1, S, F, A)[0], single.permute(1, 0, 2, 3).contiguous().permute(1, 0, 2, 3)))


# ------------------------------------------------------------------------------------------------ 7. evaluate_actions
@pytest.mark.parametrize("C,S,F,A", [(1, 64, 512, 7), (3, 40, 48, 13)])
def test_evaluate_actions(built, C, S, F, A):
    B = 75
    big, twin = policy_for(C, S, F, A, n=B)
    img = ic.random_pictures(B, C, S, seed=6)
    fwd = run(big, img)
    sd = twin.numpy_state()
    _, mean64, _ = ic.rule(sd, ic.preprocess(img))
    with torch.no_grad():
        _, lp32, ent32 = twin.evaluate_actions(torch.from_numpy(img), torch.from_numpy(fwd["action"]))
    lp64 = ic.log_prob(fwd["action"], mean64, sd["log_std"])
    twin_err = np.abs(lp32.numpy() - lp64).max()
    assert twin_err > 0
    pol, _ = policy_for(C, S, F, A)                                           # num_envs = 33: evaluate_actions takes any B
    ent64 = ic.entropy(sd["log_std"])
    ls = sd["log_std"].astype(np.float64)
    for rows in (1, 33, 75):
        value, log_prob, entropy = pol.evaluate_actions(dev(img[:rows]), dev(fwd["action"][:rows]))
        torch.cuda.synchronize()
        value, log_prob, entropy = value.cpu().numpy(), log_prob.cpu().numpy(), entropy.cpu().numpy()
        assert value.shape == log_prob.shape == entropy.shape == (rows,)
        assert np.array_equal(bits(value), bits(fwd["value"][:rows]))
        gap, err = np.abs(log_prob - fwd["log_prob"][:rows]).max(), np.abs(log_prob - lp64[:rows]).max()
        print(f"evaluate_actions B={rows}: |log_prob - forward's| {gap:.3e}, |log_prob - rule| {err:.3e}, twin {twin_err:.3e}, "
              f"ratios {gap / twin_err:.2f} {err / twin_err:.2f}")
        assert gap <= 10.0 * twin_err and err <= 10.0 * twin_err
        # A terms (1/2 + ln(2 pi) / 2 + log_std), each one float32 addition, summed in float32: at most A + 1 roundings
        assert np.abs(entropy - ent64).max() <= (A + 1) * 2.0 ** -24 * (np.abs(ls) + 0.5 + ic.LOG_SQRT_2PI).sum()
    assert pol.calls == 0


# ---------------------------------------------------------------------------------------------------- 8. stray writes
@pytest.mark.parametrize("n", [1, 17, 33])
def test_no_stray_writes(built, n):
    C, S, F, A, G = 3, 40, 48, 13, 3
    pol, _ = policy_for(C, S, F, A, n=n)
    img = dev(reference(C, S, F, A)["img"][:n])
    shapes = pol._shapes()
    big = {k: torch.full((n + 2 * G,) + shapes[k][1:], -77.25, device="cuda") for k in NAMES}
    K3 = 64 * ic.sizes(S)[2] ** 2
    scratch = torch.full((n + 2 * G, K3), -77.25, device="cuda")              # the policy's scratch, with guard rows around it
    pol._scratch = scratch[G:G + n].reshape(-1)
    pol._cbuf.scratch, pol._cbuf.scratch_floats = pol._scratch.data_ptr(), n * K3
    pol.forward(img, out={k: v[G:G + n] for k, v in big.items()})
    torch.cuda.synchronize()
    plain = run(policy_for(C, S, F, A, n=n)[0], img)
    for k, v in big.items():
        v = v.cpu().numpy()
        assert (v[:G] == -77.25).all() and (v[G + n:] == -77.25).all(), k
        assert np.array_equal(bits(v[G:G + n]), bits(plain[k])), k
    guard = torch.full((n + 2 * G,), -77.25, device="cuda")
    pol.values(img, out=guard[G:G + n])
    ev = {k: torch.full((n + 2 * G,), -77.25, device="cuda") for k in ("value", "log_prob", "entropy")}
    pol.evaluate_actions(img, dev(plain["action"]), out={k: v[G:G + n] for k, v in ev.items()})
    torch.cuda.synchronize()
    for v in (guard, *ev.values()):
        assert (v[:G] == -77.25).all() and (v[G + n:] == -77.25).all() and (v[G:G + n] != -77.25).all()
    assert np.array_equal(bits(guard[G:G + n].cpu().numpy()), bits(plain["value"]))
    s = scratch.cpu().numpy()
    assert (s[:G] == -77.25).all() and (s[G + n:] == -77.25).all() and (s[G:G + n] >= 0).all()      # ReLU outputs inside, nothing outside


# --------------------------------------------------------------------------------------------------------- 9. weights
def test_weights_state_dict_from_module_and_checkpoints(built):
    from mycobotgym_amd import CnnActorCritic
    C, S, F, A = 3, 40, 48, 13
    one, two = reference(C, S, F, A, 3), reference(C, S, F, A, 4)
    pol, twin = policy_for(C, S, F, A, weights_seed=3)
    assert_parity(run(pol, one["img"]), one, "first weights")
    twin4 = ic.Twin(C, S, F, A).randomize(4)
    pol.load_state_dict(twin4.state_dict())
    pol.calls = 0
    got = run(pol, two["img"])
    assert_parity(got, two, "second weights")
    stale = kernel_errors(got, one)
    assert stale["mean"] > 1e3 * one["twin_err"]["mean"] and stale["value"] > 1e3 * one["twin_err"]["value"], stale
    # state_dict() returns the loaded tensors bit for bit, the aliases included
    sd, loaded = pol.state_dict(), twin4.state_dict()
    assert any(k.startswith("pi_features_extractor.") for k in loaded) and any(k.startswith("vf_features_extractor.") for k in loaded)
    assert set(sd) == set(loaded) | {"seed", "calls"}
    for k, v in loaded.items():
        assert sd[k].shape == v.shape and torch.equal(sd[k].cpu(), v), k
    # from_module(twin) equals constructing and then loading
    made = CnnActorCritic.from_module(twin4, num_envs=N, channels=C, image_size=S, act_dim=A, seed=SEED)
    assert made.features_dim == F and torch.equal(made._blob, pol._blob)
    same_bits(run(made, two["img"]), got)
    # a checkpoint of weights, seed and calls continues bit for bit
    run(pol, two["img"])
    ck = pol.state_dict()
    assert ck["seed"] == SEED and ck["calls"] == 2
    fresh = CnnActorCritic(num_envs=N, channels=C, image_size=S, act_dim=A, features_dim=F, seed=999)
    assert not torch.equal(fresh._blob, pol._blob)
    fresh.load_state_dict(ck)
    assert (fresh.seed, fresh.calls) == (SEED, 2) and torch.equal(fresh._blob, pol._blob)
    same_bits(run(fresh, two["img"]), run(pol, two["img"]))
    assert fresh.calls == pol.calls == 3
    # the start: SB3's orthogonal init
    init = CnnActorCritic(num_envs=2, channels=C, image_size=S, act_dim=A, features_dim=F, seed=1).state_dict()
    assert float(init["log_std"].abs().max()) == 0.0 and float(init["action_net.bias"].abs().max()) == 0.0
    w = init["features_extractor.cnn.2.weight"].double().reshape(64, -1)
    assert torch.allclose(w @ w.T, 2.0 * torch.eye(64, dtype=torch.float64, device=w.device), atol=1e-5)      # orthogonal, gain sqrt 2
    w = init["value_net.weight"].double()
    assert torch.allclose(w @ w.T, torch.ones(1, 1, dtype=torch.float64, device=w.device), atol=1e-5)


def test_wrong_pictures_are_refused_on_the_device(built):
    C, S, F, A = 1, 36, 16, 1
    pol, _ = policy_for(C, S, F, A, n=4)
    good = torch.zeros(4, C, S, S, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="lives on cpu"):
        pol(good.cpu())
    with pytest.raises(ValueError, match="expected shape"):
        pol(good[:3])
    with pytest.raises(ValueError, match="expected torch.uint8 pictures"):
        pol.values(good.float())
    with pytest.raises(ValueError, match="expected torch.uint8 or torch.float32 pictures"):
        pol.evaluate_actions(good.double(), torch.zeros(4, A, device="cuda"))
    assert pol.calls == 0


# --------------------------------------------------------------------------------------------------- 10. on the engine
@pytest.mark.parametrize("k", [1, 4])
def test_on_the_engine_with_the_image_rollout_buffer(built, k):
    from mycobotgym_amd import CnnActorCritic, FrameStack, ImageRolloutBuffer, make
    T, n = 4, 32
    base = make(ENV_ID, num_envs=n)
    envs = base if k == 1 else FrameStack(base, k)
    C, S, A = envs.channels, envs.image_size, envs.action_dim
    assert C == k * base.channels
    twin = ic.Twin(C, S, 64, A).randomize(3)
    pol = CnnActorCritic.from_module(twin, envs, seed=SEED)
    assert (pol.num_envs, pol.channels, pol.image_size, pol.act_dim, pol.features_dim) == (n, C, S, A, 64)
    buf = ImageRolloutBuffer(envs, n_steps=T, seed=0) if k == 1 else ImageRolloutBuffer(envs, n_steps=T, seed=0, frame_stack=k)
    img, info = envs.reset(seed=0)
    buf.start(img)
    for t in range(T):
        a, v, logp = pol(img)
        img, r, term, trunc, info = envs.step(a)
        buf.add(a, v, logp, img, r, term, trunc, info, final_values=pol.values(info["final_observation"]))
    buf.finish(last_values=pol.values(img))
    assert pol.calls == T
    f32, u8 = buf.gather(0, 0, n * T, normalize=True), buf.gather(0, 0, n * T, normalize=False)
    assert f32.observations.dtype == torch.float32 and u8.observations.dtype == torch.uint8
    assert tuple(f32.observations.shape) == (n * T, C, S, S) and torch.equal(f32.actions, u8.actions)
    out32 = pol.evaluate_actions(f32.observations, f32.actions)
    out8 = pol.evaluate_actions(u8.observations, u8.actions)
    torch.cuda.synchronize()
    for x, y in zip(out32, out8):                                             # byte / 255 in the buffer and in the kernel: equal bits
        assert torch.isfinite(x).all() and torch.equal(x, y)
    for x in (f32.old_values, f32.old_log_prob, f32.advantages, f32.returns):
        assert torch.isfinite(x).all()
    value, log_prob, _ = (x.cpu().numpy() for x in out32)
    assert np.array_equal(bits(value), bits(f32.old_values.cpu().numpy()))    # the same pictures, the same weights
    # the yardstick: the twin's own evaluate_actions error against the float64 rule on the minibatch
    pictures, actions = u8.observations.cpu().numpy(), u8.actions.cpu().numpy()
    sd = twin.numpy_state()
    _, mean64, _ = ic.rule(sd, ic.preprocess(pictures))
    with torch.no_grad():
        _, lp32, _ = twin.evaluate_actions(torch.from_numpy(pictures), torch.from_numpy(actions))
    twin_err = np.abs(lp32.numpy() - ic.log_prob(actions, mean64, sd["log_std"])).max()
    gap = np.abs(log_prob - f32.old_log_prob.cpu().numpy()).max()
    print(f"engine k={k}: |evaluate_actions - stored log_prob| {gap:.3e}, twin's own error {twin_err:.3e}, ratio {gap / twin_err:.2f}")
    assert twin_err > 0 and gap <= 10.0 * twin_err
    mb = next(iter(buf.get(batch_size=48)))
    assert all(torch.isfinite(x).all() for x in pol.evaluate_actions(mb.observations, mb.actions))
    base.close()
