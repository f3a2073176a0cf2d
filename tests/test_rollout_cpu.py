"""The on-policy rollout buffer without a GPU: the ABI's layout, the host refusals, and known answers and properties of the rule
(tests/indep_rollout.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.indep_rollout import PERM_SEED, Rollout, feistel_bits, record_dtype, walk

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_structs_match_header_layout(built, tmp_path):
    """sizeof / offsetof of mcg_rollout_buf and mcg_rollout_batch as the C compiler sees include/mcg.h == the ctypes mirrors."""
    from mycobotgym_amd import _abi
    buf_fields = [n for n, _ in _abi.McgRolloutBuf._fields_]
    batch_fields = [n for n, _ in _abi.McgRolloutBatch._fields_]
    exprs = (["sizeof(mcg_rollout_buf)", "sizeof(mcg_rollout_batch)"] + [f"offsetof(mcg_rollout_buf,{n})" for n in buf_fields]
             + [f"offsetof(mcg_rollout_batch,{n})" for n in batch_fields])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_abi.McgRolloutBuf), C.sizeof(_abi.McgRolloutBatch)] + [getattr(_abi.McgRolloutBuf, n).offset for n in buf_fields]
            + [getattr(_abi.McgRolloutBatch, n).offset for n in batch_fields])
    assert got == want
    assert len(buf_fields) == 15 and len(batch_fields) == 9
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays


@pytest.mark.parametrize("D,A", [(10, 7), (25, 7), (25, 4), (25, 8)])
def test_rollout_record_bytes(built, D, A):
    from mycobotgym_amd import _abi
    got = _abi.load().mcg_rollout_record_bytes(D, A)
    fields = 4 * (D + 3 + 3 + A + 1)          # obs, achieved, desired, action, log_prob
    assert got % 16 == 0 and fields <= got < fields + 16
    assert got == record_dtype(D, A).itemsize == _abi.rollout_record_dtype(D, A).itemsize
    assert _abi.rollout_record_dtype(D, A).fields.keys() == record_dtype(D, A).fields.keys()
    for name, (dt, off) in {k: v[:2] for k, v in record_dtype(D, A).fields.items()}.items():
        assert _abi.rollout_record_dtype(D, A).fields[name][:2] == (dt, off), name


BUF_POINTERS = ("records", "reward", "value", "episode_start", "advantage", "returns", "last_obs", "last_goals", "last_start")


def _buf(_abi, **over):
    p = C.c_void_p(0x1000)            # never dereferenced: the refusals come before any HIP call
    kw = dict({n: p for n in BUF_POINTERS}, n_envs=3, obs_dim=25, act_dim=7, n_steps=4, gamma=0.99, gae_lambda=0.95)
    kw.update(over)
    return _abi.McgRolloutBuf(**kw)


def test_rollout_host_refusals_without_a_gpu(built):
    """Every argument check of the four calls: the code and a fragment of its message, with no GPU in the machine."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = C.c_void_p(0x1000)
    step = _abi.McgStepOut(**{n: 0x1000 for n, _ in _abi.McgStepOut._fields_})
    batch = _abi.McgRolloutBatch(obs=0x1000)
    ARG = _abi.MCG_ERR_ARG
    ref = lambda x: None if x is None else C.byref(x)

    def start(b, first=step):
        return L.mcg_rollout_start(ref(b), ref(first), None, None)

    def add(b, pos=0, actions=p, values=p, log_probs=p, final_values=None, out=step):
        return L.mcg_rollout_add(ref(b), pos, actions, values, log_probs, final_values, ref(out), None)

    def gae(b, last_values=p):
        return L.mcg_rollout_gae(ref(b), last_values, None)

    def gather(b, first=0, count=4, out=batch):
        return L.mcg_rollout_gather(ref(b), 0, 0, first, count, ref(out), None)

    def refused(code, text):
        assert code == ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    for call in (start, add, gae, gather):
        refused(call(None), "null mcg_rollout_buf")
        for name in BUF_POINTERS:
            refused(call(_buf(_abi, **{name: None})), "null pointer in mcg_rollout_buf")
        for name in ("n_envs", "obs_dim", "act_dim", "n_steps"):
            refused(call(_buf(_abi, **{name: 0})), "must be >= 1")
            refused(call(_buf(_abi, **{name: -4})), "must be >= 1")
        refused(call(_buf(_abi, n_envs=2 ** 20, n_steps=2 ** 11)), "below 2^31")
        refused(call(_buf(_abi, n_envs=2 ** 31 - 1, n_steps=2 ** 31 - 1)), "below 2^31")
        refused(call(_buf(_abi, records=C.c_void_p(0x1008))), "not 16-byte aligned")
        for name in ("gamma", "gae_lambda"):
            for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
                refused(call(_buf(_abi, **{name: bad})), "finite and in [0, 1]")
    good = _buf(_abi)
    refused(start(good, first=None), "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal"):
        first = _abi.McgStepOut(**{n: (None if n == name else 0x1000) for n in ("obs", "achieved_goal", "desired_goal")})
        refused(start(good, first=first), "are required")
    refused(add(good, pos=-1), "pos outside [0, n_steps)")
    refused(add(good, pos=4), "pos outside [0, n_steps)")
    refused(add(good, actions=None), "null actions")
    refused(add(good, values=None), "null values")
    refused(add(good, log_probs=None), "null log_probs")
    refused(add(good, out=None), "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal", "reward", "terminated", "truncated"):
        out = _abi.McgStepOut(**{n: (None if n == name else 0x1000) for n, _ in _abi.McgStepOut._fields_})
        refused(add(good, out=out), "are required")
    refused(gae(good, last_values=None), "null last_values")
    refused(gather(good, first=-1), "first < 0")
    refused(gather(good, count=0), "count must be >= 1")
    refused(gather(good, count=-3), "count must be >= 1")
    refused(gather(good, first=0, count=13), "first + count > n_steps * n_envs")
    refused(gather(good, first=9, count=4), "first + count > n_steps * n_envs")
    refused(gather(good, first=12, count=1), "first + count > n_steps * n_envs")
    refused(gather(good, first=2 ** 62, count=2 ** 62), "first + count > n_steps * n_envs")
    refused(gather(good, out=None), "null mcg_rollout_batch")
    refused(gather(good, out=_abi.McgRolloutBatch()), "all outputs are null")
    assert L.mcg_rollout_record_bytes(0, 7) == 0 and L.mcg_rollout_record_bytes(25, 0) == 0 and L.mcg_rollout_record_bytes(-1, -1) == 0


# ---- known answers of the rule, by hand
def _hand_rollout(with_final_values):
    N, D, A, T = 2, 2, 1, 3
    R = Rollout(N, D, A, T, gamma=0.5, gae_lambda=0.5)
    z = lambda *s: np.zeros(s)
    R.start(z(N, D), z(N, 3), z(N, 3))
    rewards = [[1.0, -1.0], [2.0, 0.5], [4.0, 2.0]]
    values = [[0.5, 1.0], [1.0, -2.0], [2.0, 0.25]]
    terminated = [[1, 0], [0, 0], [0, 0]]          # env 0: its first episode ends (by success) at step 0
    truncated = [[1, 0], [0, 0], [0, 1]]           # env 1: the time limit ends its episode at step 2
    for t in range(T):
        out = dict(obs=z(N, D), achieved_goal=z(N, 3), desired_goal=z(N, 3), reward=np.array(rewards[t]),
                   terminated=np.array(terminated[t], bool), truncated=np.array(truncated[t], bool))
        R.add(z(N, A).astype(np.float32), np.array(values[t], np.float32), z(N).astype(np.float32), out,
              final_values=np.array([64.0, 8.0], np.float32) if with_final_values else None)
    R.finish(np.array([4.0, 100.0], np.float32))
    return R


def test_rule_gae_known_answers_by_hand():
    """T = 3, N = 2, gamma = 0.5, lambda = 0.5: g = 0.5, c = 0.25, every operation exact in float32.

    Environment 0: rewards 1 2 4, values 0.5 1 2, last value 4; step 0 ends its first episode by success (terminated, and the engine sets
    truncated with it: no bootstrap although a final value of 64 is offered), so episode_start = 1 1 0 and last_start = 0.
        t = 2: nnt = 1, delta = 4 + 0.5 * 4 - 2 = 4,     last = 4 + 0.25 * 0 = 4,        returns = 6
        t = 1: nnt = 1, delta = 2 + 0.5 * 2 - 1 = 2,     last = 2 + 0.25 * 4 = 3,        returns = 4
        t = 0: nnt = 0, delta = 1 + 0 - 0.5 = 0.5,       last = 0.5 + 0 = 0.5,           returns = 1
    Environment 1: rewards -1 0.5 2, values 1 -2 0.25; the time limit ends its episode at step 2 (truncated, not terminated) with final
    value 8: reward[2] = 2 + 0.5 * 8 = 6, last_start = 1, and the last value (100) must not enter.
        t = 2: nnt = 0, delta = 6 + 0 - 0.25 = 5.75,           last = 5.75,                           returns = 6
        t = 1: nnt = 1, delta = 0.5 + 0.5 * 0.25 + 2 = 2.625,  last = 2.625 + 0.25 * 5.75 = 4.0625,   returns = 2.0625
        t = 0: nnt = 1, delta = -1 + 0.5 * -2 - 1 = -3,        last = -3 + 0.25 * 4.0625 = -1.984375, returns = -0.984375
    Without final values reward[2] stays 2: last = 1.75, 3.0625, -2.234375; returns = 2, 1.0625, -1.234375."""
    P = _hand_rollout(True).planes()
    assert P["episode_start"].T.tolist() == [[1, 1, 0], [1, 0, 0]]
    assert P["reward"].T.tolist() == [[1.0, 2.0, 4.0], [-1.0, 0.5, 6.0]]
    assert P["advantage"].T.tolist() == [[0.5, 3.0, 4.0], [-1.984375, 4.0625, 5.75]]
    assert P["returns"].T.tolist() == [[1.0, 4.0, 6.0], [-0.984375, 2.0625, 6.0]]
    assert _hand_rollout(True).carried()["last_start"].tolist() == [0, 1]
    P = _hand_rollout(False).planes()
    assert P["reward"].T.tolist() == [[1.0, 2.0, 4.0], [-1.0, 0.5, 2.0]]
    assert P["advantage"].T.tolist() == [[0.5, 3.0, 4.0], [-2.234375, 3.0625, 1.75]]
    assert P["returns"].T.tolist() == [[1.0, 4.0, 6.0], [-1.234375, 1.0625, 2.0]]
    assert all(v.dtype == (np.uint8 if k == "episode_start" else np.float32) for k, v in P.items())


def test_rule_gae_agrees_with_the_closed_form():
    """T = 33, N = 5, random inputs, episode ends at random steps.  Second route, float64: per episode the closed form
    A_t = sum_k (gamma lambda)^k delta_{t+k} up to the episode's end, delta_t = r_t + gamma v_{t+1} nnt_t - v_t, on the stored float32
    rewards and values and the exact gamma and lambda.

    Bound, per element, derived: term k of the sum carries, in the float32 recursion, three roundings of its delta (the product, the
    sum, the difference; each at most 2^-24 of a magnitude below |r| + |gamma v nnt| + |v|), two per later step (the product with c and
    the sum; c * nnt itself is exact), and the float32 casts of gamma (once) and of gamma * lambda (k times): at most 3 k + 4 <= 4 T
    relative errors of 2^-24 to first order.  So |A32 - A64| <= 4 T 2^-24 sum_k (gamma lambda)^k (|r| + |gamma v nnt| + |v|)_{t+k}.
    returns = A + v adds one rounding: 2^-24 (|A| + |v|)."""
    T, N, gamma, lam = 33, 5, 0.99, 0.95
    rng = np.random.default_rng(7)
    R = Rollout(N, 2, 1, T, gamma, lam)
    z = lambda *s: np.zeros(s)
    R.start(z(N, 2), z(N, 3), z(N, 3))
    ends = 0
    for t in range(T):
        done = rng.random(N) < 0.15
        terminated = done & (rng.random(N) < 0.5)
        ends += int(done.sum())
        out = dict(obs=z(N, 2), achieved_goal=z(N, 3), desired_goal=z(N, 3), reward=rng.normal(size=N), terminated=terminated, truncated=done)
        R.add(z(N, 1).astype(np.float32), rng.normal(size=N).astype(np.float32), z(N).astype(np.float32), out,
              final_values=rng.normal(size=N).astype(np.float32))
    last_values = rng.normal(size=N).astype(np.float32)
    R.finish(last_values)
    P, last_start = R.planes(), R.carried()["last_start"]
    assert ends >= 10 and 0 < last_start.sum() + P["episode_start"][-1].sum()
    r, v = P["reward"].astype(np.float64), P["value"].astype(np.float64)
    u, worst = 2.0 ** -24, 0.0
    for e in range(N):
        nnt = np.array([1.0 - (P["episode_start"][t + 1, e] if t + 1 < T else last_start[e]) for t in range(T)])
        vn = np.array([v[t + 1, e] if t + 1 < T else float(last_values[e]) for t in range(T)])
        delta = r[:, e] + gamma * vn * nnt - v[:, e]
        size = np.abs(r[:, e]) + np.abs(gamma * vn * nnt) + np.abs(v[:, e])
        for t in range(T):
            A, S, w = 0.0, 0.0, 1.0
            for k in range(T - t):
                A += w * delta[t + k]; S += w * size[t + k]
                if nnt[t + k] == 0.0:          # the episode ends with step t + k
                    break
                w *= gamma * lam
            bound = 4 * T * u * S
            err = abs(float(P["advantage"][t, e]) - A)
            worst = max(worst, err / bound)
            assert err <= bound, (t, e, err, bound)
            assert abs(float(P["returns"][t, e]) - (A + v[t, e])) <= bound + u * (abs(A) + abs(v[t, e])), (t, e)
    print(f"closed form: worst |A32 - A64| / bound = {worst:.3f}")


@pytest.mark.parametrize("T,N", [(1, 1), (4, 64), (7, 40), (3, 11)])
def test_rule_permutation_properties(T, N):
    """Each epoch's positions 0 .. M-1 map onto 0 .. M-1 exactly once; epochs differ; a (seed, epoch) repeats; the longest walk of the
    tests' seed over the epochs the GPU tests draw (0 .. 5, and one beyond 2^32) stays far below 64."""
    M = T * N
    b = feistel_bits(M)
    assert b % 2 == 0 and b >= 2 and (1 << b) >= M and (b == 2 or (1 << (b - 2)) < M)
    perms, longest = {}, 0
    for epoch in (0, 1, 2, 3, 4, 5, 2 ** 32 + 1):
        got = [walk(PERM_SEED, epoch, k, M) for k in range(M)]
        perms[epoch] = [x for x, _ in got]
        longest = max(longest, max(p for _, p in got))
        assert sorted(perms[epoch]) == list(range(M)), epoch
    print(f"(T, N) = ({T}, {N}): M = {M}, b = {b}, longest walk {longest} passes")
    assert longest <= 64
    if (1 << b) == M:
        assert longest == 1                    # nothing to walk past
    assert perms[0] == [x for x, _ in (walk(PERM_SEED, 0, k, M) for k in range(M))]
    if M > 1:
        assert perms[0] != perms[1] and perms[1] != perms[2 ** 32 + 1]          # the epoch's high word enters
        assert perms[0] != [x for x, _ in (walk(PERM_SEED + 1, 0, k, M) for k in range(M))]
        assert perms[0] != list(range(M))
