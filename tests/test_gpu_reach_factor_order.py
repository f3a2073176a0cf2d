"""The side waves' factor of H = H_eq + M under SplitMainCols (the joint controller's three-wave Reach kernel): build_factor_H reads H
row by row from row 11 down and factors each row as it arrives, where build_H + ldl_factor<PAT_H> read everything, rows ascending,
and then factor.  The two must give the same bits: each element takes the same fma's in the same order (mcg_dynamics.hpp).

(a) The device self-test mcg_selftest_factor_h on 64 lanes: both routes on the same LDS column.  H_eq is positive semidefinite on the
    pattern of the equality rows (PAT_E: two connect cliques over the arm dofs, the gear coupling), M positive definite on the
    kinematic tree's pattern (PAT_M), both seeded in numpy; the lanes cycle through no limit row / D on row 6 / on row 8 / on both, and
    lane SCALED_LANE is scaled so that the diagonal of H spans 1e-7 .. 1e6 (the built-in model's armatures against its link inertias
    times the constraint stiffness).  L, dinv and the solution of one right-hand side are bit-equal between the routes, and within
    1e-12 of a float64 numpy L^T D L of the same matrix: dinv relative per pivot; L and x in the scaling that makes H's diagonal one
    (R = sqrt(D) L / sqrt(diag H), entries at most one; x sqrt(diag H) relative to its largest entry), which is the measure in which
    the factorisation's rounding errors are bounded by the scaled condition number, whatever the lane's units.  The figure was checked
    on the CPU first (test_numpy_factor_against_extended_precision, which needs no GPU): the float64 numpy route against the same
    elimination in extended precision on these very matrices stays below 1e-13 in that measure, the scaled condition numbers are below
    1e3, so 1e-12 stands as the issue states it.

(b) Sub-steps and whole env-steps against the CPU oracle, on the states of tests/test_gpu_reach_side_wave_slots.py (the oracle runs of
    tests/reach_measures.py, shared through its cache): no gear row; row 6 only; row 8 only; both rows at either limit; an arm limit
    violated from the first sub-step, so that the RNE wave skips its solve and the main wave takes the unchanged route; remote -> main-wave solve -> remote;
    an auto-reset; at 165 environments (two full workgroups and a ragged one) and mixed lanes at 65.  Added here: three free-running
    env-steps with the auto-reset at the end of the second (`reset3`).  Bounds: 100 x the parent build's errors on the same states
    (profiles/r14/factor_order_parent.log); the figures are in the comments.
"""
import functools

import numpy as np
import pytest

from tests import reach_parity as rp
from tests.common import torch_cuda  # noqa: F401
from tests.reach_measures import SLOT_RUNS as RUNS, measure_slot_env_steps, measure_slot_substeps, slot_engine, slot_oracle_run
from tests.reach_parity import N, SEED

NB, TRI = 12, 78
PAR = (-1, 0, 1, 2, 3, 4, 5, 6, 5, 8, 5, 5)          # mcg_dynamics.hpp
LANES = 64
SCALED_LANE = 37
F_IN, F_OUT = 188, 204                                # MCG_SELFTEST_FACTOR_H_IN / _OUT
EPS = 1e-12


def tri(i, j):
    return i * (i + 1) // 2 + j if i >= j else j * (j + 1) // 2 + i


def patterns():
    """PAT_M, PAT_E, PAT_H of mcg_dynamics.hpp (symbolic): [12, 12] bool, lower triangles."""
    def anc(a, i):
        while i >= 0:
            if i == a: return True
            i = PAR[i]
        return False
    m = np.zeros((NB, NB), bool)
    for i in range(NB):
        for j in range(i + 1): m[i, j] = anc(j, i)
    e = m.copy()
    for grp in ((6, 7, 10), (8, 9, 11)):
        for a in grp:
            for b in grp:
                if a >= b: e[a, b] = True
            e[a, :6] = True
    e[8, 6] = True
    h = e.copy()
    for k in range(NB - 1, -1, -1):
        for i in range(k):
            if h[k, i]:
                for j in range(i + 1):
                    if h[k, j]: h[i, j] = True
    return m, e, h


@functools.lru_cache(maxsize=None)
def factor_cases():
    """-> (table [64, 188] for mcg_selftest_factor_h, H [64, 12, 12] = H_eq + M + D on the active rows, b [64, 12])."""
    pm, pe, _ = patterns()
    rng = np.random.default_rng([SEED, 14])
    table, Hs = np.zeros((LANES, F_IN)), np.zeros((LANES, NB, NB))
    for c in range(LANES):
        Lm = np.eye(NB)
        for i in range(NB):
            for j in range(i): Lm[i, j] = rng.normal(0, 0.4) if pm[i, j] else 0.0
        M = Lm.T @ np.diag(rng.uniform(0.5, 2.0, NB)) @ Lm
        E = np.zeros((NB, NB))
        for grp in ((6, 7, 10), (8, 9, 11)):
            for _ in range(3):                                        # a connect's three rows: the arm dofs and the clique
                v = np.zeros(NB); v[:6] = rng.normal(0, 0.3, 6); v[list(grp)] = rng.normal(0, 1.0, 3)
                E += rng.uniform(1.0, 30.0) * np.outer(v, v)
        v = np.zeros(NB); v[6], v[8] = 1.0, -1.0                      # the gear coupling
        E += rng.uniform(1.0, 30.0) * np.outer(v, v)
        D = rng.uniform(1.0, 50.0, 10)
        act = np.zeros(10); act[6] = (c % 4) in (1, 3); act[8] = (c % 4) in (2, 3)
        b = rng.normal(0, 1.0, NB)
        if c == SCALED_LANE:
            H0 = E + M + np.diag(np.concatenate([D * act, [0, 0]]))
            s = np.sqrt(rng.permutation(np.logspace(-7, 6, NB)) / np.diag(H0))
            M, E, D, b = M * np.outer(s, s), E * np.outer(s, s), D * s[:10] ** 2, b * s
        low = np.tril(np.ones((NB, NB), bool))
        assert not M[low & ~pm].any() and not E[low & ~pe].any()      # nothing off the patterns
        for i in range(NB):
            for j in range(i + 1): table[c, tri(i, j)], table[c, TRI + tri(i, j)] = E[i, j], M[i, j]
        table[c, 2 * TRI:2 * TRI + 10], table[c, 2 * TRI + 10:2 * TRI + 20], table[c, 2 * TRI + 20:] = D, act, b
        # H from the table's own (rounded) entries, formed as the device forms it: (H_eq + M) + D
        Hs[c] = np.tril(E) + np.tril(M); Hs[c][np.arange(10), np.arange(10)] += D * act
        Hs[c] = np.tril(Hs[c]) + np.tril(Hs[c], -1).T
    return rp.freeze((table, Hs))


def ldl_numpy(H, b, dtype=np.float64):
    """A = L^T D L from the last row up, as ldl_factor does, in plain `dtype` arithmetic: -> (L unit lower with D on the diagonal, 1 / D, x)."""
    A, x = np.tril(H).astype(dtype), b.astype(dtype).copy()
    dinv = np.zeros(NB, dtype)
    for k in range(NB - 1, -1, -1):
        dinv[k] = dtype(1) / A[k, k]
        for i in range(k - 1, -1, -1):
            l = A[k, i] * dinv[k]
            A[i, :i + 1] -= l * A[k, :i + 1]
            A[k, i] = l
    for k in range(NB - 1, -1, -1): x[:k] -= A[k, :k] * x[k]
    x *= dinv
    for k in range(NB): x[k] -= A[k, :k] @ x[:k]
    return A, dinv, x


def scaled_errors(H, got, ref):
    """(L, dinv, x) `got` against `ref` in the measure of the docstring: -> (eL, ed, ex)."""
    h = np.sqrt(np.diag(H)).astype(np.float64)
    out = []
    (Lg, dg, xg), (Lr, dr, xr) = [tuple(np.asarray(a, np.float64) for a in t) for t in (got, ref)]
    R = lambda L, d: np.tril(L, -1) / np.sqrt(d)[:, None] / h[None, :]
    eL = np.abs(R(Lg, dr) - R(Lr, dr)).max()
    ed = (np.abs(dg - dr) / np.abs(dr)).max()
    ex = np.abs((xg - xr) * h).max() / np.abs(xr * h).max()
    return float(eL), float(ed), float(ex)


def test_numpy_factor_against_extended_precision():
    """The tolerance of part (a), on the CPU: the float64 numpy route against the same elimination in extended precision, and the scaled
    condition number of every lane's H."""
    table, Hs = factor_cases()
    worst, cond = np.zeros(3), 0.0
    for c in range(LANES):
        b = table[c, 2 * TRI + 20:]
        worst = np.maximum(worst, scaled_errors(Hs[c], ldl_numpy(Hs[c], b), ldl_numpy(Hs[c], b, np.longdouble)))
        h = np.sqrt(np.diag(Hs[c]))
        cond = max(cond, np.linalg.cond(Hs[c] / np.outer(h, h)))
    d = np.diag(Hs[SCALED_LANE])
    print(f"\nfloat64 numpy against extended precision: L {worst[0]:.3e} dinv {worst[1]:.3e} x {worst[2]:.3e}; largest scaled condition number {cond:.3e}; "
          f"diagonal of the scaled lane {d.min():.3e} .. {d.max():.3e}")
    assert np.finfo(np.longdouble).eps < 1e-18                         # extended precision is what it says
    assert d.min() < 2e-7 and d.max() > 5e5
    assert (worst <= EPS / 10).all() and cond < 1e3, (worst, cond)


def run_factor(torch, fn, table):
    """-> out [n, 2, 102] of the entry `fn` (mcg_selftest_factor_h of some build): route, then L[78] dinv[12] x[12]."""
    n = table.shape[0]
    dev = torch.device("cuda:0")
    t_in = torch.as_tensor(np.array(table), device=dev)               # (a writable copy)
    out = torch.full((n, F_OUT), float("nan"), dtype=torch.float64, device=dev)
    rc = fn(t_in.data_ptr(), n, out.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    return out.cpu().numpy().reshape(n, 2, F_OUT // 2)


def check_factor(torch, fn):
    """The assertions of test_both_routes_give_the_same_factor, for any build's entry (profiles/r14/mutations.md runs mutants through it)."""
    table, Hs = factor_cases()
    _, _, ph = patterns()
    out = run_factor(torch, fn, table)
    assert np.isfinite(out).all()
    names = ("L", "dinv", "x")
    parts = lambda o: (o[:TRI], o[TRI:TRI + NB], o[TRI + NB:])
    differ = [(c, nm) for c in range(LANES) for nm, a, b in zip(names, parts(out[c, 0]), parts(out[c, 1])) if not np.array_equal(a.view(np.uint64), b.view(np.uint64))]
    worst = np.zeros(3)
    for c in range(LANES):
        ref = ldl_numpy(Hs[c], table[c, 2 * TRI + 20:])
        for route in (0, 1):
            Lp, dinv, x = parts(out[c, route])
            L = np.zeros((NB, NB))
            for i in range(NB):
                for j in range(i + 1): L[i, j] = Lp[tri(i, j)]
            assert not L[np.tril(np.ones((NB, NB), bool)) & ~ph].any()
            worst = np.maximum(worst, scaled_errors(Hs[c], (L, dinv, x), ref))
    print(f"\nfactor self-test: {LANES} lanes, routes differ in {len(differ)} (lane, array) pairs; against float64 numpy: L {worst[0]:.3e} dinv {worst[1]:.3e} x {worst[2]:.3e}")
    assert not differ, differ[:10]
    assert (worst <= EPS).all(), worst


@pytest.mark.gpu
def test_both_routes_give_the_same_factor(torch_cuda):
    from mycobotgym_amd import _abi
    check_factor(torch_cuda, _abi.load().mcg_selftest_factor_h)


# ------------------------------------------------------------------------------------------------------- (b) against the oracle
SUB_BOUNDS = {      # single sub-steps: obs, q, v, w = 100 x the parent build's worst error (the measured figures in the comment)
    ("none", N): dict(obs=7.772e-14, q=8.162e-12, v=4.081e-09, w=4.353e-11),                # 7.772e-16  8.162e-14  4.081e-11  4.353e-13
    ("row6", N): dict(obs=5.551e-14, q=8.563e-12, v=4.282e-09, w=4.693e-11),                # 5.551e-16  8.563e-14  4.282e-11  4.693e-13
    ("row8", N): dict(obs=4.996e-14, q=8.632e-12, v=4.317e-09, w=4.046e-11),                # 4.996e-16  8.632e-14  4.317e-11  4.046e-13
    ("both_lower", N): dict(obs=5.551e-14, q=1.823e-13, v=9.116e-11, w=4.663e-11),          # 5.551e-16  1.823e-15  9.116e-13  4.663e-13
    ("both_upper", N): dict(obs=5.551e-14, q=9.628e-12, v=4.813e-09, w=3.359e-11),          # 5.551e-16  9.628e-14  4.813e-11  3.359e-13
    ("arm", N): dict(obs=7.216e-14, q=1.317e-11, v=6.585e-09, w=4.004e-11),                 # 7.216e-16  1.317e-13  6.585e-11  4.004e-13
    ("switch", N): dict(obs=6.939e-14, q=9.420e-12, v=4.711e-09, w=4.222e-11),              # 6.939e-16  9.420e-14  4.711e-11  4.222e-13
    ("reset", N): dict(obs=1.221e-13, q=6.950e-12, v=3.475e-09, w=4.392e-11),               # 1.221e-15  6.950e-14  3.475e-11  4.392e-13
    ("mixed", 65): dict(obs=7.216e-14, q=6.734e-12, v=3.368e-09, w=3.365e-11),              # 7.216e-16  6.734e-14  3.368e-11  3.365e-13
}
ENV_BOUNDS = {      # whole env-steps: likewise
    ("none", N): dict(obs=2.290e-11, q=1.870e-11, v=3.243e-09, w=4.352e-10),                # 2.290e-13  1.870e-13  3.243e-11  4.352e-12
    ("row6", N): dict(obs=3.239e-11, q=2.552e-11, v=4.008e-09, w=1.104e-09),                # 3.239e-13  2.552e-13  4.008e-11  1.104e-11
    ("row8", N): dict(obs=9.566e-12, q=9.176e-12, v=1.630e-09, w=5.113e-10),                # 9.566e-14  9.176e-14  1.630e-11  5.113e-12
    ("both_lower", N): dict(obs=2.241e-11, q=1.221e-11, v=2.792e-09, w=2.518e-10),          # 2.241e-13  1.221e-13  2.792e-11  2.518e-12
    ("both_upper", N): dict(obs=4.006e-11, q=1.077e-11, v=4.034e-09, w=2.686e-09),          # 4.006e-13  1.077e-13  4.034e-11  2.686e-11
    ("arm", N): dict(obs=1.643e-11, q=1.516e-11, v=1.875e-09, w=2.868e-10),                 # 1.643e-13  1.516e-13  1.875e-11  2.868e-12
    ("switch", N): dict(obs=6.636e-12, q=4.283e-12, v=1.659e-09, w=1.960e-10),              # 6.636e-14  4.283e-14  1.659e-11  1.960e-12
    ("reset", N): dict(obs=1.298e-09, q=3.487e-09, v=1.644e-07, w=6.491e-08),               # 1.298e-11  3.487e-11  1.644e-09  6.491e-10
    ("mixed", 65): dict(obs=6.361e-12, q=3.897e-12, v=8.023e-10, w=9.548e-11),              # 6.361e-14  3.897e-14  8.023e-12  9.548e-13
}
# three free-running env-steps (the servo-driven dynamics amplify rounding from env-step to env-step: DESIGN.md section 3)
RESET3_BOUNDS = {N: dict(obs=4.738e-06, q=1.675e-06, v=3.159e-04, w=1.365e-04)}              # 4.738e-08  1.675e-08  3.159e-06  1.365e-06


@functools.lru_cache(maxsize=None)
def oracle_reset3(n):
    """Three whole env-steps from the `reset` case's state, the episodes of a fifth of the lanes one step younger: the second env-step
    truncates and auto-resets them, the third runs the fresh lanes next to running ones."""
    r = slot_oracle_run("reset", n)
    late = np.arange(n) % 5 == 2
    el = r["env_pre"]["elapsed"].copy(); el[late] = 48
    r3 = rp.replay_env_steps(rp.oracle(n, 20, SEED, 50), dict(r["env_pre"], elapsed=el), r["action"], steps=3)
    tr = [o["truncated"].astype(bool) for o in r3["env_out"]]
    assert not tr[0].any() and np.array_equal(tr[1], late) and not tr[2].any()
    return dict(action=r["action"], **rp.freeze(r3))


def measure_reset3(n):
    return rp.measure_env_steps(oracle_reset3(n), lambda frame_skip: slot_engine("reset", n, frame_skip), f"reset3 ({n}) env-steps")


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_substeps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_slot_substeps(case, n), SUB_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)


@pytest.mark.gpu
@pytest.mark.parametrize("case,n", RUNS, ids=[f"{c}-{n}" for c, n in RUNS])
def test_env_steps_against_the_oracle(torch_cuda, case, n):
    w, b = measure_slot_env_steps(case, n), ENV_BOUNDS[(case, n)]
    assert rp.within(w, b), (w, b)


@pytest.mark.gpu
def test_three_env_steps_with_an_auto_reset(torch_cuda):
    w, b = measure_reset3(N), RESET3_BOUNDS[N]
    assert rp.within(w, b), (w, b)
