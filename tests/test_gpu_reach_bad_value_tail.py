"""GPU parity of the bad-value check that ends every sub-step of the joint controller's three-wave Reach kernel (SplitMainCols).

After the Euler step the main wave asks whether any of the twelve new positions, velocities or accelerations is NaN or beyond 1e10
(mj_checkPos / mj_checkVel / mj_checkAcc) and resets the lanes where one is.  Since round 13 the question is put as one maximum over the
36 magnitudes, one sum over the positions and two compares (bad_value_any in mcg_dynamics.hpp) instead of 36 compares.  This file holds the
per-lane decision to the CPU oracle's on states that land next to the threshold, and the state of every other lane to the oracle's.

One sub-step (frame_skip = 1) from a state set in the oracle and in the engine alike, at 165 environments (two full workgroups and a
ragged one) and at 65 (one full wave plus one lane, and that lane is a bad one).  The ordinary lanes are test_gpu_reach_after_s3.py's
`mixed` state: both gear rows / row 6 / row 8 / none by lane % 4, so the remote sub-step runs with and without gear rows.  The special
lanes, two or three of each kind per run (EDGE_KINDS):

  acc_below+ acc_below- acc_above+ acc_above-   the hinge of one linkage (dof 10 or 11, which have no limit rows) turns at about 2.5e7
        rad/s, so that its joint damping alone gives an acceleration next to 1e10; the speed comes from a bisection ON THE ORACLE for the
        speed v* at which mj_checkAcc starts to fire in that lane, and is v* (1 -+ 1e-6): the oracle alone shows that the lane's largest
        |qacc| lies in 1e10 (1 - 3e-6, 1) or that the check fired.  The sign is the acceleration's.  Decided by a[] in bad_value_any.
  pos_below+ pos_below- pos_above+ pos_above-   the same hinge stands at +-(1e10 - d) rad and moves outwards at 1e4 rad/s; the oracle, run
        once from +-1e10, gives the lane's displacement D of one sub-step, and d = 1.5 D or 0.5 D puts the new position D / 2 short of
        1e10 or D / 2 beyond it (D is about 4 rad: 4e-10 of the threshold).  Velocity and acceleration stay far below 1e10.  Decided by qn[].
  vel+ vel-   arm joint 1 at +-9.9e9 rad/s, which passes the check when the step starts.  No admissible state puts a new VELOCITY next to
        1e10 with the acceleration below it -- in the oracle any of the twelve joints at 1e9 rad/s, a tenth of the threshold, already has
        mj_checkAcc fire (damping and centrifugal terms) -- so these lanes are bad through a[] and qdn[] at once.

The same state goes through an env-step of two sub-steps as well (the last test says what that shows and one sub-step cannot).

What no state reaches, and where it is tested instead: +-inf and NaN through the acceleration, two opposite infinities in one lane, a new
VELOCITY next to 1e10 on its own, a magnitude of exactly 1e10.  With the built-in model no state that passes the check at the start of a
step (every |q|, |qd|, |warm| <= 1e10) overflows a double anywhere in the sub-step -- the largest intermediate is about 1e50 -- and the
actuator clamp swallows a NaN action, so the kernel cannot be brought to produce such a value from the outside.  The last test of the
file therefore runs the predicate itself on the device (mcg_selftest_bad_value: bad_value_any beside the 36 bad_value calls it
replaces, on the same registers, the new velocities and positions formed by the sub-step's own chain of fmas) on a table of 1076 cases:
each of those values in each of the 36 slots and either sign, opposite infinities in two joints, an infinity out of the solve, sums
that overflow.  Not here: a bad value in sub-step 10 of a whole env-step (it comes in sub-step 1 of 2 instead); the hinge's position at 1e10
rad cannot be steered through ten sub-steps (the engine's sine and cosine are two-constant Cody-Waite and meaningless at 1e10 rad, see
the `pos` bounds).

Requirements.  (1) The engine resets exactly the lanes the oracle's checks flag -- mj_checkAcc in this step, or mj_checkPos / mj_checkVel on
the state the step leaves, which mj_step would apply when the next one starts: a boolean per lane, no tolerance; a reset lane holds
qpos0, zero velocity, zero warm start, and the engine counts one bad-state reset per such lane.  (2) The lanes that are not special are the
same bits as in a run of the same state without the special lanes.  (3) Every lane that is not reset is within BOUNDS of the oracle:
100 x the worst error of the parent build (round 12, 36 compares) on these very states (profiles/r13/bad_value_tail_parent.log), for the
ordinary lanes, the `acc_below` lanes and the `pos_below` lanes apart.
"""
import functools

import numpy as np
import pytest

from tests import reach_parity as rp
from tests.common import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu

SEED = 67
LIMIT = 1e10
EDGE_KINDS = ("acc_below+", "acc_below-", "acc_above+", "acc_above-", "pos_below+", "pos_below-", "pos_above+", "pos_above-", "vel+", "vel-")
SLOT0, STRIDE = 3, 6                                 # kind k sits in lanes 3 + 6 k of every workgroup: good lanes on either side of each
RUNS = (165, 65)

# obs, q, v absolute, w relative to the lane's largest |qacc|: 100 x the parent build's worst error (the measured figures in the comments)
# The `pos_below` figures are what the engine's sine and cosine at 1e10 rad are worth (above); they bound nothing of interest, the
# decision in those lanes is what counts.  The new build's errors are the parent's figure for figure.
BOUNDS = {
    165: dict(ordinary=dict(obs=5.9e-14, q=5.4e-12, v=2.7e-09, w=3.9e-11),         # 5.933e-16  5.429e-14  2.716e-11  3.990e-13
              acc_below=dict(obs=1.2e-08, q=8.6e-07, v=4.3e-04, w=1.9e-11),        # 1.208e-10  8.640e-09  4.320e-06  1.999e-13
              pos_below=dict(obs=1.4e+00, q=6.4e+01, v=3.2e+04, w=4.0e+00)),       # 1.407e-02  6.465e-01  3.233e+02  4.028e-02
    65: dict(ordinary=dict(obs=5.8e-14, q=8.2e-12, v=4.1e-09, w=2.7e-11),          # 5.898e-16  8.255e-14  4.128e-11  2.712e-13
             acc_below=dict(obs=9.6e-09, q=4.7e-07, v=2.3e-04, w=1.5e-11),         # 9.634e-11  4.713e-09  2.356e-06  1.589e-13
             pos_below=dict(obs=1.3e+00, q=4.0e+01, v=2.0e+04, w=2.5e+00)),        # 1.385e-02  4.078e-01  2.039e+02  2.538e-02
}


def kinds_of(n):
    """-> [n] index into EDGE_KINDS, -1 for an ordinary lane.  At 65 the lone lane of the second wave is an `acc_above-` lane."""
    k = -np.ones(n, np.int64)
    for lane in range(n):
        r = lane % 64 - SLOT0
        if r >= 0 and r % STRIDE == 0 and r // STRIDE < len(EDGE_KINDS): k[lane] = r // STRIDE
    if n == 65: k[64] = EDGE_KINDS.index("acc_above-")
    return k


def _warnings(ora, n):
    return np.array([int(ora.data(i).get("warning_badstate", (1,), np.int32)[0]) for i in range(n)])


def _step_from(ora, s, q, qd, a, n):
    """One oracle sub-step from state s with positions q and velocities qd: (fired [n] = a check fired inside the step, out, post)."""
    ora.set_state(**{**s, "qpos": q, "qvel": qd})
    w0 = _warnings(ora, n)
    out = ora.step(a)
    return _warnings(ora, n) > w0, out, ora.get_state()


@functools.lru_cache(maxsize=None)
def oracle_run(n):
    """The run's one sub-step on the CPU oracle alone, with the special lanes and without them (`clean`):
    dict(kind, action, pre, out, post, bad, why, pre_clean, out_clean, post_clean)."""
    rng = np.random.default_rng([SEED, n])
    ora = rp.oracle(n, 1, SEED, running=rng)
    a = rp.put_gear_case("mixed", ora, rng, n)
    s = ora.get_state()
    kind = kinds_of(n)
    name = np.array([EDGE_KINDS[k] if k >= 0 else "" for k in kind])
    sign = np.where(np.char.endswith(name, "+"), 1.0, -1.0)
    hinge = 10 + (np.arange(n) // 64) % 2                                  # dof 10 in even workgroups, 11 in odd ones
    lanes = lambda prefix: np.nonzero(np.char.startswith(name, prefix))[0]
    q, qd = s["qpos"].copy(), s["qvel"].copy()

    # acc: bisection for the hinge speed at which mj_checkAcc starts to fire (damping: the acceleration opposes the speed)
    acc = lanes("acc_")
    lo, hi = np.full(n, 1e7), np.full(n, 1e8)
    for _ in range(48):
        mid = 0.5 * (lo + hi)
        t = s["qvel"].copy(); t[acc, hinge[acc]] = -sign[acc] * mid[acc]
        fired, _, _ = _step_from(ora, s, s["qpos"], t, a, n)
        assert not fired[kind < 0].any()
        lo, hi = np.where(fired, lo, mid), np.where(fired, mid, hi)
    assert (hi[acc] - lo[acc] <= 1e-12 * hi[acc]).all() and (lo[acc] > 1e7).all() and (hi[acc] < 1e8).all()
    below = np.char.startswith(name, "acc_below")
    qd[acc, hinge[acc]] = -sign[acc] * hi[acc] * np.where(below[acc], 1 - 1e-6, 1 + 1e-6)

    # pos: the displacement of one sub-step from +-1e10, then the start that lands half a displacement short of the threshold or beyond it
    pos = lanes("pos_")
    t, tq = s["qvel"].copy(), s["qpos"].copy()
    t[pos, hinge[pos]] = sign[pos] * 1e4; tq[pos, hinge[pos]] = sign[pos] * LIMIT
    _, _, p = _step_from(ora, s, tq, t, a, n)
    disp = sign * (p["qpos"][np.arange(n), hinge] - tq[np.arange(n), hinge])
    assert (disp[pos] > 1.0).all() and (disp[pos] < 16.0).all(), disp[pos]
    short = np.char.startswith(name, "pos_below")
    qd[pos, hinge[pos]] = sign[pos] * 1e4
    q[pos, hinge[pos]] = sign[pos] * (LIMIT - np.where(short[pos], 1.5, 0.5) * disp[pos])

    vel = lanes("vel")
    qd[vel, 1] = sign[vel] * 9.9e9
    assert (np.abs(q) <= LIMIT).all() and (np.abs(qd) <= LIMIT).all() and (np.abs(s["warm"]) <= LIMIT).all()      # nothing fires at the start

    fired_c, out_c, post_c = _step_from(ora, s, s["qpos"], s["qvel"], a, n)
    pre_c = {**s}
    fired, out, post = _step_from(ora, s, q, qd, a, n)
    pre = {**s, "qpos": q, "qvel": qd}
    over = lambda x: ~(np.abs(x) <= LIMIT).all(axis=1)                      # NaN counts as over
    bad_q, bad_v = over(post["qpos"]), over(post["qvel"])
    bad = fired | bad_q | bad_v
    why = np.array(["".join(c for c, m in (("a", fired[i]), ("v", bad_v[i] and not fired[i]), ("q", bad_q[i] and not fired[i])) if m) for i in range(n)])
    assert not fired_c.any() and not over(post_c["qpos"]).any() and not over(post_c["qvel"]).any()
    return dict(kind=kind, name=name, action=rp.freeze(a), pre=rp.freeze(pre), out=rp.freeze(out), post=rp.freeze(post), bad=rp.freeze(bad), why=why,
                fired=rp.freeze(fired), hinge=hinge, sign=sign, pre_clean=rp.freeze(pre_c), out_clean=rp.freeze(out_c), post_clean=rp.freeze(post_c))


def check_sides(n, r):
    """The oracle alone: every special lane lands on the side its kind names, by the array its kind names."""
    name, post, bad, why, fired, hinge, sign = (r[k] for k in ("name", "post", "bad", "why", "fired", "hinge", "sign"))
    assert not bad[r["kind"] < 0].any()
    for k in EDGE_KINDS:
        for i in np.nonzero(name == k)[0]:
            amax, x = np.abs(post["warm"][i]).max(), sign[i] * post["qpos"][i, hinge[i]]
            print(f"{n} lane {i:3d} {k:11s} oracle: bad {bool(bad[i])} through '{why[i]}'  max|qacc| {amax:.9e}  hinge position - 1e10 {x - LIMIT:+.6e}  max|qvel| {np.abs(post['qvel'][i]).max():.3e}")
            if k.startswith("acc_below"):
                assert not bad[i] and LIMIT * (1 - 3e-6) < amax < LIMIT and sign[i] * post["warm"][i, hinge[i]] == amax
            elif k.startswith("acc_above"): assert bad[i] and why[i] == "a"
            elif k.startswith("pos_below"): assert not bad[i] and LIMIT - 12.0 < x < LIMIT - 0.4 and amax < 1e9
            elif k.startswith("pos_above"): assert bad[i] and why[i] == "q" and LIMIT + 0.4 < x < LIMIT + 12.0
            else: assert bad[i] and why[i] == "a"
    # (vel: the acceleration is beyond 1e10 long before a velocity can be; no state shows qdn alone)
    assert all((name == k).sum() >= (1 if n == 65 else 2) for k in EDGE_KINDS)


def _engine_step(torch, n, pre, action):
    envs = rp.engine(n, 1, SEED)
    rp.sync_state(envs, pre)
    obs, rew, term, trunc, info = envs.step(torch.as_tensor(action.copy()))
    st = envs.get_state()
    g = dict(obs=obs["observation"].cpu().numpy(), achieved=obs["achieved_goal"].cpu().numpy(), desired=obs["desired_goal"].cpu().numpy(),
             reward=rew.cpu().numpy(), term=term.cpu().numpy(), trunc=trunc.cpu().numpy(),
             q=st["qpos"].cpu().numpy().T.copy(), v=st["qvel"].cpu().numpy().T.copy(), w=st["warm"].cpu().numpy().T.copy(),
             resets=int(envs.counters()["bad_state_resets"]))
    envs.close()
    return g


def _errors(g, out, post, lanes):
    ew, den = np.abs(g["w"][lanes] - post["warm"][lanes]).max(axis=1), np.abs(post["warm"][lanes]).max(axis=1)
    ew = np.where(den > 0, ew / np.where(den > 0, den, 1.0), ew)
    e = max(float(np.abs(g["obs"][lanes] - out["obs"][lanes]).max()), float(np.abs(g["achieved"][lanes] - out["achieved"][lanes]).max()),
            float(np.abs(g["reward"][lanes] - out["reward"][lanes]).max()))
    return dict(obs=e, q=float(np.abs(g["q"][lanes] - post["qpos"][lanes]).max()), v=float(np.abs(g["v"][lanes] - post["qvel"][lanes]).max()), w=float(ew.max()))


def measure(torch, n):
    """-> (engine's reset decision [n], the oracle's [n], resets counted, good lanes bit-identical to the clean run, errors by class of lane)."""
    r = oracle_run(n)
    check_sides(n, r)
    g = _engine_step(torch, n, r["pre"], r["action"])
    c = _engine_step(torch, n, r["pre_clean"], r["action"])
    assert c["resets"] == 0
    reset = (g["q"] == 0).all(axis=1) & (g["v"] == 0).all(axis=1) & (g["w"] == 0).all(axis=1)
    finite = all(np.isfinite(g[x]).all() for x in ("q", "v", "w", "obs"))
    ordinary = r["kind"] < 0
    same_bits = all(np.array_equal(g[x][ordinary].view(np.uint64) if g[x].dtype == np.float64 else g[x][ordinary],
                                   c[x][ordinary].view(np.uint64) if c[x].dtype == np.float64 else c[x][ordinary])
                    for x in ("q", "v", "w", "obs", "achieved", "desired", "reward", "term", "trunc"))
    cls = dict(ordinary=np.nonzero(ordinary)[0], acc_below=np.nonzero(np.char.startswith(r["name"], "acc_below"))[0],
               pos_below=np.nonzero(np.char.startswith(r["name"], "pos_below"))[0])
    err = {k: _errors(g, r["out"], r["post"], v) for k, v in cls.items()}
    err["clean"] = _errors(c, r["out_clean"], r["post_clean"], np.arange(n))
    for i in np.nonzero(r["kind"] >= 0)[0]:
        print(f"{n} lane {i:3d} {r['name'][i]:11s} engine reset {bool(reset[i])}  oracle {bool(r['bad'][i])} ('{r['why'][i]}': decided by "
              f"{'a[]' if 'a' in r['why'][i] else 'qn[]' if 'q' in r['why'][i] else 'qdn[]' if r['why'][i] else 'nothing'} in bad_value_any)")
    for k, v in err.items(): print(f"{n} {k}: " + " ".join(f"{x} {y:.3e}" for x, y in v.items()))
    print(f"{n}: resets counted {g['resets']}, oracle's bad lanes {int(r['bad'].sum())}, good lanes the clean run's bits: {same_bits}, all finite: {finite}")
    return reset, r["bad"], g["resets"], same_bits and finite, err


BOUNDS2 = {      # the env-step of two sub-steps: 100 x the parent build's worst error, as above (the new build's are the same figures)
    165: dict(ordinary=dict(obs=8.3e-14, q=5.7e-12, v=4.6e-10, w=8.9e-10),         # 8.327e-16  5.795e-14  4.619e-12  8.978e-12
              pos_above=dict(obs=3.3e-14, q=2.3e-14, v=1.1e-11, w=2.1e-10)),       # 3.331e-16  2.340e-16  1.170e-13  2.125e-12
    65: dict(ordinary=dict(obs=7.2e-14, q=8.3e-12, v=4.4e-10, w=1.3e-09),          # 7.216e-16  8.368e-14  4.491e-12  1.335e-11
             pos_above=dict(obs=3.3e-14, q=2.3e-14, v=1.1e-11, w=2.1e-10)),        # 3.331e-16  2.340e-16  1.170e-13  2.125e-12
}


@functools.lru_cache(maxsize=None)
def oracle_run2(n):
    """The same start state, the `below` lanes made ordinary, taken through an env-step of TWO sub-steps (frame_skip = 2): the lanes
    that go bad do so in the first, and the second runs from the reset state: dict(action, pre, out, post, bad1, warned)."""
    r = oracle_run(n)
    ora = rp.oracle(n, 2, SEED)
    below = np.char.find(r["name"], "below") >= 0
    pre = {k: np.where(below.reshape((-1,) + (1,) * (v.ndim - 1)), r["pre_clean"][k], v) for k, v in r["pre"].items()}
    ora.set_state(**pre)
    w0 = _warnings(ora, n)
    out = ora.step(r["action"])
    warned = _warnings(ora, n) > w0
    post = ora.get_state()
    bad1 = r["bad"] & ~below
    assert np.array_equal(warned, bad1)                                   # the oracle reset those lanes, in its first or at the start of its second step
    assert (np.abs(post["qpos"]) <= 1.0).all() and (np.abs(post["qvel"]) <= LIMIT).all()      # and nothing goes bad in the second
    return dict(action=r["action"], pre=rp.freeze(pre), out=rp.freeze(out), post=rp.freeze(post), bad1=rp.freeze(bad1), name=r["name"])


def measure2(torch, n):
    """-> (lanes that end at the reset state [n], lanes the oracle reset [n], resets counted, errors by class of lane)."""
    r = oracle_run2(n)
    envs = rp.engine(n, 2, SEED)
    rp.sync_state(envs, r["pre"])
    obs, rew, term, trunc, info = envs.step(torch.as_tensor(r["action"].copy()))
    st = envs.get_state()
    g = dict(obs=obs["observation"].cpu().numpy(), achieved=obs["achieved_goal"].cpu().numpy(), reward=rew.cpu().numpy(),
             q=st["qpos"].cpu().numpy().T.copy(), v=st["qvel"].cpu().numpy().T.copy(), w=st["warm"].cpu().numpy().T.copy())
    counted = int(envs.counters()["bad_state_resets"])
    envs.close()
    assert all(np.isfinite(g[x]).all() for x in ("q", "v", "w", "obs"))
    at_reset = (g["q"] == 0).all(axis=1) & (g["v"] == 0).all(axis=1) & (g["w"] == 0).all(axis=1)
    cls = dict(ordinary=np.nonzero(r["name"] == "")[0], pos_above=np.nonzero(np.char.startswith(r["name"], "pos_above"))[0])
    err = {k: _errors(g, r["out"], r["post"], v) for k, v in cls.items()}
    for k, v in err.items(): print(f"{n} two sub-steps, {k}: " + " ".join(f"{x} {y:.3e}" for x, y in v.items()))
    print(f"{n} two sub-steps: lanes the oracle reset {np.nonzero(r['bad1'])[0].tolist()}, lanes that END at the reset state "
          f"{np.nonzero(at_reset)[0].tolist()}, resets counted {counted}")
    return at_reset, r["bad1"], counted, err


@pytest.mark.parametrize("n", RUNS)
def test_oracle_puts_every_lane_on_its_side(n):
    check_sides(n, oracle_run(n))


@pytest.mark.parametrize("n", RUNS)
def test_reset_decision_and_state_against_the_oracle(torch_cuda, n):
    reset, bad, counted, same_bits, err = measure(torch_cuda, n)
    assert np.array_equal(reset, bad), (np.nonzero(reset != bad)[0], oracle_run(n)["name"][reset != bad])      # a boolean per lane: no tolerance
    assert counted == int(bad.sum())
    assert same_bits
    for k, b in BOUNDS[n].items():
        assert all(err[k][x] <= b[x] for x in b), (k, err[k], b)
    assert all(err["clean"][x] <= BOUNDS[n]["ordinary"][x] for x in err["clean"]), err["clean"]


@pytest.mark.parametrize("n", RUNS)
def test_reset_in_the_first_of_two_substeps(torch_cuda, n):
    """One sub-step alone cannot show WHICH check reset a lane: the env-step's tail repeats mj_checkPos / mj_checkVel on the state it
    stores (guard_robot, 36 compares), so a lane that bad_value_any missed would be reset there all the same.  Two sub-steps can: a lane
    reset by the check of the first moves on from qpos0 in the second, as the oracle's does, and ends away from the reset state; a lane
    that only the tail catches ends AT the reset state.  The `pos_above` lanes end where the oracle's end (it resets them when its
    second step starts); the `acc_above` and `vel` lanes are a sub-step behind the oracle (test_gpu_api_round2.py has the reason)."""
    at_reset, bad1, counted, err = measure2(torch_cuda, n)
    assert not at_reset.any(), np.nonzero(at_reset)[0]
    assert counted == int(bad1.sum())
    for k, b in BOUNDS2[n].items():
        assert all(err[k][x] <= b[x] for x in b), (k, err[k], b)


# ------------------------------------------------------------------------ the predicate itself, on values no state of the engine reaches
NB = 12
SPECIALS = (LIMIT, np.nextafter(LIMIT, np.inf), np.nextafter(LIMIT, 0.0), 2e10, 1e300, np.inf, np.nan)


def predicate_table():
    """[n, 49] cases for mcg_selftest_bad_value (a[12], r[12], qd_old[12], q_old[12], h) and their names.  With h = 0 the Euler chain
    hands qd_old and q_old through unchanged (where a is finite), so a value can be put into one slot of a[], qdn[] or qn[] exactly:
    1e10, its two neighbours, beyond it, +-inf, NaN, in either sign, in each of the 36 slots, the other 35 finite and below 1e10 (some
    of them near it).  With h = 0.002 the same values travel down the chain as in a sub-step (a NaN or an infinity in a[i] reaches
    qdn[i] and qn[i]).  Then opposite infinities in two joints of one array, an infinity out of the solve (r), all 36 equal, and
    finite positions whose SUM overflows or is large."""
    rng = np.random.default_rng(SEED)
    rows, names = [], []

    def base(h):
        c = np.zeros(4 * NB + 1)
        c[:NB] = rng.uniform(-1, 1, NB) * 10.0 ** rng.integers(0, 10, NB)                  # a: up to 1e9 ...
        c[NB:2 * NB] = rng.uniform(-1e3, 1e3, NB)
        c[2 * NB:3 * NB] = rng.uniform(-1, 1, NB) * 10.0 ** rng.integers(0, 10, NB)
        c[3 * NB:4 * NB] = rng.uniform(-1, 1, NB) * 10.0 ** rng.integers(0, 10, NB)
        k = rng.integers(0, NB, 3)
        c[k[0]], c[2 * NB + k[1]], c[3 * NB + k[2]] = 9.99e9, -9.99e9, 9.99e9               # ... and one of each just below the limit
        if h != 0: c[:NB] *= 1e-3; c[2 * NB:3 * NB] *= 0.5                                  # (keeps qdn, qn of the untouched slots below it)
        c[4 * NB] = h
        return c

    for h in (0.0, 0.002):
        for _ in range(8): rows.append(base(h)); names.append(f"finite h={h}")
        for arr, off in (("a", 0), ("qd_old", 2 * NB), ("q_old", 3 * NB)):
            for i in range(NB):
                for v in SPECIALS:
                    for sg in (1.0, -1.0):
                        c = base(h); c[off + i] = sg * v
                        rows.append(c); names.append(f"{arr}[{i}] = {sg * v!r} h={h}")
        for arr, off in (("a", 0), ("r", NB), ("qd_old", 2 * NB), ("q_old", 3 * NB)):
            for i, j in ((0, 1), (3, 10), (11, 6), (5, 4)):
                c = base(h); c[off + i], c[off + j] = np.inf, -np.inf
                rows.append(c); names.append(f"{arr}[{i}] = inf, {arr}[{j}] = -inf h={h}")
            c = base(h); c[off + 7] = np.inf
            rows.append(c); names.append(f"{arr}[7] = inf h={h}")
    for v in (0.0, LIMIT, -LIMIT, np.nextafter(LIMIT, np.inf), np.inf, -np.inf, np.nan, 1.7e308, 1e308):
        c = np.full(4 * NB + 1, v); c[NB:2 * NB] = 0.0; c[4 * NB] = 0.0
        rows.append(c); names.append(f"all 36 = {v!r}")
    c = base(0.0); c[3 * NB:4 * NB] = np.resize([9.9e9, 9.9e9, 9.9e9, -1.0], NB)             # a large finite sum of good positions
    rows.append(c); names.append("sum of qn = 8.9e10")
    c = base(0.0); c[3 * NB:4 * NB] = np.resize([1.7e308, -1.7e308], NB)                      # finite, beyond the limit, partial sums overflow
    rows.append(c); names.append("qn = +-1.7e308")
    c = base(0.0); c[3 * NB:4 * NB] = 1.7e308
    rows.append(c); names.append("qn = 1.7e308: the sum is inf")
    return np.ascontiguousarray(np.stack(rows)), names


def run_predicates(torch, fn, table):
    """-> (each [n], any [n], a [n, 12], qdn [n, 12], qn [n, 12]) of the entry `fn` (mcg_selftest_bad_value of some build)."""
    n = table.shape[0]
    dev = torch.device("cuda:0")
    t_in = torch.as_tensor(table, device=dev)
    state = torch.zeros((n, 2 * NB), dtype=torch.float64, device=dev)
    each, any_ = torch.full((n,), 7, dtype=torch.uint8, device=dev), torch.full((n,), 7, dtype=torch.uint8, device=dev)
    rc = fn(t_in.data_ptr(), n, state.data_ptr(), each.data_ptr(), any_.data_ptr(), None)
    torch.cuda.synchronize()
    assert rc == 0, rc
    st = state.cpu().numpy()
    return each.cpu().numpy(), any_.cpu().numpy(), table[:, :NB], st[:, :NB], st[:, NB:]


def check_predicates(torch, fn):
    """The assertions of test_one_maximum_and_one_sum_equal_36_compares, for any build's entry (profiles/r13/mutations.md runs mutants through it)."""
    table, names = predicate_table()
    each, any_, a, qdn, qn = run_predicates(torch, fn, table)
    assert set(np.unique(each)) <= {0, 1} and set(np.unique(any_)) <= {0, 1}
    with np.errstate(invalid="ignore"):
        want = ~(np.abs(np.concatenate([a, qdn, qn], axis=1)) <= LIMIT).all(axis=1)          # the definition, on the device's own values
    nan_only = want & ~(np.abs(np.nan_to_num(np.concatenate([a, qdn, qn], axis=1), nan=0.0)) > LIMIT).any(axis=1)
    at_limit = ~want & (np.abs(np.concatenate([a, qdn, qn], axis=1)) == LIMIT).any(axis=1)
    print(f"\npredicate table: {len(names)} cases, {int(want.sum())} bad, {int(nan_only.sum())} bad through NaN alone, {int(at_limit.sum())} good with a value at "
          f"exactly 1e10; the 36 compares differ from the definition in {int((each != want).sum())}, bad_value_any from the 36 compares in {int((any_ != each).sum())}")
    assert nan_only.sum() >= 36 and at_limit.sum() >= 72 and (~want).sum() >= 100
    assert np.array_equal(each.astype(bool), want), [names[i] for i in np.nonzero(each.astype(bool) != want)[0][:10]]
    assert np.array_equal(any_, each), [names[i] for i in np.nonzero(any_ != each)[0][:10]]


def test_one_maximum_and_one_sum_equal_36_compares(torch_cuda):
    """bad_value_any against the 36 bad_value calls it replaces, evaluated side by side on the device from the same registers
    (mcg_selftest_bad_value), on the table above: the two booleans are equal in every case, and the 36 compares equal the definition
    applied in numpy to the values the device returned.  This is where the NaN detector, the hardware maximum on NaN and on
    infinities, and the compare at exactly 1e10 are run; the sub-step tests above cannot reach them."""
    from mycobotgym_amd import _abi
    check_predicates(torch_cuda, _abi.load().mcg_selftest_bad_value)
