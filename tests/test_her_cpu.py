"""The hindsight replay buffer without a GPU: the ABI's layout, the host refusals, and known answers of the rule (tests/indep_her.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.indep_her import History, record_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_her_structs_match_header_layout(built, tmp_path):
    """sizeof / offsetof of mcg_her_buf and mcg_her_batch as the C compiler sees include/mcg.h == the ctypes mirrors."""
    from mycobotgym_amd import _abi
    buf_fields = [n for n, _ in _abi.McgHerBuf._fields_]
    batch_fields = [n for n, _ in _abi.McgHerBatch._fields_]
    exprs = (["sizeof(mcg_her_buf)", "sizeof(mcg_her_batch)"] + [f"offsetof(mcg_her_buf,{n})" for n in buf_fields]
             + [f"offsetof(mcg_her_batch,{n})" for n in batch_fields])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_abi.McgHerBuf), C.sizeof(_abi.McgHerBatch)] + [getattr(_abi.McgHerBuf, n).offset for n in buf_fields]
            + [getattr(_abi.McgHerBatch, n).offset for n in batch_fields])
    assert got == want
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays


@pytest.mark.parametrize("D,A", [(10, 7), (25, 7), (25, 4), (25, 8)])
def test_record_bytes(built, D, A):
    from mycobotgym_amd import _abi
    got = _abi.load().mcg_her_record_bytes(D, A)
    fields = 4 * (2 * D + A) + 3 * 3 * 8 + 4 + 1 + 4 + 4          # obs, next_obs, action; the goals; reward, terminated, t_in_ep, ep_len
    assert got % 16 == 0 and got >= fields
    assert got == record_dtype(D, A).itemsize == _abi.her_record_dtype(D, A).itemsize
    assert _abi.her_record_dtype(D, A).fields.keys() == record_dtype(D, A).fields.keys()
    for name, (dt, off) in {k: v[:2] for k, v in record_dtype(D, A).fields.items()}.items():
        assert _abi.her_record_dtype(D, A).fields[name][:2] == (dt, off), name


def _buf(_abi, **over):
    p = C.c_void_p(0x1000)            # never dereferenced: the refusals come before any HIP call
    kw = dict(records=p, t_run=p, last_obs=p, last_achieved=p, counters=p, n_envs=3, obs_dim=25, act_dim=7, capacity=8,
              max_episode_steps=3, reward_type=_abi.REWARD_DENSE, distance_threshold=0.05)
    kw.update(over)
    return _abi.McgHerBuf(**kw)


def test_host_refusals_without_a_gpu(built):
    """Every argument check of the three calls: the code and its message, with no GPU in the machine."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = C.c_void_p(0x1000)
    step = _abi.McgStepOut(**{n: 0x1000 for n, _ in _abi.McgStepOut._fields_})
    batch = _abi.McgHerBatch()
    ARG, UNS = _abi.MCG_ERR_ARG, _abi.MCG_ERR_UNSUPPORTED

    def start(b, first=step):
        return L.mcg_her_start(None if b is None else C.byref(b), None if first is None else C.byref(first), None, None)

    def add(b, n=0, actions=p, out=step):
        return L.mcg_her_add(None if b is None else C.byref(b), n, actions, None if out is None else C.byref(out), None)

    def sample(b, n=5, batch_size=4, n_virtual=3, out=batch):
        return L.mcg_her_sample(None if b is None else C.byref(b), n, 0, 0, batch_size, n_virtual, None if out is None else C.byref(out), None)

    def refused(code, want, text):
        assert code == want, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    for call in (start, add, sample):
        refused(call(None), ARG, "null mcg_her_buf")
        for name in ("records", "t_run", "last_obs", "last_achieved", "counters"):
            refused(call(_buf(_abi, **{name: None})), ARG, "null pointer in mcg_her_buf")
        for name in ("n_envs", "obs_dim", "act_dim"):
            refused(call(_buf(_abi, **{name: 0})), ARG, "must be >= 1")
            refused(call(_buf(_abi, **{name: -4})), ARG, "must be >= 1")
        refused(call(_buf(_abi, max_episode_steps=0)), ARG, "max_episode_steps must be >= 1")
        refused(call(_buf(_abi, capacity=5)), ARG, "capacity < 2 * max_episode_steps")
        refused(call(_buf(_abi, capacity=0)), ARG, "capacity < 2 * max_episode_steps")
        refused(call(_buf(_abi, records=C.c_void_p(0x1008))), ARG, "not 16-byte aligned")
    good = _buf(_abi)
    refused(start(good, first=None), ARG, "null mcg_step_out")
    refused(start(good, first=_abi.McgStepOut(obs=0x1000)), ARG, "obs and achieved_goal")
    refused(add(good, n=-1), ARG, "n_written < 0")
    refused(add(good, actions=None), ARG, "null actions")
    refused(add(good, out=None), ARG, "null mcg_step_out")
    for name in ("obs", "achieved_goal", "desired_goal", "reward", "terminated", "truncated", "final_obs", "final_achieved", "final_desired"):
        out = _abi.McgStepOut(**{n: (None if n == name else 0x1000) for n, _ in _abi.McgStepOut._fields_})
        refused(add(good, out=out), ARG, "are required")
    refused(sample(good, n=-1), ARG, "n_written < 0")
    refused(sample(good, batch_size=0), ARG, "batch must be >= 1")
    refused(sample(good, n_virtual=-1), ARG, "n_virtual outside [0, batch]")
    refused(sample(good, n_virtual=5), ARG, "n_virtual outside [0, batch]")
    refused(sample(good, out=None), ARG, "null mcg_her_batch")
    refused(sample(_buf(_abi, reward_type=_abi.REWARD_SHAPING)), UNS, "reward_shaping")
    assert L.mcg_her_record_bytes(0, 7) == 0 and L.mcg_her_record_bytes(25, 0) == 0


# ---- known answers of the rule, on a hand-written history: 3 environments, capacity 8, time limit 3.
# done flags per insertion (rows) and environment (columns); episode lengths env 0: 3 3 3 (2 in flight), env 1: 2 1 3 2 3,
# env 2: 1 3 1 3 2 (1 in flight)
DONE = np.array([[0, 0, 1], [0, 1, 0], [1, 1, 0], [0, 0, 1], [0, 0, 1], [1, 1, 0], [0, 0, 0], [0, 1, 1], [1, 0, 0], [0, 0, 1], [0, 1, 0]], dtype=bool)


def _hand_history(n_insertions):
    N, D, A = 3, 2, 1
    rng = np.random.default_rng(5)
    H = History(N, D, A, capacity=8, max_steps=3)
    H.start(rng.normal(size=(N, D)), rng.normal(size=(N, 3)))
    for i in range(n_insertions):
        out = {k: rng.normal(size=(N, 3)) for k in ("achieved_goal", "desired_goal", "final_achieved", "final_desired")}
        out.update(obs=rng.normal(size=(N, D)), final_obs=rng.normal(size=(N, D)), reward=rng.normal(size=N),
                   truncated=DONE[i], terminated=DONE[i] & (rng.random(N) < 0.5))
        H.add(rng.uniform(-1, 1, (N, A)).astype(np.float32), out)
    return H


def test_rule_valid_pairs_known_answers():
    """Which (slot, env) may be sampled, worked out by hand.  After 11 insertions the ring holds times 3..10 (slot = time % 8): env 2's
    episode 1-3 has lost its start, so its slot 3 is out although that transition is still stored; episodes in flight are out."""
    want5 = {(s, 0) for s in (0, 1, 2)} | {(s, 1) for s in (0, 1, 2)} | {(s, 2) for s in (0, 1, 2, 3, 4)}
    want8 = {(s, 0) for s in range(6)} | {(s, 1) for s in range(8)} | {(s, 2) for s in range(8)}
    want11 = {(s, 0) for s in (0, 3, 4, 5, 6, 7)} | {(s, 1) for s in range(8)} | {(s, 2) for s in (0, 1, 4, 5, 6, 7)}
    for n, want in ((5, want5), (8, want8), (11, want11)):
        H = _hand_history(n)
        assert H.valid_pairs() == want, n
        R = H.ring()              # the same from the record fields, as the kernel decides it
        got = {(s, e) for s in range(8) for e in range(3)
               if R[s, e]["ep_len"] > 0 and (n - 1 - ((n % 8 - 1 - s) % 8)) - R[s, e]["t_in_ep"] >= max(0, n - 8) and s < min(n, 8)}
        assert got == want, n
        assert H.overlong == 0


def test_rule_sampling_known_properties():
    H = _hand_history(11)
    valid = H.valid_pairs()
    batch, n_virtual = 200, int(200 * (1 - 1 / 5))
    assert n_virtual == 160
    o = H.sample(seed=3, call=1, batch=batch, n_virtual=n_virtual)
    assert (o["draws"] <= 64).all()
    assert all((int(s), int(e)) in valid for s, e in o["index"][:, :2])
    virtual = o["index"][:, 2] >= 0
    assert virtual.sum() == n_virtual and not virtual[:batch - n_virtual].any() and virtual[batch - n_virtual:].all()
    # a future step is never before the current one or past the episode's end, and both ends occur
    f, t, L = o["future"][virtual], o["step"][virtual], o["length"][virtual]
    assert (f >= t).all() and (f <= L - 1).all()
    assert (f == t).any() and (f == L - 1).any() and (f > t).any()
    # the future slot lies f - t insertions after the sample's own
    assert ((o["index"][virtual, 0] + (f - t)) % 8 == o["index"][virtual, 2]).all()
    # another call word, other draws; the same call, the same batch
    assert not np.array_equal(H.sample(3, 2, batch, n_virtual)["index"], o["index"])
    assert np.array_equal(H.sample(3, 1, batch, n_virtual)["index"], o["index"])
    # every valid pair turns up (22 valid pairs, 200 uniform draws among them)
    assert {(int(s), int(e)) for s, e in o["index"][:, :2]} == valid


def test_rule_gives_up_and_counts_overlong():
    N, D, A = 3, 2, 1
    H = History(N, D, A, capacity=8, max_steps=3)
    z = {k: np.zeros((N, 3)) for k in ("achieved_goal", "desired_goal", "final_achieved", "final_desired")}
    z.update(obs=np.zeros((N, D)), final_obs=np.zeros((N, D)), reward=np.zeros(N), truncated=np.zeros(N, bool), terminated=np.zeros(N, bool))
    H.start(np.zeros((N, D)), np.zeros((N, 3)))
    for _ in range(2):
        H.add(np.zeros((N, A), np.float32), z)
    o = H.sample(0, 0, 16, 12)
    assert (o["index"] == -1).all() and (o["draws"] == 257).all() and H.overlong == 0
    for _ in range(3):
        H.add(np.zeros((N, A), np.float32), z)
    assert H.overlong == N and H.valid_pairs() == set()
    assert (H.ring()["t_in_ep"][:5, 0] == [0, 1, 2, 3, 3]).all() and (H.ring()["ep_len"] == 0).all()
