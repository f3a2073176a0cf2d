"""The picture replay buffer without a GPU: the ABI's layout, the host refusals, a known answer of the rule (tests/indep_replay_img.py)
worked by hand, and the argument that no live final picture is overwritten."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.indep_replay_img import MAX_DRAWS, NO_NEXT, TERMINATED, TIMEOUT, ImageReplay, record_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("mcg_replay_img_record_bytes", "mcg_replay_img_start", "mcg_replay_img_add", "mcg_replay_img_sample")


def test_replay_img_structs_match_header_layout(built, tmp_path):
    """sizeof / offsetof of mcg_replay_img_buf and mcg_replay_img_batch as the C compiler sees include/mcg.h == the ctypes mirrors."""
    from mycobotgym_amd import _abi
    buf_fields = [n for n, _ in _abi.McgReplayImgBuf._fields_]
    batch_fields = [n for n, _ in _abi.McgReplayImgBatch._fields_]
    exprs = (["sizeof(mcg_replay_img_buf)", "sizeof(mcg_replay_img_batch)"] + [f"offsetof(mcg_replay_img_buf,{n})" for n in buf_fields]
             + [f"offsetof(mcg_replay_img_batch,{n})" for n in batch_fields])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_abi.McgReplayImgBuf), C.sizeof(_abi.McgReplayImgBatch)] + [getattr(_abi.McgReplayImgBuf, n).offset for n in buf_fields]
            + [getattr(_abi.McgReplayImgBatch, n).offset for n in batch_fields])
    assert got == want
    assert len(buf_fields) == 11 and len(batch_fields) == 8
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays
    for name in NAMES:
        assert name in _abi.EXPORTS and hasattr(_abi.load(), name), name
    assert (_abi.REPLAY_IMG_TERMINATED, _abi.REPLAY_IMG_TIMEOUT, _abi.REPLAY_IMG_NO_NEXT) == (TERMINATED, TIMEOUT, NO_NEXT) == (1, 2, 4)


@pytest.mark.parametrize("A", [1, 2, 3, 4, 7, 8])
def test_replay_img_record_bytes(built, A):
    from mycobotgym_amd import _abi
    got = _abi.load().mcg_replay_img_record_bytes(A)
    fields = 4 * (A + 2)                       # action, reward, flags
    assert got % 16 == 0 and fields <= got < fields + 16
    assert got == record_dtype(A).itemsize == _abi.replay_img_record_dtype(A).itemsize
    assert _abi.replay_img_record_dtype(A).fields.keys() == record_dtype(A).fields.keys()
    for name, (dt, off) in {k: v[:2] for k, v in record_dtype(A).fields.items()}.items():
        assert _abi.replay_img_record_dtype(A).fields[name][:2] == (dt, off), name


BUF_POINTERS = ("pixels", "finals", "final_time", "records", "counters")
DIMS = ("n_envs", "channels", "size", "act_dim", "capacity", "max_episode_steps")


def _buf(_abi, **over):
    p = C.c_void_p(0x1000)            # never dereferenced: the refusals come before any HIP call
    kw = dict({n: p for n in BUF_POINTERS}, n_envs=3, channels=2, size=5, act_dim=7, capacity=4, max_episode_steps=3)
    kw.update(over)
    return _abi.McgReplayImgBuf(**kw)


def test_replay_img_host_refusals_without_a_gpu(built):
    """Every argument check of the three calls: the code and a fragment of its message, with no GPU in the machine."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = C.c_void_p(0x1000)
    batch = _abi.McgReplayImgBatch(pix=0x1000)
    ARG = _abi.MCG_ERR_ARG
    ref = lambda x: None if x is None else C.byref(x)

    def start(b, n_written=0, img=p, es=25, cs=75):
        return L.mcg_replay_img_start(ref(b), n_written, img, es, cs, None, None)

    def add(b, n_written=0, actions=p, img=p, es=25, cs=75, final_img=p, fes=25, fcs=75, reward=p, terminated=p, truncated=p):
        return L.mcg_replay_img_add(ref(b), n_written, actions, img, es, cs, final_img, fes, fcs, reward, terminated, truncated, None)

    def sample(b, n_written=3, batch_size=4, out=batch):
        return L.mcg_replay_img_sample(ref(b), n_written, 0, 0, batch_size, ref(out), None)

    def refused(code, text):
        assert code == ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    for call in (start, add, sample):
        refused(call(None), "null mcg_replay_img_buf")
        for name in BUF_POINTERS:
            refused(call(_buf(_abi, **{name: None})), "null pointer in mcg_replay_img_buf")
        for name in DIMS:
            refused(call(_buf(_abi, **{name: 0})), "must be >= 1")
            refused(call(_buf(_abi, **{name: -4})), "must be >= 1")
        refused(call(_buf(_abi, channels=9)), "channels must be <= 8")
        refused(call(_buf(_abi, size=513)), "size must be <= 512")
        refused(call(_buf(_abi, n_envs=2 ** 20, capacity=2 ** 11 - 1)), "(capacity + 1) * n_envs must be below 2^31")
        refused(call(_buf(_abi, n_envs=2 ** 31 - 1, capacity=2 ** 31 - 1)), "below 2^31")
        refused(call(_buf(_abi, pixels=C.c_void_p(0x1008))), "pixels is not 16-byte aligned")
        refused(call(_buf(_abi, finals=C.c_void_p(0x1001))), "finals is not 16-byte aligned")
        refused(call(_buf(_abi, records=C.c_void_p(0x1004))), "records is not 16-byte aligned")
        refused(call(_buf(_abi), n_written=-1), "n_written < 0")
    good = _buf(_abi)
    for call in (start, add):
        refused(call(good, img=None), "null img")
        refused(call(good, es=-25), "a stride is negative")
        refused(call(good, cs=-75), "a stride is negative")
        refused(call(good, cs=24), "chan_stride is below size * size")
        refused(call(good, cs=0), "chan_stride is below size * size")
    refused(add(good, final_img=None), "null final_img")
    refused(add(good, fes=-25), "a stride is negative")
    refused(add(good, fcs=-75), "a stride is negative")
    refused(add(good, fcs=24), "chan_stride is below size * size")
    refused(add(good, actions=None), "null actions")
    for name in ("reward", "terminated", "truncated"):
        refused(add(good, **{name: None}), "are required")
    refused(sample(good, n_written=0), "empty")
    refused(sample(good, batch_size=0), "batch must be >= 1")
    refused(sample(good, batch_size=-3), "batch must be >= 1")
    refused(sample(good, out=None), "null mcg_replay_img_batch")
    refused(sample(good, out=_abi.McgReplayImgBatch()), "all outputs are null")
    assert L.mcg_replay_img_record_bytes(0) == 0 and L.mcg_replay_img_record_bytes(-1) == 0


def test_rule_known_answer_by_hand():
    """K = 4 (five rows), N = 2, Tm = 3 (F = 3), pictures of C = 1, S = 2 (4 bytes in a slot of 16), every byte of picture k equal to k.

        start (all)           picture 10
        add 0                 the step returns 11
        add 1                 12
        add 2                 13; in environment 0 the time limit ends the episode: its last picture is 99, 13 is the next episode's first
        start (env 1 only)    picture 50: environment 1 was in mid-episode, its transition 2 has lost its next picture
        add 3                 14
        add 4                 15; environment 1 terminates: 15 is its next episode's first picture
        add 5                 16
    Six adds: the ring has wrapped, the live transitions are 2 .. 5 (transitions 0 and 1 are gone).
        environment 0    2: 12 -> 99 (the final picture), done 0    3: 13 -> 14    4: 14 -> 15    5: 15 -> 16
        environment 1    2: never sampled                            3: 50 -> 14    4: 14 -> 15, done 1 (the post-reset picture)    5: 15 -> 16
    """
    K, N, Tm = 4, 2, 3
    R = ImageReplay(N, 1, 2, 1, K, Tm)
    assert R.F == 3 and R.P == 16
    pic = lambda k: np.full((N, 1, 2, 2), k, np.uint8)
    no = np.zeros(N, bool)

    def step(a, k, terminated=no, truncated=no, final=0):
        R.add(np.full((N, 1), a, np.float32), pic(k), pic(final), np.full(N, 0.5 * a), terminated, truncated)

    R.start(pic(10))
    step(0, 11)
    step(1, 12)
    step(2, 13, truncated=np.array([True, False]), final=99)
    R.start(pic(50), mask=np.array([False, True]))
    step(3, 14)
    step(4, 15, terminated=np.array([False, True]), truncated=np.array([False, True]))          # the engine sets both: not a timeout
    step(5, 16)
    arr = R.arrays()
    px = arr["pixels"]
    assert px.shape == (K + 1, N, 16) and px.dtype == np.uint8
    assert px[:, :, 0].T.tolist() == [[15, 16, 12, 13, 14], [15, 16, 12, 50, 14]]          # times 5 6 2 3 4: the ring has wrapped
    assert (px[:, :, :4] == px[:, :, :1]).all() and (px[:, :, 4:] == 0).all()               # a picture's four bytes, then the padding
    assert arr["final_time"].tolist() == [[2, -1], [-1, -1], [-1, -1]]
    assert arr["finals"][0, 0, :4].tolist() == [99] * 4 and arr["finals"].sum() == 4 * 99
    assert arr["records"]["flags"].T.tolist() == [[0, 0, TIMEOUT, 0, 0], [0, 0, NO_NEXT, 0, TERMINATED]]
    assert arr["records"]["action"][:, 0, 0].tolist() == [5, 1, 2, 3, 4] and arr["records"]["reward"][2, 1] == np.float32(1.0)
    want = {(0, 2): (12, 99, 0.0, 1), (0, 3): (13, 14, 0.0, 0), (0, 4): (14, 15, 0.0, 0), (0, 5): (15, 16, 0.0, 0),
            (1, 3): (50, 14, 0.0, 0), (1, 4): (14, 15, 1.0, 0), (1, 5): (15, 16, 0.0, 0)}          # (env, time) -> picture, successor, done, source
    o = R.sample(seed=7, call=0, batch=200)
    seen = set()
    for k in range(200):
        e, a = int(o["index"][k, 1]), int(o["time"][k])
        assert o["index"][k, 0] == a % (K + 1)
        got = (int(o["pix"][k, 0, 0, 0]), int(o["next_pix"][k, 0, 0, 0]), float(o["done"][k, 0]), int(o["index"][k, 2]))
        assert got == want[(e, a)], (e, a)          # (1, 2) is no key: never sampled
        assert o["action"][k, 0] == a and o["reward"][k, 0] == np.float32(0.5 * a)
        assert (o["pix"][k] == o["pix"][k, 0, 0, 0]).all() and (o["next_pix"][k] == o["next_pix"][k, 0, 0, 0]).all()
        seen.add((e, a))
    assert seen == set(want)                        # each of the seven, among 200 uniform samples
    assert o["give_ups"] == 0 and o["lost"] == 0 and o["draws"].max() > 1 and o["draws"].min() == 1
    assert o["pix_f32"].dtype == np.float32 and o["pix_f32"][0, 0, 0, 0] == np.float32(int(o["pix"][0, 0, 0, 0])) / np.float32(255)


def test_rule_gives_up_when_every_transition_lost_its_next_picture():
    R = ImageReplay(2, 1, 2, 1, 4, 3)
    pic = lambda k: np.full((2, 1, 2, 2), k, np.uint8)
    R.start(pic(1))
    R.add(np.zeros((2, 1), np.float32), pic(2), pic(0), np.zeros(2), np.zeros(2, bool), np.zeros(2, bool))
    R.start(pic(3))
    o = R.sample(0, 0, 5)
    assert o["give_ups"] == 5 and (o["draws"] == MAX_DRAWS + 1).all() and (o["index"] == -1).all()
    assert not o["pix"].any() and not o["next_pix"].any() and not o["done"].any() and not o["action"].any()


@pytest.mark.parametrize("K", [4, 5, 11])          # Tm - 1, Tm, 2 Tm + 1
def test_no_live_final_picture_is_overwritten(K):
    """The collision argument itself: over random episode streams whose time-limit ends are at least Tm apart (an episode runs to
    exactly Tm steps or ends earlier by termination; masked starts cut some short), at every time every timeout among the K newest
    transitions still has its final picture, with F = ceil(K / Tm) + 1 places."""
    Tm, N, steps = 5, 6, 160
    rng = np.random.default_rng(K)
    R = ImageReplay(N, 1, 1, 1, K, Tm)
    byte = lambda: rng.integers(0, 256, (N, 1, 1, 1), dtype=np.uint8)
    R.start(byte())
    left = rng.integers(1, Tm + 1, N)
    age = np.zeros(N, int)
    timeouts = checked = 0
    for n in range(steps):
        if n % 11 == 7:
            mask = rng.random(N) < 0.3
            R.start(byte(), mask)
            left[mask], age[mask] = rng.integers(1, Tm + 1, int(mask.sum())), 0
        left -= 1
        age += 1
        done = left == 0
        truncated = done & (age == Tm)              # the time limit, at exactly Tm steps since the last reset
        terminated = done & ~truncated
        assert not (truncated & (age < Tm)).any()
        R.add(np.zeros((N, 1), np.float32), byte(), byte(), np.zeros(N), terminated, truncated)
        timeouts += int(truncated.sum())
        left[done], age[done] = rng.integers(1, Tm + 1, int(done.sum())), 0
        for e in range(N):
            for a in range(max(0, R.n - K), R.n):
                if R.steps[e][a]["timeout"]:
                    checked += 1
                    assert R.final_alive(e, a), (K, e, a, R.n)
        assert R.sample(1, n, 8)["lost"] == 0
    print(f"K = {K}: {timeouts} time-limit ends, {checked} live (transition, time) pairs checked")
    assert timeouts >= 20 and checked >= timeouts
    stamps = R.arrays()["final_time"]
    assert stamps.shape == (-(-K // Tm) + 1, N) and (stamps >= 0).sum() >= 2
