"""The picture rollout buffer without a GPU: the ABI's layout, the host refusals, and a known answer of the pixel rule
(tests/indep_rollout_img.py)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from tests.indep_rollout_img import ImageRollout, record_dtype

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_rollout_img_structs_match_header_layout(built, tmp_path):
    """sizeof / offsetof of mcg_rollout_img_buf and mcg_rollout_img_batch as the C compiler sees include/mcg.h == the ctypes mirrors."""
    from mycobotgym_amd import _abi
    buf_fields = [n for n, _ in _abi.McgRolloutImgBuf._fields_]
    batch_fields = [n for n, _ in _abi.McgRolloutImgBatch._fields_]
    exprs = (["sizeof(mcg_rollout_img_buf)", "sizeof(mcg_rollout_img_batch)"] + [f"offsetof(mcg_rollout_img_buf,{n})" for n in buf_fields]
             + [f"offsetof(mcg_rollout_img_batch,{n})" for n in batch_fields])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){'
                   + "".join(f'printf("%zu\\n",(size_t){e});' for e in exprs) + "return 0;}\n")
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([C.sizeof(_abi.McgRolloutImgBuf), C.sizeof(_abi.McgRolloutImgBatch)] + [getattr(_abi.McgRolloutImgBuf, n).offset for n in buf_fields]
            + [getattr(_abi.McgRolloutImgBatch, n).offset for n in batch_fields])
    assert got == want
    assert len(buf_fields) == 15 and len(batch_fields) == 8
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays
    for name in ("mcg_rollout_img_record_bytes", "mcg_rollout_img_start", "mcg_rollout_img_add", "mcg_rollout_img_gae", "mcg_rollout_img_carry",
                 "mcg_rollout_img_gather"):
        assert name in _abi.EXPORTS and hasattr(_abi.load(), name), name


@pytest.mark.parametrize("A", [1, 2, 3, 4, 7, 8])
def test_rollout_img_record_bytes(built, A):
    from mycobotgym_amd import _abi
    got = _abi.load().mcg_rollout_img_record_bytes(A)
    fields = 4 * (A + 1)                       # action, log_prob
    assert got % 16 == 0 and fields <= got < fields + 16
    assert got == record_dtype(A).itemsize == _abi.rollout_img_record_dtype(A).itemsize
    assert _abi.rollout_img_record_dtype(A).fields.keys() == record_dtype(A).fields.keys()
    for name, (dt, off) in {k: v[:2] for k, v in record_dtype(A).fields.items()}.items():
        assert _abi.rollout_img_record_dtype(A).fields[name][:2] == (dt, off), name


BUF_POINTERS = ("pixels", "records", "reward", "value", "episode_start", "advantage", "returns", "last_start")


def _buf(_abi, **over):
    p = C.c_void_p(0x1000)            # never dereferenced: the refusals come before any HIP call
    kw = dict({n: p for n in BUF_POINTERS}, n_envs=3, channels=2, size=5, act_dim=7, n_steps=4, gamma=0.99, gae_lambda=0.95)
    kw.update(over)
    return _abi.McgRolloutImgBuf(**kw)


def test_rollout_img_host_refusals_without_a_gpu(built):
    """Every argument check of the five calls: the code and a fragment of its message, with no GPU in the machine."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    p = C.c_void_p(0x1000)
    batch = _abi.McgRolloutImgBatch(pix=0x1000)
    ARG = _abi.MCG_ERR_ARG
    ref = lambda x: None if x is None else C.byref(x)

    def start(b, pos=0, img=p, es=25, cs=75):
        return L.mcg_rollout_img_start(ref(b), pos, img, es, cs, None, None)

    def add(b, pos=0, actions=p, values=p, log_probs=p, final_values=None, img=p, es=25, cs=75, reward=p, terminated=p, truncated=p):
        return L.mcg_rollout_img_add(ref(b), pos, actions, values, log_probs, final_values, img, es, cs, reward, terminated, truncated, None)

    def gae(b, last_values=p):
        return L.mcg_rollout_img_gae(ref(b), last_values, None)

    def carry(b, pos=4):
        return L.mcg_rollout_img_carry(ref(b), pos, None)

    def gather(b, first=0, count=4, out=batch):
        return L.mcg_rollout_img_gather(ref(b), 0, 0, first, count, ref(out), None)

    def refused(code, text):
        assert code == ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()

    for call in (start, add, gae, carry, gather):
        refused(call(None), "null mcg_rollout_img_buf")
        for name in BUF_POINTERS:
            refused(call(_buf(_abi, **{name: None})), "null pointer in mcg_rollout_img_buf")
        for name in ("n_envs", "channels", "size", "act_dim", "n_steps"):
            refused(call(_buf(_abi, **{name: 0})), "must be >= 1")
            refused(call(_buf(_abi, **{name: -4})), "must be >= 1")
        refused(call(_buf(_abi, channels=9)), "channels must be <= 8")
        refused(call(_buf(_abi, size=513)), "size must be <= 512")
        refused(call(_buf(_abi, n_envs=2 ** 20, n_steps=2 ** 11)), "below 2^31")
        refused(call(_buf(_abi, n_envs=2 ** 31 - 1, n_steps=2 ** 31 - 1)), "below 2^31")
        refused(call(_buf(_abi, pixels=C.c_void_p(0x1008))), "pixels is not 16-byte aligned")
        refused(call(_buf(_abi, records=C.c_void_p(0x1004))), "records is not 16-byte aligned")
        for name in ("gamma", "gae_lambda"):
            for bad in (float("nan"), float("inf"), -float("inf"), -0.01, 1.01):
                refused(call(_buf(_abi, **{name: bad})), "finite and in [0, 1]")
    good = _buf(_abi)
    assert L.mcg_rollout_img_carry(ref(good), 0, None) == _abi.MCG_OK          # nothing to copy: no launch, so no GPU needed either
    for call in (start, add):
        refused(call(good, pos=-1), "pos outside [0, n_steps")
        refused(call(good, img=None), "null img")
        refused(call(good, es=-25), "a stride is negative")
        refused(call(good, cs=-75), "a stride is negative")
        refused(call(good, cs=24), "chan_stride is below size * size")
        refused(call(good, cs=0), "chan_stride is below size * size")
    refused(start(good, pos=5), "pos outside [0, n_steps]")
    refused(add(good, pos=4), "pos outside [0, n_steps)")
    refused(carry(good, pos=5), "pos outside [0, n_steps]")
    refused(carry(good, pos=-1), "pos outside [0, n_steps]")
    refused(add(good, actions=None), "null actions")
    refused(add(good, values=None), "null values")
    refused(add(good, log_probs=None), "null log_probs")
    for name in ("reward", "terminated", "truncated"):
        refused(add(good, **{name: None}), "are required")
    refused(gae(good, last_values=None), "null last_values")
    refused(gather(good, first=-1), "first < 0")
    refused(gather(good, count=0), "count must be >= 1")
    refused(gather(good, count=-3), "count must be >= 1")
    refused(gather(good, first=0, count=13), "first + count > n_steps * n_envs")
    refused(gather(good, first=9, count=4), "first + count > n_steps * n_envs")
    refused(gather(good, first=12, count=1), "first + count > n_steps * n_envs")
    refused(gather(good, first=2 ** 62, count=2 ** 62), "first + count > n_steps * n_envs")
    refused(gather(good, out=None), "null mcg_rollout_img_batch")
    refused(gather(good, out=_abi.McgRolloutImgBatch()), "all outputs are null")
    assert L.mcg_rollout_img_record_bytes(0) == 0 and L.mcg_rollout_img_record_bytes(-1) == 0


def test_pixel_rule_known_answer_by_hand():
    """T = 3, N = 2, pictures of C = 1, S = 2 (4 bytes in a slot of 16), every byte of picture k equal to k.

        start (all)           picture 1 -> slot 0 of both environments
        add 0                 picture 2 -> slot 1
        start (env 1 only)    picture 9 -> slot 1 of environment 1: the write position is 1
        add 1                 picture 3 -> slot 2
        add 2                 picture 4 -> slot 3
    So environment 0 holds 1 2 3 4 and environment 1 holds 1 9 3 4; the actions of steps 0, 1, 2 were taken from slots 0, 1, 2.
    reset() copies slot 3 to slot 0: 4 2 3 4 and 4 9 3 4, and the next add writes slot 1 again."""
    T, N = 3, 2
    R = ImageRollout(N, 1, 2, 1, T, 0.5, 0.5)
    pic = lambda k: np.full((N, 1, 2, 2), k, np.uint8)
    z = lambda: np.zeros(N, np.float32)
    step = lambda k: R.add(np.zeros((N, 1), np.float32), z(), z(), pic(k), np.zeros(N), np.zeros(N, bool), np.zeros(N, bool))
    R.start(pic(1))
    step(2)
    R.start(pic(9), mask=np.array([False, True]))
    step(3)
    step(4)
    R.finish(z())
    px = R.pixels()
    assert px.shape == (T + 1, N, 16) and px.dtype == np.uint8
    assert px[:, :, 0].T.tolist() == [[1, 2, 3, 4], [1, 9, 3, 4]]
    assert (px[:, :, :4] == px[:, :, :1]).all() and (px[:, :, 4:] == 0).all()          # a picture's four bytes, then the padding
    assert R.planes()["episode_start"].T.tolist() == [[1, 0, 0], [1, 1, 0]] and R.last_start().tolist() == [0, 0]
    g = R.gather(0, 0, 0, T * N)
    assert sorted(g["index"].tolist()) == list(range(T * N))
    want = {0: 1, 1: 2, 2: 3, 3: 1, 4: 9, 5: 3}          # i = env * T + step -> the picture of its slot
    assert [int(p[0, 0, 0]) for p in g["pix"]] == [want[i] for i in g["index"].tolist()]
    assert g["pix_f32"].dtype == np.float32 and g["pix_f32"][0, 0, 0, 0] == np.float32(int(g["pix"][0, 0, 0, 0])) / np.float32(255)
    R.reset()
    assert R.pixels()[:, :, 0].T.tolist() == [[4, 2, 3, 4], [4, 9, 3, 4]]
    step(5)
    assert R.pixels()[:, :, 0].T.tolist() == [[4, 5, 3, 4], [4, 5, 3, 4]]


def test_quotient_by_255_is_not_a_product():
    """Why the kernel divides: float32(b) * float32(1 / 255) differs from float32(b) / float32(255) for some bytes b, so a product with a
    rounded reciprocal cannot be bit-identical to SB3's ``obs.float() / 255``."""
    b = np.arange(256, dtype=np.float32)
    quotient, product = b / np.float32(255), b * (np.float32(1) / np.float32(255))
    print(f"{int((quotient != product).sum())} of 256 byte values differ")          # 126
    assert (quotient != product).sum() >= 1
    exact = np.arange(256, dtype=np.float64) / 255.0
    assert np.array_equal(quotient, exact.astype(np.float32))          # the double's 53 bits settle the float32 rounding of b / 255
