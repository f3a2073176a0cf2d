"""Frame stacking without a GPU: the new entries are exported, every host refusal of both, the rules of tests/indep_frame_stack.py with
k = 1 against the unstacked rule and on a case worked by hand, and the census of the inputs that tests/test_gpu_frame_stack.py samples."""
import ctypes as C

import numpy as np
import pytest

from tests.indep_frame_stack import StackedReplay, StackRule
from tests.indep_replay_img import ImageReplay
from tests.test_replay_img_cpu import BUF_POINTERS, DIMS, _buf

NAMES = ("mcg_replay_img_sample_stacked", "mcg_frame_stack_push")


def test_entries_are_exported(built):
    from mycobotgym_amd import FrameStack, _abi  # noqa: F401
    for name in NAMES:
        assert name in _abi.EXPORTS and hasattr(_abi.load(), name), name
    assert _abi.ABI_VERSION == 8 and _abi.load().mcg_abi_version() == 8          # additive: the version stays


def _refused(L, ARG):
    def refused(code, text):
        assert code == ARG, (code, L.mcg_last_error())
        assert text.encode() in L.mcg_last_error(), L.mcg_last_error()
    return refused


def test_sample_stacked_host_refusals_without_a_gpu(built):
    """Its own two refusals and every refusal of mcg_replay_img_sample: the code and a fragment of the message, with no GPU."""
    from mycobotgym_amd import _abi
    L = _abi.load()
    refused = _refused(L, _abi.MCG_ERR_ARG)
    batch = _abi.McgReplayImgBatch(pix=0x1000)
    ref = lambda x: None if x is None else C.byref(x)

    def sample(b, n_written=3, batch_size=4, k=2, out=batch):
        return L.mcg_replay_img_sample_stacked(ref(b), n_written, 0, 0, batch_size, k, ref(out), None)

    refused(sample(None), "null mcg_replay_img_buf")
    for name in BUF_POINTERS:
        refused(sample(_buf(_abi, **{name: None})), "null pointer in mcg_replay_img_buf")
    for name in DIMS:
        refused(sample(_buf(_abi, **{name: 0})), "must be >= 1")
        refused(sample(_buf(_abi, **{name: -4})), "must be >= 1")
    refused(sample(_buf(_abi, channels=9)), "channels must be <= 8")
    refused(sample(_buf(_abi, size=513)), "size must be <= 512")
    refused(sample(_buf(_abi, n_envs=2 ** 20, capacity=2 ** 11 - 1)), "(capacity + 1) * n_envs must be below 2^31")
    refused(sample(_buf(_abi, pixels=C.c_void_p(0x1008))), "pixels is not 16-byte aligned")
    refused(sample(_buf(_abi, finals=C.c_void_p(0x1001))), "finals is not 16-byte aligned")
    refused(sample(_buf(_abi, records=C.c_void_p(0x1004))), "records is not 16-byte aligned")
    good = _buf(_abi)          # capacity 4
    for k in (0, -1, 9, 100):
        refused(sample(good, k=k), "frame_stack must be in [1, 8]")
    for k in (5, 6, 8):
        refused(sample(good, k=k), "capacity - (frame_stack - 1) must be >= 1")
    refused(sample(_buf(_abi, capacity=1), k=2), "capacity - (frame_stack - 1) must be >= 1")
    refused(sample(good, n_written=-1), "n_written < 0")
    refused(sample(good, n_written=0), "empty")
    refused(sample(good, batch_size=0), "batch must be >= 1")
    refused(sample(good, out=None), "null mcg_replay_img_batch")
    refused(sample(good, out=_abi.McgReplayImgBatch()), "all outputs are null")


def test_push_host_refusals_without_a_gpu(built):
    from mycobotgym_amd import _abi
    L = _abi.load()
    refused = _refused(L, _abi.MCG_ERR_ARG)
    p, q = C.c_void_p(0x1000), C.c_void_p(0x9000)          # never dereferenced: the refusals come before any HIP call

    def push(stack=p, final_stack=q, n=3, channels=2, size=5, k=4, img=p, es=25, cs=75, final_img=p, fes=25, fcs=75, done=p, mask=None):
        return L.mcg_frame_stack_push(stack, final_stack, n, channels, size, k, img, es, cs, final_img, fes, fcs, done, mask, None)

    refused(push(stack=None), "null stack")
    for name in ("n", "channels", "size"):
        refused(push(**{name: 0}), "n_envs, channels and size must be >= 1")
        refused(push(**{name: -2}), "n_envs, channels and size must be >= 1")
    refused(push(channels=9), "channels must be <= 8")
    refused(push(size=513), "size must be <= 512")
    for k in (0, -1, 9):
        refused(push(k=k), "frame_stack must be in [1, 8]")
    refused(push(n=2 ** 31 - 1, channels=8, size=512), "must be below 2^31")
    refused(push(final_stack=p), "final_stack is stack")
    refused(push(done=None), "null done without a mask")
    refused(push(img=None), "null img")
    refused(push(final_img=None), "null final_img")
    refused(push(es=-25), "a stride is negative")
    refused(push(cs=-75), "a stride is negative")
    refused(push(cs=24), "chan_stride is below size * size")
    refused(push(fes=-25), "a stride is negative")
    refused(push(fcs=24), "chan_stride is below size * size")


# ---------------------------------------------------------------------------------------------------------------- rules
def _random_run(R, rng, N, C, S, A, steps, Tm):
    """Random episodes (lengths 1 .. Tm; exactly Tm: the time limit) with a masked start before step 12, into R."""
    pic = lambda: rng.integers(0, 256, (N, C, S, S), dtype=np.uint8)
    R.start(pic())
    left, age = rng.integers(1, Tm + 1, N), np.zeros(N, int)
    for i in range(steps):
        if i == 12:
            mask = rng.random(N) < 0.4
            R.start(pic(), mask)
            left[mask], age[mask] = rng.integers(1, Tm + 1, int(mask.sum())), 0
        left -= 1
        age += 1
        done = left == 0
        truncated = done & (age == Tm)
        R.add(rng.uniform(-1, 1, (N, A)).astype(np.float32), pic(), pic(), rng.normal(size=N), done & ~truncated, truncated)
        left[done], age[done] = rng.integers(1, Tm + 1, int(done.sum())), 0


def test_rule_with_one_frame_is_the_unstacked_rule():
    N, C, S, A, K, Tm = 5, 2, 3, 2, 6, 4
    plain, stacked = ImageReplay(N, C, S, A, K, Tm), StackedReplay(N, C, S, A, K, Tm, 1)
    _random_run(plain, np.random.default_rng(3), N, C, S, A, 15, Tm)
    _random_run(stacked, np.random.default_rng(3), N, C, S, A, 15, Tm)
    a, b = plain.sample(2, 5, 64), stacked.sample(2, 5, 64)
    for name, v in a.items():
        assert np.array_equal(v, b[name]), name
    assert np.array_equal(b["row"], a["index"][:, 0]) and (b["depth"] == 1).all() and (a["draws"] > 1).any()


def test_rules_known_answer_by_hand():
    """N = 1, C = 1, S = 1, k = 3, K = 4, Tm = 3: every picture one byte.

        reset -> 10                    stack (0, 0, 10)
        step 0 -> 11                   (0, 10, 11)
        step 1 -> 12                   (10, 11, 12)
        step 2 -> 13, time limit, the episode's last picture 99: final stack (11, 12, 99), stack (0, 0, 13)
        step 3 -> 14, terminated       final stack (0, 13, 14) (the env hands one out at every step), stack (0, 0, 14)
        step 4 -> 15                   (0, 14, 15)
    Transitions 1 .. 4 are sampleable: 1: (0, 10, 11) -> (10, 11, 12); 2: (10, 11, 12) -> (11, 12, 99), done 0, from the finals;
    3: (0, 0, 13) -> (0, 0, 14), done 1; 4: (0, 0, 14) -> (0, 14, 15)."""
    rule = StackRule(1, 1, 1, 3)
    px = lambda b: np.full((1, 1, 1, 1), b, np.uint8)
    flat = lambda s: s.reshape(-1).tolist()
    assert flat(rule.reset(px(10))) == [0, 0, 10]
    assert [flat(x) for x in rule.step(px(11), px(0), [False])] == [[0, 10, 11], [0, 10, 0]]
    assert [flat(x) for x in rule.step(px(12), px(0), [False])] == [[10, 11, 12], [10, 11, 0]]
    assert [flat(x) for x in rule.step(px(13), px(99), [True])] == [[0, 0, 13], [11, 12, 99]] and rule.depth[0] == 1
    assert [flat(x) for x in rule.step(px(14), px(14), [True])] == [[0, 0, 14], [0, 13, 14]]
    assert [flat(x) for x in rule.step(px(15), px(0), [False])] == [[0, 14, 15], [0, 14, 0]] and rule.depth[0] == 2
    R = StackedReplay(1, 1, 1, 1, 4, 3, 3)
    no, yes = np.zeros(1, bool), np.ones(1, bool)
    R.start(px(10))
    for a, (nxt, final, term, trunc) in enumerate([(11, 0, no, no), (12, 0, no, no), (13, 99, no, yes), (14, 14, yes, yes), (15, 0, no, no)]):
        R.add(np.full((1, 1), a, np.float32), px(nxt), px(final), np.zeros(1), term, trunc)
    o = R.sample(1, 0, 64)
    want = {1: ([0, 10, 11], [10, 11, 12], 0.0, 0, 2), 2: ([10, 11, 12], [11, 12, 99], 0.0, 1, 3), 3: ([0, 0, 13], [0, 0, 14], 1.0, 0, 1),
            4: ([0, 0, 14], [0, 14, 15], 0.0, 0, 1)}          # time -> stack, next stack, done, source, depth
    for i in range(64):
        a = int(o["time"][i])
        got = (flat(o["pix"][i]), flat(o["next_pix"][i]), float(o["done"][i, 0]), int(o["index"][i, 2]), int(o["depth"][i]))
        assert got == want[a], (a, got)
        assert o["row"][i] == a % 7 and o["index"][i, 0] == a % 5
    assert set(o["time"].tolist()) == set(want) and R.wide.F == 3


@pytest.mark.parametrize("k", [2, 4])
def test_census_of_the_sampled_inputs(k):
    """The sampling seed on the synthetic schedule (seed 1: seed 0 gives no sample across row 0 for k = 4): no give-up, >= 10 sampled timeouts whose next stack comes from the finals, >= 10 sampled
    terminations, >= 10 samples at every depth 1 .. k, a sample whose history lies in the k - 1 rows older than the sampling window, one
    whose history crosses the ring's row 0, and one that needed more than one draw.  The schedule and the draws do not depend on the
    picture's shape: the smallest shape stands for all four."""
    from tests.test_gpu_frame_stack import SEED, assert_census, census, stacked_snapshots
    c = census(stacked_snapshots(2, 5, k), k)
    print(f"seed {SEED}, k = {k}: {c}")
    assert_census(c, k)
    assert c["lost"] == 0
