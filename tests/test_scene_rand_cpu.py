"""Per-environment scenes and their draw, the pieces that need no GPU: the numpy restatement of the draw (tests/indep_scene_rand.py)
against the published Philox known answers and its own invariants, the ctypes mirror against the header, the refusals of
mcg_render_scenes and mcg_scene_randomize that happen before any HIP call, and render_into's validation of a table."""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest
import torch

from tests import indep_scene_rand as isr
from tests.common import ROOT

WORLD_RANGES = {"cam_pos": 0.05, "cam_rot": math.radians(5.0), "fovy_scale": (0.9, 1.1), "light_tilt": math.radians(30.0),
                "light_ambient_scale": (0.7, 1.3), "light_diffuse_scale": (0.7, 1.3), "head_scale": (0.7, 1.3), "rgb": 0.1}


def _scene():
    from mycobotgym_amd import load_scene
    return load_scene()


def test_restated_philox_meets_the_random123_known_answers():
    """Random123's kat_vectors for philox4x32-10."""
    ph = isr.philox4x32_10
    assert ph([0] * 4, [0] * 2) == [0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8]
    assert ph([0xffffffff] * 4, [0xffffffff] * 2) == [0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd]
    assert ph([0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344], [0xa4093822, 0x299f31d0]) == [0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1]
    # the pair: top 53 bits of each 64-bit half, in [0, 1); counter and key as the header states them
    u0, u1 = isr.pair(seed=0, gid=0, episode=0, draw=0, stream=0)
    assert u0 == (0x6627e8d5e169c58d >> 11) * 2.0 ** -53 and u1 == (0xbc57ac4c9b00dbd8 >> 11) * 2.0 ** -53
    a = isr.pair(seed=(0x299f31d0 << 32) | 0xa4093822, gid=0x243f6a88, episode=0x85a308d3 - 2 ** 32, draw=0x13198a2e, stream=0x03707344)
    assert a == ((0xd16cfe0994fdcceb >> 11) * 2.0 ** -53, (0x5001e42024126ea1 >> 11) * 2.0 ** -53)
    # the global id's high word enters the fourth counter word, shifted by 8
    r = isr.philox4x32_10([5, 2, 7, isr.STREAM ^ (3 << 8)], [1, 0])
    assert isr.pair(1, 5 + (3 << 32), 2, 7) == ((((r[0] << 32) | r[1]) >> 11) * 2.0 ** -53, (((r[2] << 32) | r[3]) >> 11) * 2.0 ** -53)


def test_restated_rule_invariants(built):
    from mycobotgym_amd import _abi
    sc = _scene()
    for camera in ("sideview", "birdview", "gripper_camera_rgb"):
        base = _abi.scene_row(sc, camera)
        # zero ranges (and no ranges at all): the base row, bit for bit
        for ranges in ({}, {k: (0.0 if not k.endswith("scale") else (1.0, 1.0)) for k in WORLD_RANGES}):
            for gid, ep in ((0, 0), (5, 3), (2 ** 33 + 1, 17)):
                r = isr.row(base, ranges, 7, gid, ep, cam_slot=3)
                assert r.tobytes() == base.tobytes(), (camera, gid, ep)
        rows = isr.table(base, WORLD_RANGES, 7, range(40), [1 + (i % 3) for i in range(40)], cam_slot=1)
        R = rows[:, 3:12].reshape(-1, 3, 3)
        assert np.abs(np.einsum("nki,nkj->nij", R, R) - np.eye(3)).max() <= 1e-12 and np.all(np.linalg.det(R) > 0)
        assert np.abs(np.linalg.norm(rows[:, 13:16], axis=1) - 1.0).max() <= 1e-12
        assert rows[:, 20:38].min() >= 0.0 and rows[:, 20:38].max() <= 1.0 and np.all(rows[:, 38:] == 0.0)
        # every value within its range of the base, and the ranges are used
        assert np.abs(rows[:, 0:3] - base[0:3]).max() <= 0.05 and np.abs(rows[:, 0:3] - base[0:3]).max() > 0.03
        tilt = np.arccos(np.clip(rows[:, 13:16] @ base[13:16], -1, 1))
        assert tilt.max() <= math.radians(30.0) + 1e-12 and tilt.max() > math.radians(15.0)
        angle = np.arccos(np.clip((np.einsum("nii->n", R @ base[3:12].reshape(3, 3).T) - 1) / 2, -1, 1))
        assert angle.max() <= math.radians(5.0) * math.sqrt(3) + 1e-12 and angle.max() > math.radians(2.0)
        for k in (12, 16, 17, 18, 19):
            q = rows[:, k] / base[k]
            assert q.min() >= (0.9 if k == 12 else 0.7) - 1e-12 and q.max() <= (1.1 if k == 12 else 1.3) + 1e-12 and q.max() - q.min() > 0.1
        assert np.allclose(rows[:, 18] / base[18], rows[:, 19] / base[19], rtol=1e-15)          # one factor for both headlight terms
        assert np.abs(rows[:, 20:38] - base[20:38]).max() <= 0.1 + 1e-15
        # light and colours belong to the world: the same for every camera slot; the camera's own jitter differs
        other = isr.table(base, WORLD_RANGES, 7, range(40), [1 + (i % 3) for i in range(40)], cam_slot=0)
        assert np.array_equal(other[:, 13:38], rows[:, 13:38]) and np.all(np.any(other[:, 0:13] != rows[:, 0:13], axis=1))
        # a row is a function of (seed, global id, episode)
        assert not np.array_equal(isr.row(base, WORLD_RANGES, 7, 5, 1), isr.row(base, WORLD_RANGES, 7, 5, 2))
        assert not np.array_equal(isr.row(base, WORLD_RANGES, 7, 5, 1), isr.row(base, WORLD_RANGES, 8, 5, 1))
        assert not np.array_equal(isr.row(base, WORLD_RANGES, 7, 5, 1), isr.row(base, WORLD_RANGES, 7, 6, 1))
    # the light's frame where d0 is (nearly) along x
    base = _abi.scene_row(sc, "sideview").copy()
    base[13:16] = [-1.0, 0.0, 0.0]
    r = isr.table(base, WORLD_RANGES, 1, range(8), [1] * 8)
    assert np.abs(np.linalg.norm(r[:, 13:16], axis=1) - 1.0).max() <= 1e-12 and np.isfinite(r).all()
    # rgb by class
    r = isr.row(_abi.scene_row(sc, "sideview"), {"rgb": {"mesh": 0.2}}, 3, 4, 5)
    b = _abi.scene_row(sc, "sideview")
    assert np.array_equal(np.nonzero(r != b)[0], np.arange(32, 35))


def test_scene_row_and_its_inverse(built):
    from mycobotgym_amd import _abi
    sc = _scene()
    for camera in ("sideview", "gripper_camera_rgb"):
        row = _abi.scene_row(sc, camera)
        assert row.shape == (40,) and row.dtype == np.float64
        cam, scene = _abi.scene_from_row(row, target_half=sc["target_half"])
        src = sc["cameras"][camera] if camera in sc["cameras"] else sc["body_cameras"][camera]
        assert cam == {"pos": src["pos"], "mat": np.asarray(src["mat"], dtype=np.float64).tolist(), "fovy": src["fovy"]}
        assert scene == {k: sc[k] for k in ("light", "headlight", "rgb", "target_half")}
        assert "target_half" not in _abi.scene_from_row(row)[1]
        s = _abi.McgScene.from_camera(sc, src)
        assert np.array_equal(_abi.scene_row(s), row) and np.array_equal(_abi.scene_row(sc, src), row)
    assert row[_abi.SCENE_FOVY] == 50.0 and list(row[_abi.SCENE_LIGHT_DIR:_abi.SCENE_LIGHT_DIR + 3]) == sc["light"]["dir"]
    assert list(row[_abi.SCENE_RGB + 15:_abi.SCENE_RGB + 18]) == sc["rgb"]["sky"] and list(row[_abi.SCENE_PAD:]) == [0.0, 0.0]
    with pytest.raises(ValueError, match="unknown camera"):
        _abi.scene_row(sc, "wrist")
    r = _abi.McgSceneRand.from_dict({"cam_pos": 0.05, "cam_rot": [0.1, 0.2, 0.3], "fovy_scale": (0.9, 1.1), "rgb": {"mesh": 0.2, "sky": 0.1}})
    assert list(r.cam_pos) == [0.05] * 3 and list(r.cam_rot) == [0.1, 0.2, 0.3] and list(r.fovy_scale) == [0.9, 1.1]
    assert list(r.head_scale) == [1.0, 1.0] and r.light_tilt == 0.0 and list(r.rgb) == [0, 0, 0, 0, 0.2, 0.1]
    assert list(_abi.McgSceneRand.from_dict({"rgb": 0.1}).rgb) == [0.1] * 6
    with pytest.raises(ValueError, match="unknown range"):
        _abi.McgSceneRand.from_dict({"cam_position": 0.1})
    with pytest.raises(ValueError, match="colour class"):
        _abi.McgSceneRand.from_dict({"rgb": {"robot": 0.1}})
    assert {"mcg_render_scenes", "mcg_scene_randomize"} <= set(_abi.EXPORTS)


def test_scene_table_mirror_matches_the_header(built, tmp_path):
    """The row's offsets and sizeof / offsetof of mcg_scene_rand as the C compiler sees include/mcg.h == the ctypes mirror; a row is the
    head of mcg_scene."""
    from mycobotgym_amd import _abi
    names = ["ENV_DOUBLES", "CAM_POS", "CAM_MAT", "FOVY", "LIGHT_DIR", "LIGHT_AMBIENT", "LIGHT_DIFFUSE", "HEAD_AMBIENT", "HEAD_DIFFUSE",
             "RGB", "PAD", "RAND_CAM_SLOTS"]
    rand = [n for n, _ in _abi.McgSceneRand._fields_]
    head = ["cam_pos", "cam_mat", "fovy", "light_dir", "light_ambient", "light_diffuse", "head_ambient", "head_diffuse", "rgb_ground",
            "target_half"]
    items = ([f"(size_t)MCG_SCENE_{n}" for n in names] + ["sizeof(mcg_scene_rand)"] + [f"offsetof(mcg_scene_rand,{n})" for n in rand]
             + [f"offsetof(mcg_scene,{n})" for n in head] + ["(size_t)MCG_ABI_VERSION"])
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "mcg.h"\nint main(void){size_t v[]={' + ",".join(items)
                   + '};for(size_t i=0;i<sizeof(v)/sizeof(v[0]);i++)printf("%zu ",v[i]);return 0;}\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split()]
    want = ([_abi.SCENE_ENV_DOUBLES, _abi.SCENE_CAM_POS, _abi.SCENE_CAM_MAT, _abi.SCENE_FOVY, _abi.SCENE_LIGHT_DIR, _abi.SCENE_LIGHT_AMBIENT,
             _abi.SCENE_LIGHT_DIFFUSE, _abi.SCENE_HEAD_AMBIENT, _abi.SCENE_HEAD_DIFFUSE, _abi.SCENE_RGB, _abi.SCENE_PAD,
             _abi.SCENE_RAND_CAM_SLOTS]
            + [C.sizeof(_abi.McgSceneRand)] + [getattr(_abi.McgSceneRand, n).offset for n in rand]
            + [getattr(_abi.McgScene, n).offset for n in head] + [_abi.ABI_VERSION])
    assert got == want
    assert got[0] == 40 and C.sizeof(_abi.McgSceneRand) == 21 * 8 and got[-1] == 8           # additive: the ABI version stays
    # the row's offsets are the head of mcg_scene, in doubles
    row_offsets = [_abi.SCENE_CAM_POS, _abi.SCENE_CAM_MAT, _abi.SCENE_FOVY, _abi.SCENE_LIGHT_DIR, _abi.SCENE_LIGHT_AMBIENT,
                   _abi.SCENE_LIGHT_DIFFUSE, _abi.SCENE_HEAD_AMBIENT, _abi.SCENE_HEAD_DIFFUSE, _abi.SCENE_RGB, _abi.SCENE_PAD]
    assert [getattr(_abi.McgScene, n).offset // 8 for n in head] == row_offsets


def test_render_scenes_refuses_bad_arguments_before_any_hip_call(built):
    """Through the C ABI with a null handle: the argument checks come first, so each refusal names its own reason."""
    from mycobotgym_amd import _abi
    lib = _abi.load()
    out = _abi.McgRenderOut(rgb=0x1000)           # never dereferenced: every call below is refused on the host
    half = (C.c_double * 3)(0.01, 0.01, 0.01)
    def call(table=0x2000, th=half, body=5, znear=0.01, w=64, h=64, s=1, o=out):
        code = lib.mcg_render_scenes(None, table, th, body, znear, w, h, s, 0, None, C.byref(o) if o is not None else None, None)
        return code, lib.mcg_last_error().decode()
    cases = [
        (dict(table=None), "null scene table"), (dict(th=None), "null target_half"), (dict(o=None), "output block"),
        (dict(o=_abi.McgRenderOut()), "all four outputs"), (dict(w=0), "width and height"), (dict(w=513), "width and height"),
        (dict(h=0), "width and height"), (dict(h=513), "width and height"), (dict(s=0), "samples"), (dict(s=5), "samples"),
        (dict(body=-2), "body"), (dict(body=12), "body"), (dict(znear=-1.0), "znear"), (dict(znear=float("nan")), "znear"),
        (dict(znear=float("inf")), "znear"),
    ]
    for kw, text in cases:
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and text in msg and "mcg_render_scenes" in msg, (kw, code, msg)
    for kw in (dict(), dict(body=-1, znear=0.0), dict(body=0), dict(body=11, znear=0.0)):      # all arguments good: only the handle is missing
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and "null handle" in msg, (kw, msg)


def test_scene_randomize_refuses_bad_arguments_before_any_hip_call(built):
    from mycobotgym_amd import _abi
    lib = _abi.load()
    sc = _scene()
    good = _abi.McgScene.from_dict(sc, "sideview")
    def base(**kw):
        s = _abi.McgScene.from_dict(sc, "sideview")
        for k, v in kw.items():
            if isinstance(v, (int, float)):
                setattr(s, k, v)
            else:
                for j, x in enumerate(v):
                    getattr(s, k)[j] = x
        return s
    def rand(**kw):
        return _abi.McgSceneRand.from_dict(dict(WORLD_RANGES, **kw))
    def call(b=good, r=rand(), slot=0, table=0x2000):
        code = lib.mcg_scene_randomize(None, C.byref(b) if b is not None else None, C.byref(r) if r is not None else None, slot, None,
                                       table, None)
        return code, lib.mcg_last_error().decode()
    nan, inf = float("nan"), float("inf")
    cases = [
        (dict(b=None), "null base"), (dict(r=None), "null base scene, ranges"), (dict(table=None), "scene table"),
        (dict(slot=-1), "cam_slot"), (dict(slot=8), "cam_slot"),
        (dict(r=rand(cam_pos=[0.05, -0.01, 0.05])), "negative or not finite"), (dict(r=rand(cam_pos=nan)), "negative or not finite"),
        (dict(r=rand(cam_rot=[0.0, 0.0, inf])), "negative or not finite"), (dict(r=rand(cam_rot=-0.1)), "negative or not finite"),
        (dict(r=rand(rgb=-0.1)), "negative or not finite"), (dict(r=rand(rgb={"mesh": nan})), "negative or not finite"),
        (dict(r=rand(light_tilt=-0.1)), "negative or not finite"), (dict(r=rand(light_tilt=nan)), "negative or not finite"),
        (dict(r=rand(light_tilt=3.2)), "light_tilt"),
        (dict(r=rand(fovy_scale=(0.0, 1.0))), "scale pair"), (dict(r=rand(fovy_scale=(1.1, 0.9))), "scale pair"),
        (dict(r=rand(light_ambient_scale=(-1.0, 1.0))), "scale pair"), (dict(r=rand(light_diffuse_scale=(1.0, nan))), "scale pair"),
        (dict(r=rand(light_diffuse_scale=(1.0, inf))), "scale pair"), (dict(r=rand(head_scale=(nan, 1.0))), "scale pair"),
        (dict(r=rand(head_scale=(2.0, 1.0))), "scale pair"),
        (dict(r=rand(fovy_scale=(0.9, 4.0))), "below 180"),                      # 45 * 4 = 180
        (dict(b=base(fovy=0.0)), "fovy"), (dict(b=base(fovy=nan)), "fovy"),
        (dict(b=base(cam_mat=[1, 1e-6, 0, 0, 1, 0, 0, 0, 1])), "orthonormal"), (dict(b=base(light_dir=[0, 0, -2])), "unit vector"),
    ]
    for kw, text in cases:
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and text in msg and "mcg_scene_randomize" in msg, (kw, code, msg)
    for kw in (dict(), dict(slot=7), dict(r=_abi.McgSceneRand.from_dict({})), dict(r=rand(light_tilt=math.pi), slot=3),
               dict(r=rand(fovy_scale=(0.9, 3.99)))):                              # all arguments good: only the handle is missing
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and "null handle" in msg, (kw, msg)


def test_validation_of_a_scene_table_on_cpu_tensors(built):
    from mycobotgym_amd import _abi, validate_scenes
    sc = _scene()
    base = _abi.scene_row(sc, "sideview")
    good = torch.as_tensor(isr.table(base, WORLD_RANGES, 7, range(16), [1] * 16))
    validate_scenes(good)
    validate_scenes(good, num_envs=16)
    validate_scenes(torch.as_tensor(base).repeat(4, 1))
    def bad(row, col, value):
        t = good.clone()
        t[row, col] = value
        return t
    skew = good.clone()
    skew[5, 3:12] = torch.as_tensor([1.0, 1e-6, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0])
    cases = [(skew, 5, "orthonormal"), (bad(3, 1, float("nan")), 3, "not finite"), (bad(9, 30, float("inf")), 9, "not finite"),
             (bad(7, 12, 180.0), 7, "fovy"), (bad(0, 12, 0.0), 0, "fovy"), (bad(2, 15, -2.0), 2, "unit vector"),
             (bad(11, 25, 1.5), 11, "colour"), (bad(15, 37, -0.1), 15, "colour")]
    for t, row, text in cases:
        with pytest.raises(ValueError, match=f"row {row}: .*{text}"):
            validate_scenes(t)
    two = bad(12, 12, 180.0)
    two[4, 20] = 2.0
    with pytest.raises(ValueError, match="row 4: a colour"):             # the first bad row is named
        validate_scenes(two)
    for t in (good.float(), good[:, :39], good.reshape(-1), good.numpy()):
        with pytest.raises(ValueError, match="float64 tensor"):
            validate_scenes(t)
    with pytest.raises(ValueError, match="float64 tensor"):
        validate_scenes(good, num_envs=8)
