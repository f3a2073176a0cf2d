"""The renderer's pieces that need no GPU: the compiled scene against the MJCF's settings, known answers of the independent rule
(tests/indep_render.py), the class every registered id resolves to, and mcg_render's refusals that happen before any HIP call."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch

from tests import indep_render as ir
from tests.common import ROOT, load_json

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_settings.json")


def _scene():
    from mycobotgym_amd import load_scene
    return load_scene()


def _table(name="mycobot280"):
    from mycobotgym_amd.model.mjcf import _np_model
    return _np_model(load_json(name))


def test_scene_asset_matches_the_mjcf_settings():
    sc = _scene()
    with open(GOLDEN) as f:
        want = json.load(f)
    assert set(sc["cameras"]) == set(want["cameras"]) == {"corner1", "backview", "frontview", "birdview", "sideview"}
    for name, w in want["cameras"].items():
        cam = sc["cameras"][name]
        R = np.asarray(cam["mat"], dtype=np.float64)
        assert np.allclose(cam["pos"], w["pos"], atol=0, rtol=0), name
        assert cam["fovy"] == want["fovy_default"]["value"]
        assert np.abs(R.T @ R - np.eye(3)).max() < 1e-12 and np.linalg.det(R) > 0, name          # a right-handed orthonormal frame
        if "xyaxes" in w:
            x = np.asarray(w["xyaxes"][:3]); y = np.asarray(w["xyaxes"][3:])
            assert np.allclose(R[:, 0], x / np.linalg.norm(x), atol=1e-12), name
            assert R[:, 1] @ y > 0.99 * np.linalg.norm(y), name           # the stated y, orthogonalised against x
        else:
            q = np.asarray(w["quat"], dtype=np.float64); q /= np.linalg.norm(q)
            assert abs(q[0] - q[3]) < 1e-12 and q[1] == q[2] == 0          # a quarter turn about z: x -> y, y -> -x, z stays
            assert np.allclose(R, [[0, -1, 0], [1, 0, 0], [0, 0, 1]], atol=1e-12)
    for k, w in want["rgb"].items():
        assert np.allclose(sc["rgb"][k], w["value"], atol=0, rtol=0), k
    assert sc["target_half"] == want["target_half"]["value"]
    L = want["light"]
    assert np.allclose(sc["light"]["dir"], L["dir"]) and sc["light"]["ambient"] == L["ambient"] and sc["light"]["diffuse"] == L["diffuse"]
    assert sc["headlight"] == {k: want["headlight_default"][k] for k in ("ambient", "diffuse")}
    # sideview looks down its -z at the table: the ray through the picture's centre meets the table top
    cam = sc["cameras"]["sideview"]
    view = -np.asarray(cam["mat"])[:, 2]
    assert view[2] < 0
    t = (want["table"]["pos"][2] + want["table"]["half"][2] - cam["pos"][2]) / view[2]
    hit = np.asarray(cam["pos"]) + t * view
    assert np.all(np.abs(hit[:2] - np.asarray(want["table"]["pos"][:2])) < np.asarray(want["table"]["half"][:2]))
    # the compiled model agrees with the fixture on the table the renderer reads from the model block
    from mycobotgym_amd.model.specialize import specialize
    spec = specialize(_table())
    assert np.allclose(spec["table_pos"], want["table"]["pos"]) and np.allclose(spec["table_half"], want["table"]["half"])


def test_mcg_scene_from_dict_fills_every_field():
    from mycobotgym_amd import _abi
    sc = _scene()
    s = _abi.McgScene.from_dict(sc, "corner1")
    assert list(s.cam_pos) == sc["cameras"]["corner1"]["pos"]
    assert np.allclose(np.asarray(list(s.cam_mat)).reshape(3, 3), sc["cameras"]["corner1"]["mat"], atol=0)
    assert s.fovy == 45.0 and list(s.light_dir) == [0.0, 0.0, -1.0]
    assert (s.light_ambient, s.light_diffuse, s.head_ambient, s.head_diffuse) == (0.5, 0.8, 0.1, 0.4)
    assert list(s.rgb_target) == [0.0, 1.0, 0.0] and list(s.rgb_sky) == [0.9, 0.95, 0.95] and list(s.target_half) == [0.01] * 3
    with pytest.raises(ValueError, match="unknown camera"):
        _abi.McgScene.from_dict(sc, "gripper_camera_rgb")


def test_rule_known_answers():
    sc, tab = _scene(), _table()
    q = np.asarray(tab["qpos0"], dtype=np.float64)
    from mycobotgym_amd.model.specialize import specialize
    target0 = np.asarray(specialize(tab)["target0"])
    W = H = 64
    for cam in ("sideview", "birdview", "corner1"):
        pic = ir.picture(tab, q, target0, sc, cam, W, H)
        for point, gid in ((q[12:15], 2), (target0, 3)):           # the cube's centre, the target site's centre
            x, y = ir.project(sc["cameras"][cam], W, H, point)
            assert pic["geom"][int(np.floor(y)), int(np.floor(x))] == gid, (cam, gid, x, y)
        # depth is the distance along the viewing axis: the target box's near face is within its half-diagonal of its centre
        x, y = ir.project(sc["cameras"][cam], W, H, target0)
        c = sc["cameras"][cam]
        zc = -(np.asarray(c["mat"]).T @ (target0 - np.asarray(c["pos"])))[2]
        assert abs(pic["depth"][int(np.floor(y)), int(np.floor(x))] - zc) < 0.01 * np.sqrt(3)
    # hidden cube (Reach): no pixel of id 2
    pic = ir.picture(tab, q, target0, sc, "sideview", W, H, draw_cube=False)
    assert not (pic["geom"] == 2).any() and (pic["geom"] == 3).any()
    # a camera turned straight up sees only sky
    up = {"pos": [0.0, 0.0, 0.9], "mat": [[1, 0, 0], [0, -1, 0], [0, 0, -1]], "fovy": 45.0}       # its -z is the world's +z
    pic = ir.picture(tab, q, target0, sc, up, W, H)
    assert (pic["geom"] == -1).all() and np.isinf(pic["depth"]).all()
    assert np.allclose(pic["rgb"], 255.0 * np.asarray(sc["rgb"]["sky"]))
    # the ground, lit from straight above and seen by the headlight: 0.2 * (0.5 + 0.8 + 0.1 + 0.4 * cos) per channel
    pic = ir.picture(tab, q, target0, sc, "birdview", W, H)
    g = pic["geom"] == 0
    assert g.any()
    assert np.all(pic["rgb"][g] <= 255 * 0.2 * 1.8 + 1e-9) and np.all(pic["rgb"][g] >= 255 * 0.2 * 1.4)


def test_every_id_resolves_to_its_class():
    import mycobotgym_amd as mg
    from mycobotgym_amd import MyCobotImgVecEnv, MyCobotVecEnv, env_class
    assert issubclass(MyCobotImgVecEnv, MyCobotVecEnv)
    v0 = [i for i in mg.REGISTRY if i.endswith("-v0")]; v1 = [i for i in mg.REGISTRY if i.endswith("-v1")]
    assert len(v0) == 30 and len(v1) == 20
    assert all(env_class(i) is MyCobotImgVecEnv for i in v1)
    assert all(env_class(i) is MyCobotVecEnv for i in v0)
    assert MyCobotVecEnv.metadata["render_modes"] == ["rgb_array", "depth_array"]
    with pytest.raises(ValueError, match="reward_shaping"):
        MyCobotImgVecEnv(1, reward_type="reward_shaping")


def test_v1_ids_construct_up_to_the_gpu(built):
    """Every -v1 id gets as far as the engine: without a GPU it is refused there (McgError), not at an unimplemented observation."""
    import mycobotgym_amd as mg
    from mycobotgym_amd._abi import McgError
    from mycobotgym_amd import MyCobotVecEnv
    with pytest.raises(NotImplementedError, match="MyCobotImgVecEnv"):
        MyCobotVecEnv(1, image_obs=True)                      # the state class goes on refusing; its text names the image class
    with pytest.raises(McgError):
        mg.make("MyCobotReach-Dense-joint-v1", device="cpu")  # the engine's own refusal, on any machine
    if not torch.cuda.is_available():
        with pytest.raises(McgError):
            mg.make("MyCobotReach-Dense-joint-v1")
        for i in mg.REGISTRY:
            if i.endswith("-v1"):
                with pytest.raises(McgError):
                    mg.make(i, num_envs=2)


def test_render_refuses_bad_arguments_before_any_hip_call(built):
    """Through the C ABI with a null handle: the argument checks come first, so each refusal names its own reason."""
    from mycobotgym_amd import _abi
    lib = _abi.load()
    good = _abi.McgScene.from_dict(_scene(), "sideview")
    out = _abi.McgRenderOut(rgb=0x1000)           # never dereferenced: every call below is refused on the host
    def call(scene=good, w=64, h=64, s=1, o=out):
        code = lib.mcg_render(None, C.byref(scene) if scene is not None else None, w, h, s, 0, None, C.byref(o) if o is not None else None, None)
        return code, lib.mcg_last_error().decode()
    def variant(**kw):
        s = _abi.McgScene.from_dict(_scene(), "sideview")
        for k, v in kw.items():
            if isinstance(v, (int, float)):
                setattr(s, k, v)
            else:
                for j, x in enumerate(v):
                    getattr(s, k)[j] = x
        return s
    cases = [
        (dict(scene=None), "null scene"), (dict(o=None), "null scene or output"), (dict(o=_abi.McgRenderOut()), "all four outputs"),
        (dict(w=0), "width and height"), (dict(w=513), "width and height"), (dict(h=0), "width and height"), (dict(h=513), "width and height"),
        (dict(s=0), "samples"), (dict(s=5), "samples"),
        (dict(scene=variant(fovy=0.0)), "fovy"), (dict(scene=variant(fovy=180.0)), "fovy"), (dict(scene=variant(fovy=float("nan"))), "fovy"),
        (dict(scene=variant(cam_mat=[1, 0, 0, 0, 1, 0, 0, 0, 1.0001])), "orthonormal"),
        (dict(scene=variant(cam_mat=[1, 1e-6, 0, 0, 1, 0, 0, 0, 1])), "orthonormal"),
        (dict(scene=variant(light_dir=[0, 0, -2])), "unit vector"),
    ]
    for kw, text in cases:
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and text in msg, (kw, code, msg)
    code, msg = call()                              # all arguments good: only the handle is missing
    assert code == _abi.MCG_ERR_ARG and "null handle" in msg
