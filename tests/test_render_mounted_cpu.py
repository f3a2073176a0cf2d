"""The body-mounted camera's pieces that need no GPU: the compiled ``body_cameras`` against the MJCF's own attributes placed through the
MJCF body tree, mcg_render_mounted's refusals that happen before any HIP call, and known answers of the one-sided independent rule
(tests/indep_render_mounted.py)."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import indep_render as ir
from tests import indep_render_mounted as irm
from tests.common import ROOT, load_json

GOLDEN = os.path.join(ROOT, "tests", "golden", "scene_body_cameras.json")
CAMERA = "gripper_camera_rgb"
FLANGE = 4 + 6           # mcg_render_out.geom of the flange's polytope


def _scene():
    from mycobotgym_amd import load_scene
    return load_scene()


def _table(name="mycobot280"):
    from mycobotgym_amd.model.mjcf import _np_model
    return _np_model(load_json(name))


def _fixture():
    with open(GOLDEN) as f:
        return json.load(f)


def test_body_camera_asset_matches_the_mjcf_attributes():
    sc, tab, fx = _scene(), _table(), _fixture()
    assert set(sc["cameras"]) == {"corner1", "backview", "frontview", "birdview", "sideview"}          # still the five world cameras
    assert set(sc["body_cameras"]) == set(fx["cameras"]) == {CAMERA}
    cam, entry = sc["body_cameras"][CAMERA], fx["cameras"][CAMERA]
    assert cam["fovy"] == 50.0 == entry["camera"]["fovy"]
    assert cam["body"] == 5 == entry["engine_body"]["index"] and cam["body_name"] == "link6" == entry["engine_body"]["name"]
    assert cam["znear"] == fx["znear"]["value"] == 0.01
    # the compiled table's tree has the carriers where the fixture says the MJCF puts them
    names = list(tab["body_name"])
    for c in entry["carriers"]:
        b = names.index(c["name"])
        assert names[tab["body_parent"][b]] == c["parent"], c
        assert np.allclose(tab["body_pos"][b], c["pos"], atol=0) and np.allclose(tab["body_quat"][b], c["quat"], atol=1e-15), c
        assert tab["body_dofnum"][b] == 0, c
    Rc = np.asarray(cam["mat"], dtype=np.float64)
    assert np.abs(Rc.T @ Rc - np.eye(3)).max() < 1e-12 and np.linalg.det(Rc) > 0
    # engine body 5 is MJCF body link6 (specialize.MOVING); its frame composed with the asset's pose against the independent placement
    from mycobotgym_amd.model.refdyn import kinematics
    from mycobotgym_amd.model.specialize import MOVING
    assert MOVING[5] == "link6"
    q0 = np.asarray(tab["qpos0"], dtype=np.float64)
    rng = np.random.default_rng(21)
    poses = [q0] + [np.concatenate([q0[:6] + rng.uniform(-1.5, 1.5, 6), q0[6:]]) for _ in range(5)]
    for q in poses:
        want = irm.mounted_camera(tab, q, entry)
        kin = kinematics(tab, q)
        b = names.index("link6")
        R5, p5 = np.asarray(kin["xmat"][b]).reshape(3, 3), np.asarray(kin["xpos"][b])
        assert np.abs(p5 + R5 @ np.asarray(cam["pos"]) - want["pos"]).max() <= 1e-12
        assert np.abs(R5 @ Rc - np.asarray(want["mat"])).max() <= 1e-12
    # at qpos0 the camera looks along the gripper: horizontally, toward gripper_tcp, z up
    w0 = irm.mounted_camera(tab, q0, entry)
    view, up = -np.asarray(w0["mat"])[:, 2], np.asarray(w0["mat"])[:, 1]
    kin = kinematics(tab, q0)
    tcp = np.asarray(kin["xpos"][names.index("gripper_tcp")]) - np.asarray(w0["pos"])
    assert abs(view[2]) < 2e-4 and view @ tcp / np.linalg.norm(tcp) > 0.9 and up[2] > 0.999


def test_python_resolves_both_kinds_of_camera(built):
    """``_scene`` is what render(), render_into() and MyCobotImgVecEnv resolve a name with; it needs no engine."""
    from mycobotgym_amd import MyCobotVecEnv, _abi
    sc = _scene()
    env = MyCobotVecEnv.__new__(MyCobotVecEnv)            # no engine: only the resolution is exercised
    env._closed = True
    s, body, znear = env._scene(CAMERA, None)
    assert body == 5 and znear == 0.01 and s.fovy == 50.0 and list(s.cam_pos) == sc["body_cameras"][CAMERA]["pos"]
    s, body, znear = env._scene("sideview", None)
    assert body == -1 and znear == 0.0 and s.fovy == 45.0
    with pytest.raises(ValueError, match="unknown camera.*sideview.*gripper_camera_rgb"):
        env._scene("wrist", None)
    with pytest.raises(ValueError, match="unknown camera"):         # from_dict keeps its behaviour: world cameras only
        _abi.McgScene.from_dict(sc, CAMERA)
    assert "mcg_render_mounted" in _abi.EXPORTS


def test_render_mounted_refuses_bad_arguments_before_any_hip_call(built):
    """Through the C ABI with a null handle: the argument checks come first, so each refusal names its own reason."""
    from mycobotgym_amd import _abi
    lib = _abi.load()
    good = _abi.McgScene.from_camera(_scene(), _scene()["body_cameras"][CAMERA])
    out = _abi.McgRenderOut(rgb=0x1000)           # never dereferenced: every call below is refused on the host
    def call(body=5, znear=0.01, scene=good, w=64, h=64, s=1, o=out):
        code = lib.mcg_render_mounted(None, C.byref(scene) if scene is not None else None, body, znear, w, h, s, 0, None,
                                      C.byref(o) if o is not None else None, None)
        return code, lib.mcg_last_error().decode()
    cases = [
        (dict(body=-2), "body"), (dict(body=12), "body"), (dict(znear=-1.0), "znear"), (dict(znear=float("nan")), "znear"),
        (dict(znear=float("inf")), "znear"),
        (dict(scene=None), "null scene"), (dict(o=_abi.McgRenderOut()), "all four outputs"), (dict(w=0), "width and height"),
        (dict(h=513), "width and height"), (dict(s=5), "samples"),
    ]
    for kw, text in cases:
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and text in msg and "mcg_render_mounted" in msg, (kw, code, msg)
    for kw in (dict(), dict(body=-1, znear=0.0), dict(body=0), dict(body=11, znear=0.0)):      # all arguments good: only the handle is missing
        code, msg = call(**kw)
        assert code == _abi.MCG_ERR_ARG and "null handle" in msg, (kw, msg)


def test_one_sided_rule_known_answers():
    sc, tab, fx = _scene(), _table(), _fixture()
    q = np.asarray(tab["qpos0"], dtype=np.float64)
    from mycobotgym_amd.model.specialize import specialize
    target0 = np.asarray(specialize(tab)["target0"])
    W = H = 64
    # a camera outside every solid, no near plane: indep_render's picture (a ray from outside meets a front face first)
    two = ir.picture(tab, q, target0, sc, "sideview", W, H)
    one = irm.picture(tab, q, target0, sc, sc["cameras"]["sideview"], W, H, znear=0.0)
    assert np.array_equal(one["geom"], two["geom"]) and np.array_equal(one["depth"], two["depth"])
    assert np.abs(one["rgb"] - two["rgb"]).max() < 1e-9          # (the normal is the hull's equation here, a cross product there)
    # from inside the flange's polytope that geom is never seen; the two-sided rule sees nothing else
    cam = irm.mounted_camera(tab, q, fx["cameras"][CAMERA])
    inside = ir.picture(tab, q, target0, sc, cam, W, H)
    assert (inside["geom"] == FLANGE).all() and inside["depth"].max() < 0.02
    pic = irm.picture(tab, q, target0, sc, cam, W, H, znear=0.01)
    ids, counts = np.unique(pic["geom"], return_counts=True)
    seen = dict(zip(ids.tolist(), counts.tolist()))
    print(f"\n[mounted rule] qpos0, 64 x 64: pixels per geom id {seen}, nearest hit {pic['depth'].min():.4f} m")
    assert FLANGE not in seen
    hinges = [4 + 12, 4 + 13]
    assert all(seen.get(g, 0) > 200 for g in hinges), seen           # the two hinge links fill the lower middle of the picture
    near = np.unravel_index(pic["depth"].argmin(), pic["depth"].shape)
    assert pic["geom"][near] in hinges and 0.05 < pic["depth"].min() < 0.06
    assert len(seen) >= 6
    # a near plane beyond the hinge links: they vanish, what lies behind them shows
    far = irm.picture(tab, q, target0, sc, cam, W, H, znear=0.07)
    assert far["depth"].min() >= 0.07
    gone = (pic["depth"] < 0.07)
    assert gone.any() and (far["geom"][gone] != pic["geom"][gone]).all()
    keep = ~gone                                                      # what lies wholly beyond the plane is not touched by it
    assert np.array_equal(far["geom"][keep], pic["geom"][keep])
