#!/usr/bin/env python3
"""Offline: compile what a picture of the reference's scene needs into ``mycobotgym_amd/assets/scene.json``.

    python tools/compile_scene.py [--assets /root/reference/mycobotgym/envs/assets]

Reads the reference's MJCF where it lies (``mycobot280.xml`` and its include, parsed with ``MjcfCompiler``'s loader) and writes resolved
numbers only: the five world cameras (position, 3x3 frame with the camera's x, y, z as columns -- a MuJoCo camera looks along its -z --
and fovy), the cameras that hang on a body (``body_cameras``: the same, stated in the frame of the engine body the camera rides on, with
every joint-less body in between composed in float64, and the near plane), the directional light, MuJoCo's default headlight, the colours and the target site's box.  The model tables
(``tools/compile_model.py``) are not touched: they are stamped and compared against the oracle's tables, a picture is not physics.

Values the MJCF leaves to MuJoCo's defaults are [RECALL]: camera fovy 45 degrees, geom rgba 0.5 0.5 0.5 1, headlight ambient 0.1 /
diffuse 0.4.  The cube's geom (default grey) carries a coincident white site of the same size (``mycobot280_main.xml:263-264``): the
cube is drawn white, the colour a viewer sees where two coincident surfaces fight.

The near plane of a body camera: the MJCF states no ``<visual><map znear>``, and MuJoCo's default is 0.01 x the model's extent [RECALL],
which is not computed here.  ZNEAR = 0.01 m is this project's choice, not parity.
"""
import argparse
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))

from mycobotgym_amd.model.mjcf import MjcfCompiler, _floats, euler_to_quat, quat_normalize, quat_to_mat  # noqa: E402
from mycobotgym_amd.model.specialize import MOVING  # noqa: E402

OUT = os.path.join(os.path.dirname(__file__), "..", "mycobotgym_amd", "assets", "scene.json")
DEFAULT_FOVY, DEFAULT_GEOM_RGB = 45.0, [0.5, 0.5, 0.5]
HEADLIGHT = {"ambient": 0.1, "diffuse": 0.4}
ZNEAR = 0.01


def camera_frame(a: dict) -> np.ndarray:
    """3x3 parent <- camera, columns x (right), y (up), z (the camera looks along -z), from ``xyaxes``, ``quat`` or ``euler`` (radians,
    sequence xyz: the MJCF's compiler settings)."""
    if "xyaxes" in a:
        v = np.array(_floats(a["xyaxes"]))
        x = v[:3] / np.linalg.norm(v[:3])
        y = v[3:] - x * (x @ v[3:])                 # MuJoCo orthogonalises y against x
        y /= np.linalg.norm(y)
        return np.stack([x, y, np.cross(x, y)], axis=1)
    if "quat" in a:
        q = quat_normalize(_floats(a["quat"]))
    elif "euler" in a:
        q = euler_to_quat(_floats(a["euler"]))
    else:
        q = np.array([1.0, 0, 0, 0])
    return np.asarray(quat_to_mat(q), dtype=np.float64).reshape(3, 3)


def body_cameras(world) -> dict:
    """Every <camera> under a body, in the frame of the engine body it rides on: a body of ``specialize.MOVING`` (index = engine body;
    its frame is the MJCF body's own) or a joint-less descendant of one, whose ``pos`` / ``quat`` / ``euler`` are composed on the way."""
    out = {}

    def walk(e, carrier, R, p):
        for b in e.findall("body"):
            a = b.attrib
            if a.get("name") in MOVING:
                cb, Rb, pb = MOVING.index(a["name"]), np.eye(3), np.zeros(3)
            elif carrier is None:
                cb, Rb, pb = None, None, None
            else:
                assert b.find("joint") is None and b.find("freejoint") is None, a.get("name")
                cb, pb, Rb = carrier, p + R @ np.array(_floats(a.get("pos", "0 0 0"))), R @ camera_frame(a)
            if cb is not None:
                for c in b.findall("camera"):
                    ca = c.attrib
                    out[ca["name"]] = {"body": cb, "body_name": MOVING[cb], "pos": (pb + Rb @ np.array(_floats(ca.get("pos", "0 0 0")))).tolist(),
                                       "mat": (Rb @ camera_frame(ca)).tolist(), "fovy": float(ca.get("fovy", DEFAULT_FOVY)), "znear": ZNEAR}
            walk(b, cb, Rb, pb)

    walk(world, None, None, None)
    return out


def compile_scene(xml_path: str) -> dict:
    root = MjcfCompiler(xml_path).root            # <include> expanded
    world = next(e for e in root if e.tag == "worldbody")
    rgb = lambda e: _floats(e.attrib["rgba"])[:3]
    cams = {}
    for c in world.findall("camera"):             # the world's own cameras: the gripper camera hangs on a body
        cams[c.attrib["name"]] = {"pos": _floats(c.attrib["pos"]), "mat": camera_frame(c.attrib).tolist(),
                                  "fovy": float(c.attrib.get("fovy", DEFAULT_FOVY))}
    plane = next(g for g in world.findall("geom") if g.attrib.get("type") == "plane")
    table = next(b for b in world.findall("body") if b.attrib.get("name") == "table").find("geom")
    target = next(s for s in world.findall("site") if s.attrib.get("name") == "target0")
    cube = next(b for b in world.findall("body") if b.attrib.get("name") == "object0")
    cube_site = cube.find("site")
    meshes = [g for g in world.iter("geom") if g.attrib.get("type") == "mesh" and "rgba" in g.attrib]
    mesh_rgb = {tuple(rgb(g)) for g in meshes}
    assert len(mesh_rgb) == 1, mesh_rgb           # one colour for the whole robot
    light = next(l for l in world.findall("light") if l.attrib.get("name") == "light0")
    assert light.attrib.get("directional") == "true" and light.attrib.get("castshadow") == "false"
    amb, dif = _floats(light.attrib["ambient"]), _floats(light.attrib["diffuse"])
    assert len(set(amb)) == 1 and len(set(dif)) == 1            # a white light: one number each
    d = np.array(_floats(light.attrib["dir"])); d /= np.linalg.norm(d)
    sky = next(t for t in root.iter("texture") if t.attrib.get("type") == "skybox")
    assert "rgba" not in cube.find("geom").attrib
    return {
        "cameras": cams,
        "body_cameras": body_cameras(world),
        "light": {"dir": d.tolist(), "ambient": amb[0], "diffuse": dif[0]},
        "headlight": dict(HEADLIGHT),
        "rgb": {"ground": rgb(plane), "table": rgb(table), "cube": rgb(cube_site), "target": rgb(target), "mesh": list(mesh_rgb.pop()),
                "sky": _floats(sky.attrib["rgb1"])},
        "cube_geom_rgb": DEFAULT_GEOM_RGB,
        "target_half": _floats(target.attrib["size"]),
    }


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--assets", default="/root/reference/mycobotgym/envs/assets")
    args = ap.parse_args()
    scene = compile_scene(os.path.join(args.assets, "mycobot280.xml"))
    with open(OUT, "w") as f:
        json.dump(scene, f, indent=1)
        f.write("\n")
    print(f"{len(scene['cameras'])} cameras {sorted(scene['cameras'])}, body cameras {sorted(scene['body_cameras'])} -> {os.path.relpath(OUT)}")


if __name__ == "__main__":
    main()
