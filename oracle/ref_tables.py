"""Model tables compiled from the upstream MyCobotGym MJCF (TEST INFRASTRUCTURE ONLY; the output stays out of git).

``build()`` runs this repository's MJCF compiler (mycobotgym_amd/model/mjcf.py) over the upstream checkout's
``mycobotgym/envs/assets`` and writes the same eight tables as tools/compile_model.py to ``oracle/_ref/tables/<name>.json``,
together with ``stamp.json``: the sha256 of the compiler sources that made them.  tests/test_model_compiler.py compares them
with the committed ``mycobotgym_amd/assets/*.json``, so no test reads outside the repository.

The upstream checkout is ``$MCG_REFERENCE`` (default ``/root/reference``).  Where it is absent, tables made earlier are
kept as they are; the stamp lets the test tell whether they were made by the compiler it is testing.
"""
from __future__ import annotations

import hashlib
import json
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(_HERE)
OUT = os.path.join(_HERE, "_ref", "tables")
STAMP = os.path.join(OUT, "stamp.json")
COMPILER_SOURCES = [os.path.join(ROOT, "mycobotgym_amd", "model", f) for f in ("mjcf.py", "refdyn.py")]

# (output name, xml, mesh rule, dropped bodies): tools/compile_model.py's jobs
JOBS = (
    ("mycobot280", "mycobot280.xml", "legacy", ()),
    ("mycobot280_reach", "mycobot280.xml", "legacy", ("object0",)),
    ("mycobot280_exactmesh", "mycobot280.xml", "exact", ()),
    ("mycobot280_reach_exactmesh", "mycobot280.xml", "exact", ("object0",)),
    ("mycobot280_mocap", "mycobot280_mocap.xml", "legacy", ()),
    ("mycobot280_mocap_reach", "mycobot280_mocap.xml", "legacy", ("object0",)),
    ("mycobot280_mocap_exactmesh", "mycobot280_mocap.xml", "exact", ()),
    ("mycobot280_mocap_reach_exactmesh", "mycobot280_mocap.xml", "exact", ("object0",)),
)


def upstream_assets() -> str:
    return os.path.join(os.environ.get("MCG_REFERENCE", "/root/reference"), "mycobotgym", "envs", "assets")


def compiler_hash() -> str:
    h = hashlib.sha256()
    for p in COMPILER_SOURCES:
        h.update(os.path.basename(p).encode())
        with open(p, "rb") as f:
            h.update(f.read())
    return h.hexdigest()


def read_stamp():
    try:
        with open(STAMP) as f:
            return json.load(f)
    except (OSError, ValueError):
        return None


def build() -> str:
    """Compile the tables when the upstream assets are readable and the stamp is not current; otherwise keep what is there."""
    assets = upstream_assets()
    want = compiler_hash()
    st = read_stamp()
    if not os.path.isfile(os.path.join(assets, "mycobot280.xml")) or (st and st.get("compiler_sha256") == want):
        return OUT
    from mycobotgym_amd.model.mjcf import MjcfCompiler, save_model
    os.makedirs(OUT, exist_ok=True)
    if os.path.exists(STAMP):
        os.remove(STAMP)                   # no stamp while the tables are half rewritten
    for name, xml, rule, drop in JOBS:
        save_model(MjcfCompiler(os.path.join(assets, xml), mesh_inertia=rule, drop_bodies=drop).compile(),
                   os.path.join(OUT, name + ".json"))
    with open(STAMP, "w") as f:
        json.dump({"compiler_sha256": want, "tables": [j[0] for j in JOBS]}, f)
    return OUT
