"""Caller-supplied models (CPU): the perturbed-model fixture moves what it claims to, mcg_create's host-side checks refuse polytope blocks
and models the kernels cannot run (before any HIP call), and the initial state of a given table is that table's own."""
import ctypes as C

import numpy as np
import pytest

from tests.common import load_json, perturbed_table

NAMES = ("mycobot280", "mycobot280_reach", "mycobot280_mocap")


def _spec(tab):
    from mycobotgym_amd.model.mjcf import _np_model
    from mycobotgym_amd.model.specialize import specialize
    return specialize(_np_model(tab))


def _arr(model, name):
    return np.ctypeslib.as_array(getattr(model, name)).copy()


@pytest.mark.parametrize("name", NAMES)
def test_perturbation_moves_every_listed_field(name):
    """A no-op perturbation must not pass: every field the fixture claims to move differs from the built-in block, entry by entry where
    the built-in entry is non-zero."""
    from mycobotgym_amd._abi import McgModel
    base, pert = McgModel.from_spec(_spec(load_json(name))), McgModel.from_spec(_spec(perturbed_table(name)))
    B, P = _arr(base, "body"), _arr(pert, "body")          # rows: r(3) mass mc(3) inertia(6) armature damping hull_rad
    def moved(what, a, b):
        a, b = np.asarray(a), np.asarray(b)
        live = a != 0
        assert live.any() and np.all(a[live] != b[live]), (name, what, a, b)
        print(f"{name} {what}: {int(live.sum())} entries moved, largest relative change {np.max(np.abs(b[live] / a[live] - 1)):.3f}")
    hung = [6, 8, 10, 11]                                  # the gripper's bodies on link6 (the fingers hang on the gears)
    moved("body[].r", np.linalg.norm(B[[1, 2, 3, 4, 5] + hung, 0:3], axis=1), np.linalg.norm(P[[1, 2, 3, 4, 5] + hung, 0:3], axis=1))
    assert np.all(np.abs(P[hung, 0] - B[hung, 0]) > 0.004), "the spacer moves the gripper's bodies along link6's x"
    moved("mass", B[:12, 3], P[:12, 3])
    moved("inertia", B[:12, 7:10], P[:12, 7:10])
    moved("armature", B[:12, 13], P[:12, 13])
    moved("damping", B[:12, 14], P[:12, 14])
    moved("jnt_range", _arr(base, "jnt_range")[:6], _arr(pert, "jnt_range")[:6])
    moved("act_gain", _arr(base, "act_gain"), _arr(pert, "act_gain"))
    moved("act_bias", _arr(base, "act_bias"), _arr(pert, "act_bias"))
    moved("site_eef", _arr(base, "site_eef"), _arr(pert, "site_eef"))
    if name == "mycobot280_mocap":
        moved("weld_anchor[0]", _arr(base, "weld_anchor")[:1], _arr(pert, "weld_anchor")[:1])      # the spacer: along link6's x
    if name != "mycobot280_reach":
        moved("cube_half", _arr(base, "cube_half"), _arr(pert, "cube_half"))
        moved("table top", [base.table_pos[2] + base.table_half[2]], [pert.table_pos[2] + pert.table_half[2]])
        moved("pad_box", _arr(base, "pad_box")[:, 3:], _arr(pert, "pad_box")[:, 3:])
        moved("mesh_box[6:8]", _arr(base, "mesh_box")[6:8, 0], _arr(pert, "mesh_box")[6:8, 0])
        moved("geom_friction0[cube]", _arr(base, "geom_friction0")[2:], _arr(pert, "geom_friction0")[2:])
        moved("mesh_fric", [base.mesh_fric], [pert.mesh_fric])
        moved("hull_rad[5]", B[5:6, 15], P[5:6, 15])


def test_perturbed_table_keeps_the_cube_at_rest_on_the_table():
    tab = perturbed_table("mycobot280")
    s = _spec(tab)
    top = s["table_pos"][2] + s["table_half"][2]
    z = tab["qpos0"][14]
    print(f"\ntable top {top:.6f}, cube centre {z:.6f}, half-size {s['cube_half'][2]:.6f}")
    assert abs(z - s["cube_half"][2] - top) < 1e-12 and tab["body_pos"][tab["body_name"].index("object0")][2] == z


# ------------------------------------------------------------------------------------------------- mcg_create's host checks
def _cfg(mocap=False, has_object=1):
    from mycobotgym_amd import _abi
    return _abi.McgConfig(n_envs=4, has_object=has_object, controller=_abi.CTRL_MOCAP if mocap else _abi.CTRL_JOINT, reward_type=1,
                          frame_skip=20, control_steps=5, max_episode_steps=50)


def _create(model, blob, mocap=False, n=None):
    """mcg_create's return code and message; a handle that a GPU host hands out is destroyed at once."""
    from mycobotgym_amd import _abi
    lib = _abi.load()
    cfg = _cfg(mocap)
    b = None if blob is None else np.ascontiguousarray(blob, dtype=np.float64)
    h = C.c_void_p()
    rc = lib.mcg_create(C.byref(cfg), None if model is None else C.byref(model), None if b is None else b.ctypes.data,
                        0 if b is None else (len(b) if n is None else n), 0, C.byref(h))
    msg = lib.mcg_last_error().decode()
    if rc == _abi.MCG_OK:
        lib.mcg_destroy(h)
    return rc, msg


def _passes(rc, msg):
    """Past the host checks: created (GPU host) or stopped at the device query (GPU-less host)."""
    from mycobotgym_amd import _abi
    return rc == _abi.MCG_OK or (rc == _abi.MCG_ERR_HIP and "no HIP device" in msg)


def _model_and_blob(tab):
    from mycobotgym_amd._abi import McgModel
    s = _spec(tab)
    return McgModel.from_spec(s), np.asarray(s["polytopes"], dtype=np.float64)


def test_valid_models_and_blocks_get_past_the_checks(built):
    from mycobotgym_amd import _abi
    lib = _abi.load()
    for variant in range(4):
        m = _abi.McgModel()
        assert lib.mcg_default_model(variant, C.byref(m)) == 0
        rc, msg = _create(m, None, mocap=variant >= 2)
        assert _passes(rc, msg), (variant, rc, msg)
    assert _passes(*_create(None, None))
    for name, mocap in (("mycobot280", False), ("mycobot280_mocap", True)):
        m, blob = _model_and_blob(load_json(name))
        assert _passes(*_create(m, blob, mocap)), name                         # the built-in model with its own (= the built-in) block
        m, blob = _model_and_blob(perturbed_table(name))
        rc, msg = _create(m, blob, mocap)
        assert _passes(rc, msg), (name, rc, msg)


def _mutations(blob):
    """(what, mutated blob, n_polytopes or None, expected words of the message) -- each malformed in one way."""
    from mycobotgym_amd.model import polytope as pt
    meta = blob[:pt.NMESH * pt.META].reshape(pt.NMESH, pt.META)
    out = [("truncated", blob, len(blob) - 1, "polytope block")]
    def mut(what, m, k, val, words="polytope block"):
        b = blob.copy(); b[pt.META * m + k] = val; out.append((what, b, None, words))
    m = 7                                                          # gripper_base
    b = blob.copy(); b[pt.META * m + 1] = b[pt.META * m + 5] = 0; out.append(("Fp = 0 (F = 0)", b, None, "polytope block"))
    b = blob.copy(); b[pt.META * m + 2] = b[pt.META * m + 6] = 0; out.append(("Ep = 0 (E = 0)", b, None, "polytope block"))
    mut("Fp = 0", m, 5, 0)
    mut("Ep = 0", m, 6, 0)
    mut("negative nf", m, 1, -1)
    mut("negative ne", m, 2, -1)
    mut("fractional V", m, 0, meta[m, 0] - 0.5)
    mut("fractional spare entry", m, 7, 0.25)
    mut("offset into the meta region", 0, 3, pt.NMESH * pt.META - 8)
    return out


def test_malformed_polytope_blocks_are_refused(built):
    from mycobotgym_amd import _abi
    m, blob = _model_and_blob(perturbed_table("mycobot280"))
    for what, b, n, words in _mutations(blob):
        rc, msg = _create(m, b, n=n)
        print(f"{what}: {rc} {msg}")
        assert rc == _abi.MCG_ERR_ARG and words in msg, (what, rc, msg)


def test_vertices_outside_the_models_bounds_are_refused(built):
    """A vertex outside its mesh_box, and one inside the box but beyond its body's hull_rad: the broad phase would skip its contacts."""
    from mycobotgym_amd import _abi
    from mycobotgym_amd.model import polytope as pt
    m, blob = _model_and_blob(perturbed_table("mycobot280"))
    box, body = _arr(m, "mesh_box"), _arr(m, "body")
    meta = blob[:pt.NMESH * pt.META].reshape(pt.NMESH, pt.META)
    def with_vertex(mi, k, v):
        b = blob.copy(); off, vp = int(meta[mi, 3]), int(meta[mi, 4])
        b[off + k], b[off + vp + k], b[off + 2 * vp + k] = v
        return b
    for mi in (6, 7, 9):
        v = pt.unpack(blob)[mi]["verts"][0].copy(); v[0] = box[mi, 0] + box[mi, 3] + 1e-9
        rc, msg = _create(m, with_vertex(mi, 0, v))
        assert rc == _abi.MCG_ERR_ARG and "mesh_box" in msg, (mi, rc, msg)
    tried = 0
    for mi in range(pt.NMESH):
        bi = mi if mi < 6 else (5 if mi < 8 else mi - 2)
        corners = box[mi, :3] + np.array([[sx, sy, sz] for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]) * box[mi, 3:] * (1 - 1e-9)
        far = corners[np.argmax(np.linalg.norm(corners, axis=1))]
        if np.linalg.norm(far) <= body[bi, 15] + 1e-9:
            continue
        rc, msg = _create(m, with_vertex(mi, 1, far))
        assert rc == _abi.MCG_ERR_ARG and "hull_rad" in msg, (mi, rc, msg)
        tried += 1
    print(f"\nvertex beyond hull_rad inside mesh_box: refused for {tried} meshes")
    assert tried >= 8


def test_built_in_polytopes_with_a_moved_gripper_are_refused(built):
    """The built-in block (NULL, or passed explicitly) with a model whose flange sits 5 mm further out: the flange's and the gripper
    base's polytopes would be collided 5 mm from where the model puts them."""
    from mycobotgym_amd import _abi
    builtin = _model_and_blob(load_json("mycobot280"))[1]
    spacer = load_json("mycobot280"); spacer["body_pos"][spacer["body_name"].index("flange")][0] += 0.005
    for tab in (spacer, perturbed_table("mycobot280")):
        m, own = _model_and_blob(tab)
        for blob in (None, builtin):
            rc, msg = _create(m, blob)
            assert rc == _abi.MCG_ERR_ARG and "does not fit the model" in msg, (rc, msg)
        assert _passes(*_create(m, own))
    m, _ = _model_and_blob(perturbed_table("mycobot280_mocap"))
    rc, msg = _create(m, None, mocap=True)
    assert rc == _abi.MCG_ERR_ARG and "does not fit the model" in msg, (rc, msg)


def _gate_models():
    spacer = load_json("mycobot280"); spacer["body_pos"][spacer["body_name"].index("flange")][0] += 0.015
    cube = load_json("mycobot280"); cube["geom_size"][cube["geom_name"].index("object0")] = [0.03] * 3
    pads = load_json("mycobot280")
    for g in ("right_finger_layer", "left_finger_layer"):
        h = np.asarray(pads["geom_size"][pads["geom_name"].index(g)], dtype=np.float64)
        pads["geom_size"][pads["geom_name"].index(g)] = list(h * (0.021 / np.linalg.norm(h)))
    return (("15 mm spacer", spacer, "GATE_STATIC_REACH"), ("cube half-size 0.03", cube, "GATE_CUBE_REACH"),
            ("pad half-diagonal 0.021", pads, "GATE_PAD_GROUND"))


@pytest.mark.parametrize("what", ["15 mm spacer", "cube half-size 0.03", "pad half-diagonal 0.021"])
def test_models_beyond_the_broad_phase_gates_are_refused(built, what):
    """The kernels' broad-phase gates are literals tuned to the MyCobot-280 (mcg_cube.hpp: GATE_*): a model whose conservative bounds reach
    them would lose contacts silently, so mcg_create refuses it, naming the gate, even with its own consistent polytope block."""
    from mycobotgym_amd import _abi
    tab, gate = [(t, g) for w, t, g in _gate_models() if w == what][0]
    m, blob = _model_and_blob(tab)
    rc, msg = _create(m, blob)
    print(f"\n{what}: {msg}")
    assert rc == _abi.MCG_ERR_UNSUPPORTED and gate in msg, (rc, msg)


def test_gate_bounds_of_the_shipped_and_perturbed_models(built):
    """The bounds mcg_create checks, recomputed here from the specialised blocks: the built-in and perturbed models stay below every gate
    (they are accepted above), and the margins are printed."""
    for name in ("mycobot280", "mycobot280_mocap"):
        for tab in (load_json(name), perturbed_table(name)):
            s = _spec(tab)
            r, hr, pb = s["body"][:, 0:3], s["body"][:, 15], s["pad_box"]
            n = np.linalg.norm
            reach = max(max(n(r[g]) + hr[g], n(r[g]) + n(r[g + 1]) + hr[g + 1], n(r[10 + sd]) + hr[10 + sd],
                            n(r[g]) + n(r[g + 1]) + n(pb[sd][:3]) + n(pb[sd][3:])) for sd, g in ((0, 6), (1, 8)))
            crad = n(s["cube_half"])
            print(f"{name}: gripper reach {reach:.5f} (< 0.17), + cube radius {reach + crad:.5f} (< 0.2), pad half-diagonal "
                  f"{n(pb[0][3:]):.5f} (< 0.02), cube radius {crad:.5f} (< 0.05)")
            assert reach < 0.17 and reach + crad < 0.2 and n(pb[0][3:]) < 0.02 and crad < 0.05


# ------------------------------------------------------------------------------------------------- initial state of a given table
def _oracle_sites(tab, qpos):
    from oracle import pyoracle as po
    d = po.OracleData(po.OracleModel(tab, enable_contact=False))
    q = np.zeros(tab["nq"]); q[:len(qpos)] = qpos
    d.set_state(qpos=q, qvel=np.zeros(tab["nv"])); d.forward()
    return d.get("site_xpos", (tab["nsite"], 3))


@pytest.mark.parametrize("name,has_object,mocap", [("mycobot280", True, False), ("mycobot280_reach", False, False),
                                                   ("mycobot280_mocap", True, True)])
def test_initial_state_of_a_perturbed_table(built, name, has_object, mocap):
    """initial_state(table=...) against the oracle's forward kinematics of the same table: the EEF site at qpos0, and the z of site object0."""
    from mycobotgym_amd.vec_env import initial_state
    tab = perturbed_table(name)
    qpos, qvel, ctrl, igx, height = initial_state(has_object, False, mocap=mocap, table=tab)
    assert np.array_equal(qpos, np.asarray(tab["qpos0"])[:len(qpos)]) and len(qpos) == (19 if has_object else 12)
    sx = _oracle_sites(tab, qpos)
    e_eef = np.abs(igx - sx[tab["site_name"].index("EEF")]).max()
    _, _, _, igx0, height0 = initial_state(has_object, False, mocap=mocap)
    print(f"\n{name}: EEF site {igx} (built-in {igx0}), |hip - oracle FK| {e_eef:.1e}; height_offset {height:.6f} (built-in {height0:.6f})")
    assert e_eef < 1e-14 and np.abs(igx - igx0).max() > 4e-3
    if has_object:
        e_h = abs(height - sx[tab["site_name"].index("object0")][2])
        print(f"height_offset against the oracle's site object0: {e_h:.1e}")
        assert e_h < 1e-14 and abs(height - height0 - 0.006) < 1e-12


@pytest.mark.parametrize("has_object,fetch,mocap", [(True, False, False), (False, False, False), (True, True, False), (False, True, True),
                                                    (True, False, True)])
def test_initial_state_of_a_built_in_table_is_the_default(built, has_object, fetch, mocap):
    """table=<the built-in table> gives the built-in snapshot bit for bit (MyCobotVecEnv(table=...) then equals MyCobotVecEnv())."""
    from mycobotgym_amd.vec_env import initial_state, load_table
    want = initial_state(has_object, fetch, mocap=mocap)
    got = initial_state(has_object, fetch, mocap=mocap, table=load_table(has_object, mocap=mocap))
    for a, b in zip(want, got):
        assert np.array_equal(np.asarray(a), np.asarray(b)), (a, b)
