"""mcg_render_mounted on the GPU: the gripper camera's pictures against the one-sided independent rule
(tests/indep_render_mounted.py), the world entry through the new one, no side effects, the image environment with the wrist view.

Shapes: 64 x 64 (and one 160 x 120 picture), N = 16.  The camera the rule uses is placed from the MJCF's own attributes
(tests/golden/scene_body_cameras.json) through the MJCF body tree, not from the compiled scene the engine reads.

State sets of the geometry check.
  * "down": the arm's six joints at qpos0 + uniform(-1, 1) (default_rng(1), six numbers per draw, clipped to the joints' ranges), the
    first 16 draws whose camera looks down (view z <= -0.6) from z >= 0.45; put in with set_state.  A picture that sees the horizon has
    12-14.5 % of its pixels unstable under the rule alone (the ground's depth changes by more than 1e-3 per 0.01 pixel there), which
    no implementation can meet; before the GPU is touched the poses whose unstable share is <= 1 % are kept, at least 12 must be.
  * "grasp": scenarios.grasp_state(16, seed=3) after five steps with its action: straight down onto table, cube and fingers.
  * "down, znear 0.07": the same poses with the near plane beyond the hinge links (0.055 m): they vanish in rule and kernel alike.

Bounds.  Stable pixels and the cap on pixels left out (MAX_UNSTABLE = 0.02 per picture) as in tests/test_gpu_render.py.  Depth:
|kernel - rule| <= 1e-4 * depth + OFF_TOL / |n . ray|, OFF_TOL = 1e-5 m: the polytopes' face planes are fitted to the hull's triangles
within 1e-5 m (model/polytope.py: faces_and_edges off_tol), which moves a hit by that over |n . ray| along the ray (n: the rule's own
normal of the face hit); at 5 cm from the camera that alone is 2e-4 relative, the purely relative bound of test_gpu_render.py was sized
for a camera 1 m away.  Colour: one rounding, 1 level.

Measured under the rule alone (CPU): unstable share of the kept downward poses 0.15-0.37 % (one pose of the 16 has 2.69 % and is left
out), 0.98-1.15 % at znear 0.07, 0.27 % for the 160 x 120 picture.  The kernel's worst depth and colour errors are printed by every
test ("[mounted render] ..."); they have NOT been measured on an MI355X yet (no GPU could be had when this file was written).
"""
import json
import os

import numpy as np
import pytest
import torch

from tests import indep_render_mounted as irm
from tests.common import ROOT, load_json, table_name

pytestmark = pytest.mark.gpu

CAMERA = "gripper_camera_rgb"
FLANGE = 4 + 6
MAX_UNSTABLE = 0.02
KEEP_UNSTABLE = 0.01
DEPTH_RTOL, OFF_TOL = 1e-4, 1e-5
N = 16
PNP = dict(has_object=True, controller_type="joint")


def _np_table(kw):
    from mycobotgym_amd.model.mjcf import _np_model
    return _np_model(load_json(table_name(kw["has_object"], mocap=kw["controller_type"] == "mocap")))


def _entry():
    with open(os.path.join(ROOT, "tests", "golden", "scene_body_cameras.json")) as f:
        return json.load(f)["cameras"][CAMERA]


@pytest.fixture(scope="module")
def scene(built):
    from mycobotgym_amd import load_scene
    return load_scene()


def _render_all(envs, camera, W, H, samples=1, show_goal=True, mask=None, **more):
    n, dev = envs.num_envs, envs.device
    out = {"rgb": torch.zeros(n, H, W, 3, dtype=torch.uint8, device=dev), "gray": torch.zeros(n, H, W, dtype=torch.uint8, device=dev),
           "depth": torch.zeros(n, H, W, dtype=torch.float32, device=dev), "geom": torch.zeros(n, H, W, dtype=torch.int8, device=dev)}
    envs.render_into(out, camera=camera, samples=samples, show_goal=show_goal, mask=mask, **more)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


def _downward_poses(table, entry, count=N, seed=1):
    """[19, count]: qpos0 with the arm's joints redrawn until `count` poses look down from high enough (the recipe in the docstring)."""
    q0 = np.asarray(table["qpos0"], dtype=np.float64)
    lo, hi = np.asarray(table["jnt_range"], dtype=np.float64)[:6].T
    rng = np.random.default_rng(seed)
    kept = []
    while len(kept) < count:
        q = q0.copy()
        q[:6] = np.clip(q0[:6] + rng.uniform(-1, 1, 6), lo, hi)
        cam = irm.mounted_camera(table, q, entry)
        if -np.asarray(cam["mat"])[2, 2] <= -0.6 and cam["pos"][2] >= 0.45:
            kept.append(q)
    return np.stack(kept, axis=1)


def _rule(table, qpos, target, scene, cam, W, H, draw_cube, znear):
    solids = irm.scene_solids(table, qpos, target, scene, draw_cube)
    ref = irm.picture(table, qpos, target, scene, cam, W, H, draw_cube=draw_cube, solids=solids, znear=znear)
    ok = irm.stable_mask(ref, table, qpos, target, scene, cam, W, H, draw_cube=draw_cube, solids=solids, znear=znear)
    return ref, ok


def _compare(tag, got, e, ref, ok, worst):
    """Geometry and colour of environment e's picture (samples = 1) against the rule's (ref, stable mask); updates `worst`, asserts."""
    share = 1.0 - ok.mean()
    worst["unstable"] = max(worst["unstable"], share)
    assert share <= MAX_UNSTABLE, f"{tag}: {share:.4f} of the pixels are unstable under the rule alone (cap {MAX_UNSTABLE})"
    gid, dep, rgb = got["geom"][e].astype(np.int64), got["depth"][e].astype(np.float64), got["rgb"][e].astype(np.float64)
    bad = ok & (gid != ref["geom"])
    assert not bad.any(), f"{tag}: {bad.sum()} stable pixels show another geom, first {np.argwhere(bad)[0]}: kernel {gid[bad][0]} rule {ref['geom'][bad][0]}"
    sky = ~np.isfinite(ref["depth"])
    assert np.all(np.isposinf(dep[ok & sky]))
    m = ok & ~sky
    err = np.abs(dep[m] - ref["depth"][m])
    bound = DEPTH_RTOL * ref["depth"][m] + OFF_TOL / ref["ndot"][m]
    if err.size:
        worst["depth_of_bound"] = max(worst["depth_of_bound"], float((err / bound).max()))
        worst["depth_rel"] = max(worst["depth_rel"], float((err / ref["depth"][m]).max()))
        assert (err <= bound).all(), f"{tag}: depth off by {(err / bound).max():.3f} of its bound ({(err / ref['depth'][m]).max():.3e} relative)"
    dc = np.abs(rgb - irm.ir.round_half_up(ref["rgb"])).max(-1)
    worst["rgb"] = max(worst["rgb"], float(dc[ok].max()))
    assert dc[ok].max() <= 1, f"{tag}: colour off by {dc[ok].max()} levels"
    worst["ids"] |= set(np.unique(ref["geom"][ok]).tolist())


def _new_worst():
    return {"unstable": 0.0, "depth_of_bound": 0.0, "depth_rel": 0.0, "rgb": 0.0, "ids": set()}


def _report(name, worst):
    print(f"\n[mounted render] {name}: largest unstable share {worst['unstable']:.5f}, worst depth error {worst['depth_of_bound']:.3f} of its "
          f"bound ({worst['depth_rel']:.3e} relative), worst colour error {worst['rgb']:.0f} level, ids seen {sorted(worst['ids'])}")
    assert len(worst["ids"]) >= 4, worst["ids"]


@pytest.fixture(scope="module")
def down(scene):
    """The downward poses and the rule's answers for them (computed once, before the GPU is touched; shared, left unchanged)."""
    table, entry = _np_table(PNP), _entry()
    qpos = _downward_poses(table, entry)
    from mycobotgym_amd.model.specialize import specialize
    target0 = np.asarray(specialize(table)["target0"])
    cams = [irm.mounted_camera(table, qpos[:, e], entry) for e in range(N)]
    rule = {}
    for znear in (scene["body_cameras"][CAMERA]["znear"], 0.07):
        rule[znear] = [_rule(table, qpos[:, e], target0, scene, cams[e], 64, 64, True, znear) for e in range(N)]
    share = np.array([1.0 - ok.mean() for _, ok in rule[scene["body_cameras"][CAMERA]["znear"]]])
    kept = [e for e in range(N) if share[e] <= KEEP_UNSTABLE]
    print(f"\n[mounted render] downward poses: unstable share per pose {np.round(share, 4).tolist()}, kept {len(kept)}")
    assert len(kept) >= 12, share
    return {"table": table, "qpos": qpos, "target0": target0, "cams": cams, "rule": rule, "kept": kept}


def _engine_at(qpos, seed=11):
    from mycobotgym_amd import MyCobotVecEnv
    envs = MyCobotVecEnv(N, reward_type="dense", seed=seed, auto_reset=False, **PNP)
    envs.reset(seed=seed)
    nv = envs.get_state()["qvel"].shape[0]
    envs.set_state(qpos=torch.as_tensor(qpos), qvel=torch.zeros(nv, N, dtype=torch.float64), qpos_lag=torch.as_tensor(qpos))
    assert np.array_equal(envs.get_state()["qpos"].cpu().numpy(), qpos)
    return envs


@pytest.mark.parametrize("znear", [None, 0.07], ids=["down", "down-znear-0.07"])
def test_downward_poses_against_the_one_sided_rule(scene, down, znear):
    zn = scene["body_cameras"][CAMERA]["znear"] if znear is None else znear
    envs = _engine_at(down["qpos"])
    got = _render_all(envs, CAMERA, 64, 64, show_goal=False, znear=znear)          # show_goal=False: the target box at target0
    worst = _new_worst()
    for e in down["kept"]:
        ref, ok = down["rule"][zn][e]
        _compare(f"down znear {zn} env {e}", got, e, ref, ok, worst)
    assert not (got["geom"] == FLANGE).any()
    if znear is not None:
        assert got["depth"].min() >= 0.07 * (1 - 1e-6)
        plain = _render_all(envs, CAMERA, 64, 64, show_goal=False)
        hinge = (plain["geom"] == 4 + 12) | (plain["geom"] == 4 + 13)
        assert (plain["depth"][hinge] < 0.07).any() and plain["depth"].min() < 0.07       # what the plane cuts was there without it
    else:
        # one picture that is not square: fovy is the vertical angle
        e = down["kept"][0]
        ref, ok = _rule(down["table"], down["qpos"][:, e], down["target0"], scene, down["cams"][e], 160, 120, True, zn)
        big = _render_all(envs, CAMERA, 160, 120, show_goal=False)
        _compare(f"down 160x120 env {e}", big, e, ref, ok, worst)
        assert not (big["geom"] == FLANGE).any()
    _report(f"down, znear {zn}", worst)
    envs.close()


def test_grasp_states_against_the_one_sided_rule(scene):
    from mycobotgym_amd import MyCobotVecEnv
    from mycobotgym_amd.scenarios import grasp_state
    table, entry = _np_table(PNP), _entry()
    envs = MyCobotVecEnv(N, reward_type="dense", seed=11, auto_reset=False, **PNP)
    envs.reset(seed=11)
    st = grasp_state(N, seed=3)
    act = st.pop("action")
    envs.set_state(**{k: torch.as_tensor(v) for k, v in st.items()})
    for _ in range(5):
        envs.step(act)
    s = envs.get_state()
    qpos, goal = s["qpos"].cpu().numpy(), s["goal"].cpu().numpy()
    zn = scene["body_cameras"][CAMERA]["znear"]
    got = _render_all(envs, CAMERA, 64, 64)                    # the target box at the goal, as render() draws it
    worst = _new_worst()
    for e in range(N):
        cam = irm.mounted_camera(table, qpos[:, e], entry)
        ref, ok = _rule(table, qpos[:, e], goal[:, e], scene, cam, 64, 64, True, zn)
        _compare(f"grasp env {e}", got, e, ref, ok, worst)
    assert not (got["geom"] == FLANGE).any()
    _report("grasp", worst)
    envs.close()


def test_world_camera_through_the_mounted_entry_is_mcg_render(scene):
    """mcg_render_mounted(body = -1, znear = 0) against mcg_render, all four outputs, byte for byte; states of a 50-step pnp-IK rollout.

    That call runs the world camera's own kernel.  The mounted kernel with the world as its carrier (body = -1 and a near plane nothing
    reaches) is a different instantiation: the compiler contracts a * b + c into one rounding or two as it sees fit in each (the two
    differ in their packed multiply / add / fma counts), so its pictures agree with the world kernel's within float32 rounding, not bit
    for bit.  It is held to the independent rule instead, by the criteria of every other picture here."""
    import ctypes as C
    from mycobotgym_amd import MyCobotVecEnv, _abi
    envs = MyCobotVecEnv(N, reward_type="dense", seed=11, auto_reset=False, has_object=True, controller_type="IK")
    envs.reset(seed=11)
    rng = np.random.default_rng(5)
    for _ in range(50):
        envs.step(rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32))
    sc = _abi.McgScene.from_dict(scene, "sideview")
    def draw(entry, samples, *head):
        out = {"rgb": torch.zeros(N, 64, 64, 3, dtype=torch.uint8, device=envs.device), "gray": torch.zeros(N, 64, 64, dtype=torch.uint8, device=envs.device),
               "depth": torch.zeros(N, 64, 64, dtype=torch.float32, device=envs.device), "geom": torch.zeros(N, 64, 64, dtype=torch.int8, device=envs.device)}
        ro = _abi.McgRenderOut(**{k: t.data_ptr() for k, t in out.items()})
        with torch.cuda.device(envs.device):
            _abi.check(getattr(envs._lib, entry)(envs._h, C.byref(sc), *head, 64, 64, samples, 1, None, C.byref(ro), envs._stream()), entry)
        torch.cuda.synchronize()
        return {k: v.cpu().numpy() for k, v in out.items()}
    for samples in (1, 2):
        a = draw("mcg_render", samples)
        b = draw("mcg_render_mounted", samples, -1, 0.0)
        assert all(np.array_equal(a[k], b[k]) for k in a), samples
        assert len(np.unique(a["geom"])) >= 4
    # the mounted kernel itself with the world as the carrier, and a near plane nothing reaches (the world cameras stand about 1 m off)
    c = draw("mcg_render_mounted", 1, -1, 1e-3)
    kw = dict(has_object=True, controller_type="IK")
    table = _np_table(kw)
    st = envs.get_state()
    qpos, goal = st["qpos"].cpu().numpy(), st["goal"].cpu().numpy()
    worst = _new_worst()
    for e in range(4):
        ref, ok = _rule(table, qpos[:, e], goal[:, e], scene, scene["cameras"]["sideview"], 64, 64, True, 1e-3)
        _compare(f"world carrier env {e}", c, e, ref, ok, worst)
    _report("sideview through the mounted kernel", worst)
    envs.close()


def _state_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_no_side_effects_determinism_and_mask(scene):
    from mycobotgym_amd import MyCobotVecEnv
    kw = dict(has_object=True, controller_type="IK")
    a = MyCobotVecEnv(N, reward_type="sparse", seed=2, **kw); b = MyCobotVecEnv(N, reward_type="sparse", seed=2, **kw)
    a.reset(seed=2); b.reset(seed=2)
    rng = np.random.default_rng(9)
    for t in range(20):
        act = rng.uniform(-1, 1, (N, a.action_dim)).astype(np.float32)
        oa = a.step(act); ob = b.step(act)
        a.render(camera=CAMERA, width=64, height=64)
        for x, y in zip(oa[:4], ob[:4]):
            if isinstance(x, dict):
                assert all(torch.equal(x[k], y[k]) for k in x), t
            else:
                assert torch.equal(x, y), t
    assert _state_equal(a.get_state(), b.get_state())
    one = _render_all(a, CAMERA, 64, 64, samples=2); two = _render_all(a, CAMERA, 64, 64, samples=2)
    assert all(np.array_equal(one[k], two[k]) for k in one)
    assert len(np.unique(one["geom"])) >= 4 and not (one["geom"] == FLANGE).any()
    # the arms differ, so the wrist views do (a world camera's picture of two environments differs only where the scene does)
    assert not np.array_equal(one["rgb"][0], one["rgb"][1])
    dev = a.device
    out = {"rgb": torch.full((N, 48, 64, 3), 7, dtype=torch.uint8, device=dev), "depth": torch.full((N, 48, 64), -1.0, device=dev)}
    mask = torch.zeros(N, dtype=torch.bool, device=dev); mask[::3] = True
    a.render_into(out, camera=CAMERA, mask=mask)
    full = {"rgb": torch.zeros_like(out["rgb"]), "depth": torch.zeros_like(out["depth"])}
    a.render_into(full, camera=CAMERA)
    assert (out["rgb"][~mask] == 7).all() and (out["depth"][~mask] == -1.0).all()
    assert torch.equal(out["rgb"][mask], full["rgb"][mask]) and torch.equal(out["depth"][mask], full["depth"][mask])
    with pytest.raises(ValueError, match="unknown camera"):
        a.render(camera="wrist")
    a.close(); b.close()


@pytest.mark.parametrize("env_id", ["MyCobotPickAndPlace-Sparse-IK-v1", "MyCobotReach-Sparse-joint-v1"])
def test_image_environment_with_the_gripper_camera(scene, env_id):
    import mycobotgym_amd as mg
    n, seed = N, 4
    img = mg.make(env_id, num_envs=n, seed=seed, camera=CAMERA)
    both = mg.make(env_id, num_envs=n, seed=seed, camera=("sideview", CAMERA))
    side = mg.make(env_id, num_envs=n, seed=seed)
    ref = mg.make(env_id.replace("-v1", "-v0"), num_envs=n, seed=seed)
    twin = mg.make(env_id, num_envs=n, seed=seed, camera=CAMERA, auto_reset=False)      # keeps the pre-reset state of a finished episode
    assert img.single_observation_space.shape == (1, 64, 64) and img.observation_space.shape == (n, 1, 64, 64)
    assert both.single_observation_space.shape == (2, 64, 64) and both.observation_space.shape == (n, 2, 64, 64)
    assert both.single_observation_space.dtype == np.uint8
    obs, info = img.reset(seed=seed); bobs, _ = both.reset(seed=seed); sobs, _ = side.reset(seed=seed); robs, _ = ref.reset(seed=seed)
    twin.reset(seed=seed)
    assert obs.shape == (n, 1, 64, 64) and obs.dtype == torch.uint8 and bobs.shape == (n, 2, 64, 64) and bobs.dtype == torch.uint8
    assert torch.equal(bobs[:, 0], sobs[:, 0]) and torch.equal(bobs[:, 1], obs[:, 0]) and not torch.equal(obs, sobs)
    assert torch.equal(info["desired_goal"], robs["desired_goal"])
    rng = np.random.default_rng(8)
    ends = 0
    prev = img.get_state()
    for t in range(60):
        act = rng.uniform(-1, 1, (n, img.action_dim)).astype(np.float32)
        o, r, term, trunc, inf = img.step(act)
        bo, br, _, btrunc, binf = both.step(act)
        so, _, _, _, sinf = side.step(act)
        ro, rr, rterm, rtrunc, rinf = ref.step(act)
        assert torch.equal(r, rr) and torch.equal(term, rterm) and torch.equal(trunc, rtrunc) and torch.equal(br, rr), t
        assert torch.equal(inf["is_success"], rinf["is_success"]) and torch.equal(inf["desired_goal"], ro["desired_goal"]), t
        assert torch.equal(inf["achieved_goal"], ro["achieved_goal"]), t
        assert _state_equal(img.get_state(), ref.get_state()) and _state_equal(both.get_state(), ref.get_state()), t
        # the observation is render_into's gray of the same state
        g = {"gray": torch.zeros(n, 64, 64, dtype=torch.uint8, device=img.device)}
        img.render_into(g, camera=CAMERA, samples=img.samples, show_goal=False)
        assert torch.equal(o[:, 0], g["gray"]), t
        # two cameras: one channel each, in the order given
        assert bo.shape == (n, 2, 64, 64) and torch.equal(bo[:, 0], so[:, 0]) and torch.equal(bo[:, 1], o[:, 0]), t
        done = trunc.clone()
        if done.any():
            twin.set_state(**prev)
            twin.step(act)
            assert torch.equal(inf["final_observation"][done], twin._img[done]), t
            assert torch.equal(inf["_final_observation"], done)
            fb = binf["final_observation"]
            assert fb.shape == (n, 2, 64, 64)
            assert torch.equal(fb[done][:, 1], inf["final_observation"][done][:, 0]), t
            assert torch.equal(fb[done][:, 0], sinf["final_observation"][done][:, 0]), t
            ends += int(done.sum())
        prev = img.get_state()
    assert ends >= n
    for x in (img, both, side, ref, twin):
        x.close()
