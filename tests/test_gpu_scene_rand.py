"""Per-environment scenes on the GPU: mcg_scene_randomize against the numpy restatement (tests/indep_scene_rand.py), mcg_render_scenes
against the independent rules (tests/indep_render.py, tests/indep_render_mounted.py) fed one scene per environment, and the image
environment with ``visual_randomization``.

Shapes: N = 16, 64 x 64 pictures (and one 160 x 120).  Ranges ("world ranges"): camera position +-0.05 m, rotation vector +-5 degrees per
component, fovy x [0.9, 1.1], light tilt up to 30 degrees, the three intensity scales [0.7, 1.3], colours +-0.1; the gripper camera,
5 cm from what it sees, moves by +-0.005 m and +-2 degrees.

Bounds.  Table entries: 1e-12 absolute against the restatement (values O(1), a handful of float64 operations, the restatement has no
fused multiply-add; a wrong key, stream or draw index is off by the size of a range).  Pictures: the criteria and constants of
tests/test_gpu_render.py's ``_compare`` (world camera) and tests/test_gpu_render_mounted.py's (mounted: depth within
1e-4 * depth + 1e-5 / |n.ray|), imported from there; a world picture with more than 2 % unstable pixels fails.  A zero-range table
against mcg_render: same geom ids, colours within 1 level, depth within 1e-5 relative (two float32 evaluations of one formula that the
compiler may contract differently, about 1e-7, with a hundredfold margin).

Measured under the rule alone (CPU): of the 16 downward poses with the jittered gripper camera 15 have 0.12-0.71 % unstable pixels and
are kept (at most 1 %; at least 12 must be), one has 2.9 %.  The draw kernel's text compiled for the host agrees with the restatement
within 7.2e-15 (fovy, a value of 45) and bit for bit at zero ranges.  Every test prints its worst figures ("[scene rand] ..."); they
have NOT been measured on an MI355X yet: no GPU could be had while this file was written.
"""
import json
import math
import os

import numpy as np
import pytest
import torch

from tests import indep_render as ir
from tests import indep_render_mounted as irm
from tests import indep_scene_rand as isr
from tests.common import ROOT, load_json, table_name
from tests.test_gpu_render import DEPTH_RTOL, MAX_UNSTABLE, _compare as compare_world
from tests.test_gpu_render_mounted import KEEP_UNSTABLE, _compare as compare_mounted, _new_worst as new_worst_mounted

pytestmark = pytest.mark.gpu

N = 16
CAMERA = "gripper_camera_rgb"
FLANGE = 4 + 6
PNP = dict(has_object=True, controller_type="joint")
SCALE = (0.7, 1.3)
WORLD_RANGES = {"cam_pos": 0.05, "cam_rot": math.radians(5.0), "fovy_scale": (0.9, 1.1), "light_tilt": math.radians(30.0),
                "light_ambient_scale": SCALE, "light_diffuse_scale": SCALE, "head_scale": SCALE, "rgb": 0.1}
MOUNTED_RANGES = dict(WORLD_RANGES, cam_pos=0.005, cam_rot=math.radians(2.0))
ZERO_RANGES = {"cam_pos": 0.0, "cam_rot": 0.0, "fovy_scale": (1.0, 1.0), "light_tilt": 0.0, "light_ambient_scale": (1.0, 1.0),
               "light_diffuse_scale": (1.0, 1.0), "head_scale": (1.0, 1.0), "rgb": 0.0}
TABLE_TOL = 1e-12


def _np_table(kw=PNP):
    from mycobotgym_amd.model.mjcf import _np_model
    return _np_model(load_json(table_name(kw["has_object"], mocap=kw["controller_type"] == "mocap")))


def _bits(t):
    return (t.detach().cpu().contiguous() if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t))).view(torch.int64)


def _same_bits(a, b):
    return torch.equal(_bits(a), _bits(b))


def _render_all(envs, camera, W, H, samples=1, show_goal=True, **more):
    n, dev = envs.num_envs, envs.device
    out = {"rgb": torch.zeros(n, H, W, 3, dtype=torch.uint8, device=dev), "gray": torch.zeros(n, H, W, dtype=torch.uint8, device=dev),
           "depth": torch.zeros(n, H, W, dtype=torch.float32, device=dev), "geom": torch.zeros(n, H, W, dtype=torch.int8, device=dev)}
    envs.render_into(out, camera=camera, samples=samples, show_goal=show_goal, **more)
    torch.cuda.synchronize()
    return {k: v.cpu().numpy() for k, v in out.items()}


@pytest.fixture(scope="module")
def scene(built):
    from mycobotgym_amd import load_scene
    return load_scene()


@pytest.fixture(scope="module")
def world(scene):
    """The engine of the draws (PickAndPlace-joint, env_id_offset 5, reset(seed=7)), its tables at reset, and after ten seeded random
    steps without auto-reset its state and the kernel's table for ``sideview``: computed once, shared, left unchanged."""
    from mycobotgym_amd import MyCobotVecEnv
    envs = MyCobotVecEnv(N, reward_type="dense", seed=3, env_id_offset=5, auto_reset=False, **PNP)
    envs.reset(seed=7)
    at_reset = {"episode": envs.get_state()["episode"].cpu().numpy(),
                "slots": [envs.randomize_scenes(WORLD_RANGES, camera="sideview", cam_slot=c).cpu().numpy() for c in (0, 1)],
                "zero": envs.randomize_scenes(ZERO_RANGES, camera="sideview", cam_slot=2).cpu()}
    rng = np.random.default_rng(5)
    for _ in range(10):
        envs.step(rng.uniform(-1, 1, (N, envs.action_dim)).astype(np.float32))
    st = envs.get_state()
    tab = envs.randomize_scenes(WORLD_RANGES, camera="sideview", cam_slot=0)
    torch.cuda.synchronize()
    yield {"envs": envs, "at_reset": at_reset, "qpos": st["qpos"].cpu().numpy(), "goal": st["goal"].cpu().numpy(),
           "episode": st["episode"].cpu().numpy(), "table": tab, "rows": tab.cpu().numpy()}
    envs.close()


def test_the_draws_against_the_restatement(scene, world):
    from mycobotgym_amd import _abi
    base = _abi.scene_row(scene, "sideview")
    ep = world["at_reset"]["episode"]
    assert (ep == 1).all()                                            # one reset since the engine was made
    got0, got1 = world["at_reset"]["slots"]
    worst = 0.0
    for slot, got in ((0, got0), (1, got1)):
        want = isr.table(base, WORLD_RANGES, 7, 5 + np.arange(N), ep, cam_slot=slot)
        err = np.abs(got - want).max()
        worst = max(worst, float(err))
        assert err <= TABLE_TOL, (slot, err, np.unravel_index(np.abs(got - want).argmax(), got.shape))
    print(f"\n[scene rand] draws: largest |kernel - restatement| over two slots x {N} rows x 40 entries: {worst:.3e}")
    # a wrong key would still pass a comparison of a table with itself: the jitter is there, and it differs between environments
    assert np.abs(got0[:, :3] - base[:3]).max() > 0.03 and np.unique(got0[:, 0]).size == N
    # light and colours belong to the world, the camera's own jitter to its slot
    assert _same_bits(got0[:, 13:38], got1[:, 13:38])
    assert np.all(np.any(got0[:, :13] != got1[:, :13], axis=1)) and np.all(got0[:, 38:] == 0.0)
    # zero ranges: the base row, bit for bit (signed zeros of the compiled scene included)
    assert _same_bits(world["at_reset"]["zero"], torch.as_tensor(base).repeat(N, 1))
    # the table after ten steps is that of the same episode
    assert (world["episode"] == 1).all() and _same_bits(world["rows"], got0)


def test_keyed_not_stateful(scene):
    from mycobotgym_amd import MyCobotVecEnv
    a = MyCobotVecEnv(N, reward_type="dense", seed=9, **PNP)
    b = MyCobotVecEnv(N // 2, reward_type="dense", seed=9, env_id_offset=N // 2, **PNP)
    a.reset(seed=9); b.reset(seed=9)
    ta, tb = a.randomize_scenes(WORLD_RANGES), b.randomize_scenes(WORLD_RANGES)
    assert _same_bits(ta[N // 2:], tb)                               # the split over engines does not matter
    assert _same_bits(a.randomize_scenes(WORLD_RANGES), ta)          # drawing twice gives the same bits
    mask = torch.zeros(N, dtype=torch.bool, device=a.device); mask[::2] = True
    a.reset(mask=mask)
    after = a.randomize_scenes(WORLD_RANGES)
    ep = a.get_state()["episode"].cpu().numpy()
    assert (ep[::2] == 2).all() and (ep[1::2] == 1).all()
    assert _same_bits(after[1::2], ta[1::2])                         # the episodes that go on keep their scene
    assert bool((after[::2] != ta[::2]).any(dim=1).all())            # a new episode, a new scene
    # with a mask the other rows of `out` are left as they are
    out = torch.full((N, 40), 7.0, dtype=torch.float64, device=a.device)
    ret = a.randomize_scenes(WORLD_RANGES, mask=mask, out=out)
    assert ret is out and bool((out[1::2] == 7.0).all()) and _same_bits(out[::2], after[::2])
    # without `out` they are the base scene's
    from mycobotgym_amd import _abi
    part = a.randomize_scenes(WORLD_RANGES, mask=mask)
    assert _same_bits(part[1::2], torch.as_tensor(_abi.scene_row(scene, "sideview")).repeat(N // 2, 1)) and _same_bits(part[::2], after[::2])
    with pytest.raises(ValueError, match="contiguous float64 device tensor"):
        a.randomize_scenes(WORLD_RANGES, out=torch.zeros(N, 40, dtype=torch.float64))
    with pytest.raises(_abi.McgError, match="cam_slot"):
        a.randomize_scenes(WORLD_RANGES, cam_slot=8)
    a.close(); b.close()


def test_world_camera_pictures_against_the_independent_rule(scene, world):
    from mycobotgym_amd import _abi
    envs, table = world["envs"], _np_table()
    qpos, goal, rows = world["qpos"], world["goal"], world["rows"]
    got = _render_all(envs, "sideview", 64, 64, scenes=world["table"])
    worst = {"unstable": 0.0, "depth": 0.0, "rgb": 0.0}
    per_env = [_abi.scene_from_row(rows[e], target_half=scene["target_half"]) for e in range(N)]
    for e in range(N):
        cam, sc = per_env[e]
        compare_world(f"scenes sideview 64x64 env {e}", got, e, table, qpos[:, e], goal[:, e], sc, cam, 64, 64, True, worst)
    big = _render_all(envs, "sideview", 160, 120, scenes=world["table"])              # not square: fovy is the vertical angle
    cam, sc = per_env[1]
    compare_world("scenes sideview 160x120 env 1", big, 1, table, qpos[:, 1], goal[:, 1], sc, cam, 160, 120, True, worst)
    print(f"\n[scene rand] world camera: largest unstable share {worst['unstable']:.5f} (cap {MAX_UNSTABLE}), worst depth error "
          f"{worst['depth']:.3e} relative (bound {DEPTH_RTOL}), worst colour error {worst['rgb']:.0f} level")
    # sub-sampled gray on environment 0, as tests/test_gpu_render.py does it
    e, s = 0, 2
    cam, sc = per_env[e]
    geoms = ir.scene_triangles(table, qpos[:, e], goal[:, e], sc, True)
    sub = _render_all(envs, "sideview", 64, 64, samples=s, scenes=world["table"])
    acc = np.zeros((64, 64)); ok = np.ones((64, 64), dtype=bool)
    for b in range(s):
        for a in range(s):
            fx, fy = (a + 0.5) / s, (b + 0.5) / s
            ref = ir.picture(table, qpos[:, e], goal[:, e], sc, cam, 64, 64, fx, fy, geoms=geoms)
            ok &= ir.stable_mask(ref, table, qpos[:, e], goal[:, e], sc, cam, 64, 64, fx, fy, geoms=geoms)
            acc += ref["rgb"] @ ir.GRAY_W
    d = np.abs(sub["gray"][e].astype(np.float64) - ir.round_half_up(acc / (s * s)))
    print(f"[scene rand] world camera: samples {s}: gray off by at most {d[ok].max():.0f} level on {ok.mean():.3f} of the pixels")
    assert ok.mean() > 0.8 and d[ok].max() <= 1
    assert np.array_equal(sub["geom"], got["geom"]) and np.array_equal(sub["depth"], got["depth"])


def _downward_poses(table, entry, count=N, seed=1):
    """[19, count]: the recipe of tests/test_gpu_render_mounted.py, restated: qpos0 with the arm's six joints at qpos0 + uniform(-1, 1)
    (default_rng(seed), six numbers per draw, clipped to the joints' ranges), the first `count` draws whose camera looks down (view
    z <= -0.6) from z >= 0.45."""
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


def _carried(table, qpos, cam, body_name="link6"):
    """A camera stated in the frame of an MJCF body -> in the world, by the MJCF tree's own kinematics."""
    from mycobotgym_amd.model.refdyn import kinematics
    qfull = np.asarray(table["qpos0"], dtype=np.float64).copy()
    qfull[:len(qpos)] = qpos[:len(qfull)]
    kin = kinematics(table, qfull)
    b = list(table["body_name"]).index(body_name)
    R, p = np.asarray(kin["xmat"][b]).reshape(3, 3), np.asarray(kin["xpos"][b])
    return {"pos": (p + R @ np.asarray(cam["pos"])).tolist(), "mat": (R @ np.asarray(cam["mat"])).tolist(), "fovy": cam["fovy"]}


SEED_MOUNTED = 11


@pytest.fixture(scope="module")
def down(scene):
    """The downward poses, their rows by the restatement (episode 1 of seed 11: one reset) and the rule's answers: before the GPU is
    touched; shared, left unchanged."""
    from mycobotgym_amd import _abi
    from mycobotgym_amd.model.specialize import specialize
    with open(os.path.join(ROOT, "tests", "golden", "scene_body_cameras.json")) as f:
        entry = json.load(f)["cameras"][CAMERA]
    table = _np_table()
    assert scene["body_cameras"][CAMERA]["body_name"] == "link6"
    qpos = _downward_poses(table, entry)
    target0 = np.asarray(specialize(table)["target0"])
    rows = isr.table(_abi.scene_row(scene, CAMERA), MOUNTED_RANGES, SEED_MOUNTED, np.arange(N), [1] * N, cam_slot=1)
    znear = scene["body_cameras"][CAMERA]["znear"]
    rule = []
    for e in range(N):
        cam, sc = _abi.scene_from_row(rows[e], target_half=scene["target_half"])
        wcam = _carried(table, qpos[:, e], cam)
        solids = irm.scene_solids(table, qpos[:, e], target0, sc, True)
        ref = irm.picture(table, qpos[:, e], target0, sc, wcam, 64, 64, draw_cube=True, solids=solids, znear=znear)
        ok = irm.stable_mask(ref, table, qpos[:, e], target0, sc, wcam, 64, 64, draw_cube=True, solids=solids, znear=znear)
        rule.append((ref, ok))
    share = np.array([1.0 - ok.mean() for _, ok in rule])
    kept = [e for e in range(N) if share[e] <= KEEP_UNSTABLE]
    print(f"\n[scene rand] downward poses, jittered gripper camera: unstable share per pose {np.round(share, 4).tolist()}, kept {len(kept)}")
    assert len(kept) >= 12, share
    return {"qpos": qpos, "rows": rows, "rule": rule, "kept": kept}


def test_the_mounted_camera_against_the_one_sided_rule(scene, down):
    from mycobotgym_amd import MyCobotVecEnv
    envs = MyCobotVecEnv(N, reward_type="dense", seed=SEED_MOUNTED, auto_reset=False, **PNP)
    envs.reset(seed=SEED_MOUNTED)
    nv = envs.get_state()["qvel"].shape[0]
    envs.set_state(qpos=torch.as_tensor(down["qpos"]), qvel=torch.zeros(nv, N, dtype=torch.float64), qpos_lag=torch.as_tensor(down["qpos"]))
    assert (envs.get_state()["episode"].cpu().numpy() == 1).all()
    tab = envs.randomize_scenes(MOUNTED_RANGES, camera=CAMERA, cam_slot=1)
    err = np.abs(tab.cpu().numpy() - down["rows"]).max()
    assert err <= TABLE_TOL, err
    got = _render_all(envs, CAMERA, 64, 64, show_goal=False, scenes=tab)             # show_goal=False: the target box at target0
    worst = new_worst_mounted()
    for e in down["kept"]:
        ref, ok = down["rule"][e]
        compare_mounted(f"scenes down env {e}", got, e, ref, ok, worst)
    assert not (got["geom"] == FLANGE).any()
    print(f"\n[scene rand] mounted camera: table within {err:.3e} of the restatement; largest unstable share {worst['unstable']:.5f}, worst "
          f"depth error {worst['depth_of_bound']:.3f} of its bound ({worst['depth_rel']:.3e} relative), worst colour error {worst['rgb']:.0f} "
          f"level, ids seen {sorted(worst['ids'])}")
    assert len(worst["ids"]) >= 4
    envs.close()


def test_a_table_that_repeats_the_base_scene(scene, world):
    envs, table = world["envs"], _np_table()
    qpos, goal = world["qpos"], world["goal"]
    zero = envs.randomize_scenes(ZERO_RANGES, camera="sideview")
    plain = _render_all(envs, "sideview", 64, 64)                     # mcg_render
    rows = _render_all(envs, "sideview", 64, 64, scenes=zero)
    worst = {"depth": 0.0, "rgb": 0, "gray": 0, "stable": 1.0}
    for e in range(N):
        geoms = ir.scene_triangles(table, qpos[:, e], goal[:, e], scene, True)
        ref = ir.picture(table, qpos[:, e], goal[:, e], scene, "sideview", 64, 64, geoms=geoms)
        ok = ir.stable_mask(ref, table, qpos[:, e], goal[:, e], scene, "sideview", 64, 64, geoms=geoms)
        worst["stable"] = min(worst["stable"], float(ok.mean()))
        assert ok.mean() >= 1.0 - MAX_UNSTABLE, e
        assert np.array_equal(plain["geom"][e][ok], rows["geom"][e][ok]), e
        a, b = plain["depth"][e][ok].astype(np.float64), rows["depth"][e][ok].astype(np.float64)
        hit = np.isfinite(a)
        assert np.array_equal(hit, np.isfinite(b)), e
        rel = np.abs(a[hit] - b[hit]) / a[hit]
        worst["depth"] = max(worst["depth"], float(rel.max()))
        for k in ("rgb", "gray"):
            worst[k] = max(worst[k], int(np.abs(plain[k][e][ok].astype(np.int64) - rows[k][e][ok].astype(np.int64)).max()))
    print(f"\n[scene rand] zero-range table against mcg_render: depth within {worst['depth']:.3e} relative, rgb within {worst['rgb']} level, "
          f"gray within {worst['gray']} level, smallest stable share {worst['stable']:.4f}")
    assert worst["depth"] <= 1e-5 and worst["rgb"] <= 1 and worst["gray"] <= 1
    # a row of NaNs gives a bad picture of its own environment and nothing else
    bad = zero.clone()
    bad[3] = float("nan")
    with pytest.raises(ValueError, match="row 3"):
        envs.render_into({"gray": torch.zeros(N, 64, 64, dtype=torch.uint8, device=envs.device)}, scenes=bad)      # validate=True is the default
    other = _render_all(envs, "sideview", 64, 64, scenes=bad, validate=False)
    keep = np.arange(N) != 3
    assert all(np.array_equal(other[k][keep], rows[k][keep]) for k in rows)
    assert _same_bits(envs.randomize_scenes(ZERO_RANGES, camera="sideview"), zero)        # the engine goes on working
    again = _render_all(envs, "sideview", 64, 64, scenes=zero)
    assert all(np.array_equal(again[k], rows[k]) for k in rows)


def _state_equal(a, b):
    return all(torch.equal(a[k], b[k]) for k in a)


def test_the_image_environment_with_visual_randomization(scene):
    import mycobotgym_amd as mg
    from mycobotgym_amd import _abi
    env_id, n, seed = "MyCobotPickAndPlace-Sparse-IK-v1", N, 4
    cams = ("sideview", CAMERA)
    vr = dict(WORLD_RANGES, cameras={CAMERA: {"cam_pos": MOUNTED_RANGES["cam_pos"], "cam_rot": MOUNTED_RANGES["cam_rot"]}})
    per_cam = [WORLD_RANGES, MOUNTED_RANGES]
    img = mg.make(env_id, n, seed=seed, camera=cams, visual_randomization=vr)
    ref = mg.make(env_id, n, seed=seed, camera=cams)                          # the same id without randomisation
    twin = mg.MyCobotVecEnv(n, seed=seed, auto_reset=False, **{k: v for k, v in mg.spec(env_id).items() if k != "image_obs"})
    obs, info = img.reset(seed=seed); robs, rinfo = ref.reset(seed=seed); twin.reset(seed=seed)
    assert obs.shape == (n, 2, 64, 64) and obs.dtype == torch.uint8 and not torch.equal(obs, robs)
    assert torch.equal(info["desired_goal"], rinfo["desired_goal"])
    bases = [_abi.scene_row(scene, c) for c in cams]

    def fresh_pictures(env):
        """render_into of the current state with freshly drawn tables, one gray plane per camera."""
        planes, tabs = [], []
        for c, cam in enumerate(cams):
            tab = env.randomize_scenes(per_cam[c], camera=cam, cam_slot=c)
            g = {"gray": torch.zeros(n, 64, 64, dtype=torch.uint8, device=env.device)}
            env.render_into(g, camera=cam, samples=env.samples, show_goal=False, scenes=tab)
            planes.append(g["gray"]); tabs.append(tab)
        return torch.stack(planes, dim=1), tabs

    want, tabs = fresh_pictures(img)
    assert torch.equal(obs, want)
    rng = np.random.default_rng(8)
    ends, prev, prev_tabs = 0, img.get_state(), [t.clone() for t in tabs]
    for t in range(60):
        act = rng.uniform(-1, 1, (n, img.action_dim)).astype(np.float32)
        o, r, term, trunc, inf = img.step(act)
        ro, rr, rterm, rtrunc, rinf = ref.step(act)
        # state parity: the pictures' randomisation touches nothing of the physics
        assert torch.equal(r, rr) and torch.equal(term, rterm) and torch.equal(trunc, rtrunc), t
        assert torch.equal(inf["is_success"], rinf["is_success"]) and torch.equal(inf["desired_goal"], rinf["desired_goal"]), t
        assert torch.equal(inf["achieved_goal"], rinf["achieved_goal"]), t
        assert torch.equal(inf["episode"]["r"], rinf["episode"]["r"]) and torch.equal(inf["episode"]["l"], rinf["episode"]["l"]), t
        st = img.get_state()
        assert _state_equal(st, ref.get_state()), t
        # every observation is render_into(..., scenes=...) of the current state with a freshly drawn table
        want, tabs = fresh_pictures(img)
        assert torch.equal(o, want), t
        # default: without randomisation the observation is plain render_into's
        for c, cam in enumerate(cams):
            g = {"gray": torch.zeros(n, 64, 64, dtype=torch.uint8, device=ref.device)}
            ref.render_into(g, camera=cam, samples=ref.samples, show_goal=False)
            assert torch.equal(ro[:, c], g["gray"]), (t, cam)
        done = trunc.clone()
        # an environment's rows are constant within an episode and differ between two
        for c in range(2):
            assert _same_bits(tabs[c][~done], prev_tabs[c][~done]), (t, c)
            assert _same_bits(tabs[c], img._vr_tables[c]), (t, c)
            if done.any():
                assert bool((tabs[c][done] != prev_tabs[c][done]).any(dim=1).all()), (t, c)
        if done.any():
            # final_observation: the finished episode's last state under the finished episode's own scene, its rows recomputed by the
            # restatement from episode - 1
            twin.set_state(**prev)
            twin.step(act)
            idx = torch.nonzero(done).reshape(-1).cpu().numpy()
            ep = st["episode"].cpu().numpy()
            assert np.array_equal(ep[idx] - 1, prev["episode"].cpu().numpy()[idx])
            for c, cam in enumerate(cams):
                old = tabs[c].clone()
                rows = isr.table(bases[c], per_cam[c], seed, idx, ep[idx] - 1, cam_slot=c)
                assert np.abs(rows - prev_tabs[c][done].cpu().numpy()).max() <= TABLE_TOL, (t, c)
                old[done] = torch.as_tensor(rows, device=old.device)
                g = {"gray": torch.zeros(n, 64, 64, dtype=torch.uint8, device=twin.device)}
                twin.render_into(g, camera=cam, samples=img.samples, show_goal=False, scenes=old)
                assert torch.equal(inf["final_observation"][done][:, c], g["gray"][done]), (t, cam)
            assert torch.equal(inf["_final_observation"], done)
            ends += int(done.sum())
        prev, prev_tabs = st, [x.clone() for x in tabs]
    assert ends >= n                                                  # one round of episode ends
    # checkpoint: the tables are a function of the state, state_dict() does not carry them
    sd = img.state_dict()
    assert set(sd) == set(ref.state_dict())
    fresh = mg.make(env_id, n, seed=seed + 1, camera=cams, visual_randomization=vr)
    fresh.load_state_dict(sd)
    act = rng.uniform(-1, 1, (n, img.action_dim)).astype(np.float32)
    a, b = img.step(act), fresh.step(act)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[4]["final_observation"], b[4]["final_observation"])
    assert all(_same_bits(x, y) for x, y in zip(img._vr_tables, fresh._vr_tables))
    with pytest.raises(ValueError, match="not among"):
        mg.make(env_id, 2, visual_randomization={"cameras": {"birdview": {}}})
    for x in (img, ref, twin, fresh):
        x.close()
