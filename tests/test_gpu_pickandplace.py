"""GPU parity for PickAndPlace (has_object): cube free joint, box/plane contacts, 25-number observation, object reset.

Same method as tests/test_gpu_parity.py: sub-steps compared from identical state (teacher-forced) because free-running
trajectories are chaotic; reset draws bit-exact.
"""
import numpy as np
import pytest

from tests.common import torch_cuda  # noqa: F401

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("controller", ["joint", "IK"])
def test_reset_bit_exact_with_object(torch_cuda, controller):
    from tests.common import make_pair
    envs, ora = make_pair(512, has_object=True, controller_type=controller, seed=21)
    obs, _ = envs.reset(seed=21)
    o_obs, o_ag, o_dg = ora.reset(seed=21)
    assert obs["observation"].shape == (512, 25)
    assert np.array_equal(obs["desired_goal"].cpu().numpy(), o_dg)
    assert np.array_equal(obs["achieved_goal"].cpu().numpy(), o_ag)             # cube xy from the same Philox draws
    assert np.abs(obs["observation"].cpu().numpy() - o_obs).max() < 1e-14
    envs.close()


def _substep_run(torch, n, steps, prepare=None, seed=5, hold_pose=False, table=None):
    from tests.common import make_pair, sync_oracle_to, step_errors
    kw = dict(has_object=True, controller_type="joint", reward_type="dense", seed=seed, frame_skip=1, max_episode_steps=10 ** 9)
    envs, ora = make_pair(n, table=table, **kw)
    envs.reset(seed=seed); ora.reset(seed=seed)
    if prepare is not None:
        prepare(ora)
    rng = np.random.default_rng(3)
    worst = dict(obs=0.0, qpos=0.0, qvel=0.0)
    ncon_seen = set()
    for t in range(steps):
        if t % 20 == 0:
            a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
            if hold_pose:        # joint controller: ctrl := action; stay near the prepared pose (clipped to [-1, 1] by the env)
                a = (ora.get_state()["ctrl"] + 0.05 * rng.normal(size=(n, 7))).astype(np.float32)
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        st, so = envs.get_state(), ora.get_state()
        worst["obs"] = max(worst["obs"], e.max())
        worst["qpos"] = max(worst["qpos"], np.abs(st["qpos"].cpu().numpy().T - so["qpos"]).max())
        worst["qvel"] = max(worst["qvel"], np.abs(st["qvel"].cpu().numpy().T - so["qvel"]).max())
        for i in range(0, n, 8):
            ncon_seen.add(int(ora.data(i).get("ncon", (1,), np.int32)[0]))
    envs.close()
    return worst, ncon_seen


def test_substeps_cube_resting_on_table(torch_cuda):
    worst, ncon = _substep_run(torch_cuda, 128, 400)
    print(f"\nresting cube, 400 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert 4 in ncon
    assert worst["obs"] < 1e-13 and worst["qpos"] < 1e-12 and worst["qvel"] < 5e-10      # measured 5.6e-16, 1.0e-14, 5.2e-12


def test_contact_rule_keyframe_variant(torch_cuda):
    """contact_rule="keyframe": Rpy = 4 mu^2 R in the kernels (mcg_model.contact_rpy) and in the oracle (rule[3] = 2).  Per-sub-step parity
    of the variant with the cube settling on the table and during a grasp, and the rest height the reference's keyframes store
    (z = 0.209981: penetration 1.85e-5 .. 1.95e-5, mycobot280.xml:6) reached on the GPU."""
    torch = torch_cuda
    from tests.common import make_pair, sync_oracle_to, step_errors
    n = 64
    kw = dict(has_object=True, controller_type="joint", reward_type="dense", seed=5, frame_skip=1, max_episode_steps=10 ** 9, contact_rule="keyframe")
    envs, ora = make_pair(n, **kw)
    envs.reset(seed=5); ora.reset(seed=5)
    _grasp_state(ora, n)
    a = np.clip(np.tile(np.concatenate([ora.get_state()["ctrl"][0, :6], [1.0]]).astype(np.float32), (n, 1)), -1, 1)
    worst = 0.0
    for t in range(150):
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        worst = max(worst, e.max())
    # and free-running at rest: the kernels alone settle at the keyframes' height
    rest = MyCobotVecEnvRest(torch, "keyframe"); base = MyCobotVecEnvRest(torch, "mujoco")
    print(f"\ncontact_rule=keyframe: 150 sub-steps through a grasp, max obs error {worst:.2e}; cube rest penetration on the GPU {rest:.3e} "
          f"(default rule {base:.3e}; the reference's keyframes 1.85e-5 .. 1.95e-5)")
    assert worst < 1e-10
    assert 1.85e-5 <= rest <= 1.95e-5 and 9.0e-6 < base < 1.0e-5
    envs.close()


def MyCobotVecEnvRest(torch, rule):
    """Penetration of the resting cube after 40 env-steps with the arm parked (joint controller holding its initial pose)."""
    from mycobotgym_amd import MyCobotVecEnv
    envs = MyCobotVecEnv(32, has_object=True, controller_type="joint", reward_type="dense", seed=0, contact_rule=rule, max_episode_steps=10 ** 9)
    envs.reset(seed=0)
    hold = envs.get_state()["qpos"][:7].T.clone().float(); hold[:, 6] = 0
    for _ in range(40): envs.step(hold)
    z = envs.get_state()["qpos"][14].double()
    envs.close()
    return float((0.21 - z).mean())


def _contact_poses(kind, count=128, seed=0, table=None):
    """Rejection-sampled arm poses (cube at rest on the table) with a SHALLOW contact of the wanted kind (a deep one is a violent
    state).  kind "pad": a finger pad on the table / the ground, no mesh contact; kind "mesh": a mesh geom of the arm or the gripper (collision
    polytope, condim 3: 4 rows) on the table / the ground.  `table`: another model table than the built-in one."""
    from tests.common import load_json
    from oracle import pyoracle as po
    tab = table if table is not None else load_json("mycobot280")
    m = po.OracleModel(tab, enable_contact=True, scope_geom=tab["geom_name"].index("object0"))
    d = po.OracleData(m)
    rng = np.random.default_rng(seed)
    poses = []
    while len(poses) < count:
        q = np.array(tab["qpos0"], float)
        q[:6] = rng.uniform(-2.5, 2.5, 6); q[6] = q[8] = rng.uniform(0, 0.7)
        d.set_state(qpos=q, qvel=np.zeros(18)); d.forward()
        n = int(d.get("ncon", (1,), np.int32)[0]); nefc = int(d.get("nefc", (1,), np.int32)[0])
        if n <= 4: continue
        rows = d.get("efc_type", (416,), np.int32)[:nefc] == 2                      # contact rows (pyramid)
        ids = d.get("efc_id", (416,), np.int32)[:nefc][rows]
        per_contact = np.bincount(ids)
        has_mesh = bool((per_contact == 4).any())                                  # condim 3
        has_pad = int((per_contact == 6).sum()) > 4                                # condim 4 beyond the cube's four
        if d.get("efc_pos", (416,))[:nefc][rows].min() <= -2e-3: continue
        if kind == "gripper_mesh":
            raw = d.get("contact", (64, 28))
            gm = {g for g in range(tab["ngeom"]) if tab["geom_type"][g] == 7 and ("finger" in tab["geom_mesh"][g] or "gear" in tab["geom_mesh"][g] or "hinge" in tab["geom_mesh"][g])}
            if any(int(raw[c, 26:28].copy().view(np.int32)[2]) in gm for c in range(n)): poses.append(q)
            continue
        if (kind == "mesh" and has_mesh) or (kind == "pad" and has_pad and not has_mesh): poses.append(q)
    return np.array(poses)


def _cap_poses(count=48, seed=11, depth=-2.5e-2):
    """Arm poses whose contact list is cut by the cap of 16 entries (mesh entries come last in the pair order and are the ones cut).  Such
    poses are deep ones under uniform sampling -- an arm folded into the table; the shallowest are kept."""
    from tests.common import load_json
    from oracle import pyoracle as po
    tab = load_json("mycobot280")
    m = po.OracleModel(tab, enable_contact=True, scope_geom=tab["geom_name"].index("object0"))
    d = po.OracleData(m)
    rng = np.random.default_rng(seed)
    poses = []; tries = 0
    while len(poses) < count and tries < 400000:
        tries += 1
        q = np.array(tab["qpos0"], float)
        q[:6] = rng.uniform(-2.5, 2.5, 6); q[6] = q[8] = rng.uniform(0, 0.7)
        d.set_state(qpos=q, qvel=np.zeros(18)); d.forward()
        if int(d.get("ndrop", (1,), np.int32)[0]) == 0: continue
        nefc = int(d.get("nefc", (1,), np.int32)[0])
        rows = d.get("efc_type", (416,), np.int32)[:nefc] == 2
        if d.get("efc_pos", (416,))[:nefc][rows].min() > depth: poses.append(q)
    return np.array(poses)


def _pose_prepare(poses):
    def prepare(ora):
        s = ora.get_state()
        s["qpos"][:, :12] = poses[:, :12]; s["qpos_lag"] = s["qpos"].copy()
        s["ctrl"][:, :6] = poses[:, :6]; s["ctrl"][:, 6] = poses[:, 6] / 0.7
        ora.set_state(**s)
    return prepare


def test_substeps_finger_pads_on_the_table_and_the_ground(torch_cuda):
    """Arm poses that press a finger pad onto the table top or onto the ground plane next to the table (box-box / plane-box
    contacts with rows in the robot's dofs only, mycobot280_main.xml:81,87-88,195-199,222-225), cube resting or being pushed."""
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=_pose_prepare(_contact_poses("pad")), hold_pose=True)
    print(f"\npads on the table / ground, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) > 4
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_arm_meshes_on_the_table_and_the_ground(torch_cuda):
    """the mesh geoms (their collision polytopes, exact separating-axis test) against the table and the ground: one condim-3
    contact per mesh on the axis of least penetration, duplicated visual/collision meshes as one entry of double weight."""
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=_pose_prepare(_contact_poses("mesh", seed=1)), hold_pose=True)
    print(f"\narm meshes on the table / ground, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) > 4
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_with_the_cap_cutting_the_list(torch_cuda):
    """The list at the cap of MAXCON = 16 entries: the mesh phase appends behind the primitive pairs' contacts until the list is full and
    counts what it cuts, as the oracle's pair order does.  Per-sub-step parity on such states (teacher-forced), and the kernels' own
    count of cut contacts."""
    poses = _cap_poses()
    n = len(poses)
    assert n >= 8, "too few capped poses found"
    from tests.common import make_pair, sync_oracle_to, step_errors
    kw = dict(has_object=True, controller_type="joint", reward_type="dense", seed=5, frame_skip=1, max_episode_steps=10 ** 9)
    envs, ora = make_pair(n, **kw)
    envs.reset(seed=5); ora.reset(seed=5)
    _pose_prepare(poses)(ora)
    sync_oracle_to(envs, ora)
    kc = envs.debug_contacts()
    at_cap = int((kc["count"] >= 16).sum()); cut = int((kc["dropped"] > 0).sum())
    odrop = sum(int(ora.data(i).get("ndrop", (1,), np.int32)[0]) for i in range(n))
    assert int(kc["dropped"].sum()) == odrop, (int(kc["dropped"].sum()), odrop)
    envs.counters(clear=True)
    a = np.clip(ora.get_state()["ctrl"], -1, 1).astype(np.float32)
    worst = dict(obs=0.0, qpos=0.0)
    for t in range(6):                                            # a few sub-steps: the deep ones among these states blow up soon after
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        st, so = envs.get_state(), ora.get_state()
        worst["obs"] = max(worst["obs"], float(e.max()))
        worst["qpos"] = max(worst["qpos"], float(np.abs(st["qpos"].cpu().numpy().T - so["qpos"]).max()))
    dropped = envs.counters()["contacts_dropped"]
    print(f"\nlists at the cap, 6 sub-steps x {n} envs: {worst}; envs at the cap {at_cap}, with cut contacts {cut}; contacts cut over the run (mcg_counters) {dropped}")
    assert at_cap >= n // 2 and cut > 0 and dropped > 0
    assert worst["obs"] < 1e-9 and worst["qpos"] < 1e-9
    envs.close()


def test_whole_env_step_from_random_policy_states(torch_cuda):
    """One WHOLE env-step (20 sub-steps inside one launch: what the teacher-forced per-sub-step tests cannot see -- staging areas, flags and
    carried active sets that live from one sub-step to the next) against the oracle, from states a random IK policy reached on the GPU:
    half of the picked environments hold an arm-mesh contact (the staged / merged entries of the M / RNE waves), half do not."""
    torch = torch_cuda
    from mycobotgym_amd import MyCobotVecEnv
    from tests.common import make_pair, step_errors
    n0 = 2048
    src = MyCobotVecEnv(n0, has_object=True, controller_type="IK", reward_type="dense", seed=3)
    src.reset(seed=3)
    g = torch.Generator(device="cuda"); g.manual_seed(99)
    for t in range(80): src.step_async(torch.rand(n0, src.action_dim, device="cuda", generator=g) * 2 - 1)
    torch.cuda.synchronize()
    st = {k: v.cpu() for k, v in src.get_state().items()}
    kc = src.debug_contacts()
    ty, cnt = kc["type"].cpu(), kc["count"].cpu()
    src.close()
    live = torch.arange(ty.shape[1])[None, :] < cnt[:, None]
    arm = ((ty >= 5) & (ty < 19) & live).any(dim=1)
    n = 128
    pick = torch.cat([arm.nonzero().flatten()[: n // 2], (~arm).nonzero().flatten()[: n - min(n // 2, int(arm.sum()))]])[:n]
    n = len(pick)
    assert int(arm[pick].sum()) >= 16, "the random policy reached too few arm-mesh contacts"
    envs, ora = make_pair(n, has_object=True, controller_type="joint", reward_type="dense", seed=0, max_episode_steps=10 ** 9)
    envs.reset(seed=0); ora.reset(seed=0)
    sel = {k: (v[..., pick] if v.ndim and v.shape[-1] == n0 else v) for k, v in st.items()}
    ost = {k: sel[k].numpy().T.copy() for k in ("qpos", "qvel", "warm", "qpos_lag", "goal", "ctrl")}
    ost["elapsed"] = np.zeros(n, np.int32); ost["episode"] = sel["episode"].numpy().astype(np.int32)
    ora.set_state(**ost)
    envs.set_state(qpos=sel["qpos"], qvel=sel["qvel"], ctrl=sel["ctrl"], warm=sel["warm"], qpos_lag=sel["qpos_lag"], goal=sel["goal"],
                   elapsed=torch.zeros(n, dtype=torch.int32), episode=sel["episode"])
    a = np.clip(ost["ctrl"] + 0.05 * np.random.default_rng(1).normal(size=(n, 7)), -1, 1).astype(np.float32)      # joint targets near the reached pose
    e, flags_equal, o = step_errors(envs, ora, a)
    assert flags_equal
    isarm = arm[pick].numpy()
    print(f"\none env-step (20 sub-steps, one launch) from random-policy states: max error vs oracle {e[isarm].max():.2e} over {int(isarm.sum())} envs with an "
          f"arm-mesh contact, {e[~isarm].max():.2e} over {int((~isarm).sum())} without")
    assert e.max() < 1e-9                                          # measured 5e-12 / 7e-14 here, 3e-11 / 2e-12 over 256 envs (tools/state_vs_oracle.py)
    envs.close()
    # ... and the same states under the reference's DEFAULT controller (IK: 100 sub-steps in one launch), judged on the arm-contact subset
    # by the oracle's own sensitivity there (a twin oracle started 1e-14 away): chaotic states, no absolute number
    from tests.common import make_oracle, twin_errors, assert_within_oracle_sensitivity
    kw = dict(has_object=True, controller_type="IK", reward_type="dense", seed=0, max_episode_steps=10 ** 9)
    envs, ora = make_pair(n, **kw)
    twin = make_oracle(n, **kw)
    envs.reset(seed=0); ora.reset(seed=0); twin.reset(seed=0)
    ora.set_state(**ost)
    envs.set_state(qpos=sel["qpos"], qvel=sel["qvel"], ctrl=sel["ctrl"], warm=sel["warm"], qpos_lag=sel["qpos_lag"], goal=sel["goal"],
                   elapsed=torch.zeros(n, dtype=torch.int32), episode=sel["episode"])
    state = ora.get_state()
    a = np.random.default_rng(2).uniform(-0.3, 0.3, (n, 7)).astype(np.float32)
    e, flags_equal, o = step_errors(envs, ora, a)
    te = twin_errors(twin, state, a, o, np.random.default_rng(5))
    assert_within_oracle_sensitivity([e[isarm]], [te[isarm]], "[PickAndPlace IK env-step, environments with an arm-mesh contact]")
    assert_within_oracle_sensitivity([e[~isarm]], [te[~isarm]], "[PickAndPlace IK env-step, environments without]")
    envs.close()


def _finger_mesh_poses(count=128, seed=2, meshes=("right_finger_link", "left_finger_link"), table=None):
    """Gripper poses around the cube (the scripted-grasp states, perturbed) in which the polytope of one of `meshes` touches the
    cube (the oracle's contact list names the geoms); shallow contacts only (a deep one is a violent state).  `table`: another model
    table than the built-in one (the cube of the grasp states moved to its rest height there)."""
    from tests.common import load_json
    from oracle import pyoracle as po
    from mycobotgym_amd.scenarios import grasp_state
    builtin = load_json("mycobot280")
    tab = table if table is not None else builtin
    scope = tab["geom_name"].index("object0")
    d1 = po.OracleData(po.OracleModel(tab, enable_contact=True, scope_geom=scope))
    geoms = {g for g in range(tab["ngeom"]) if tab["geom_type"][g] == 7 and tab["geom_mesh"][g] in meshes}
    q0 = np.asarray(grasp_state(64, seed=0)["qpos"]); q0 = q0.T if q0.shape[0] == 19 else q0
    if table is not None:
        q0 = q0.copy(); q0[:, 14] += tab["qpos0"][14] - builtin["qpos0"][14]
    rng = np.random.default_rng(seed)
    poses = []
    while len(poses) < count:
        q = q0[rng.integers(len(q0))].copy()
        q[:6] += rng.normal(0, 0.04, 6); q[6] = q[8] = np.clip(q[6] + rng.normal(0, 0.1), 0, 0.7)
        d1.set_state(qpos=q, qvel=np.zeros(18)); d1.forward()
        n1 = int(d1.get("ncon", (1,), np.int32)[0]); raw = d1.get("contact", (64, 28))
        hit = any(int(raw[c, 26:28].copy().view(np.int32)[1]) in geoms and int(raw[c, 26:28].copy().view(np.int32)[2]) == scope for c in range(n1))
        if hit and raw[:n1, 0].min() > -3e-3: poses.append(q)
    return np.array(poses)


def _link_cube_poses(count=128, seed=6, meshes=("link2", "link3", "link4", "link5", "link6", "flange"), table=None):
    """Random arm poses with the cube put (in the air or on the table) where it just touches one of the arm's links: the pairs an arm
    link sweeping the cube off the table goes through.  Shallow contacts only.  `table`: another model table than the built-in one."""
    from tests.common import load_json
    from oracle import pyoracle as po
    tab = table if table is not None else load_json("mycobot280")
    zmin = 0.215 if table is None else tab["qpos0"][14] + 0.005              # the cube clear of the table top
    scope = tab["geom_name"].index("object0")
    d1 = po.OracleData(po.OracleModel(tab, enable_contact=True, scope_geom=scope))
    geoms = [g for g in range(tab["ngeom"]) if tab["geom_type"][g] == 7 and tab["geom_mesh"][g] in meshes]
    gset = set(geoms)
    rng = np.random.default_rng(seed)
    poses = []
    while len(poses) < count:
        q = np.array(tab["qpos0"], float)
        q[:6] = rng.uniform(-1.5, 1.5, 6); q[6] = q[8] = rng.uniform(0, 0.7)
        d1.set_state(qpos=q, qvel=np.zeros(18)); d1.forward()
        if int(d1.get("ncon", (1,), np.int32)[0]) > 4: continue             # the arm itself must be clear of the table
        g = geoms[rng.integers(len(geoms))]
        gx = d1.get("geom_xpos", (48, 3))[g]; gR = d1.get("geom_xmat", (48, 9))[g].reshape(3, 3)
        ctr = gx + gR @ rng.uniform(-0.03, 0.06, 3)
        dirn = rng.normal(size=3); dirn /= np.linalg.norm(dirn)
        for r in np.linspace(0.09, 0.0, 46):                                    # walk the cube in until it touches
            q[12:15] = ctr + r * dirn
            quat = rng.normal(size=4); q[15:19] = quat / np.linalg.norm(quat)
            if q[14] < zmin: break
            d1.set_state(qpos=q, qvel=np.zeros(18)); d1.forward()
            n1 = int(d1.get("ncon", (1,), np.int32)[0])
            if n1 == 0: continue
            raw = d1.get("contact", (64, 28))
            ids = [raw[c, 26:28].copy().view(np.int32) for c in range(n1)]
            if all(int(i[1]) in gset and int(i[2]) == scope for i in ids) and raw[:n1, 0].min() > -2e-3: poses.append(q.copy())
            break
    return np.array(poses)


def test_substeps_arm_link_meshes_on_the_cube(torch_cuda):
    """the arm's links (2-6, flange) against the cube -- an arm link that sweeps the cube off the table no longer
    passes through it.  The cube is put where it just touches a link; teacher-forced per sub-step."""
    poses = _link_cube_poses()
    def prepare(ora):
        s = ora.get_state()
        s["qpos"][:] = poses; s["qpos_lag"] = s["qpos"].copy()
        s["ctrl"][:, :6] = poses[:, :6]; s["ctrl"][:, 6] = poses[:, 6] / 0.7
        ora.set_state(**s)
    worst, ncon = _substep_run(torch_cuda, 128, 100, prepare=prepare, hold_pose=True)
    print(f"\narm-link meshes on the cube, 100 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) >= 2
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_gear_and_hinge_link_meshes_on_the_cube(torch_cuda):
    """the gripper's gear and hinge links (mycobot280_main.xml:176-184, 203-211, 229-247) against the cube: rows in
    the arm's six dofs and the link's own joint (the hinge joints are dofs 10 and 11 of the robot)."""
    poses = _finger_mesh_poses(count=128, seed=8, meshes=("right_gear_link", "left_gear_link", "right_hinge_link", "left_hinge_link"))
    def prepare(ora):
        s = ora.get_state()
        s["qpos"][:] = poses; s["qpos_lag"] = s["qpos"].copy()
        s["ctrl"][:, :6] = poses[:, :6]; s["ctrl"][:, 6] = poses[:, 6] / 0.7
        ora.set_state(**s)
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=prepare, hold_pose=True)
    print(f"\ngear / hinge link meshes on the cube, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) >= 2
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_gripper_meshes_on_the_table_and_the_ground(torch_cuda):
    """the finger, gear and hinge links against the table / the ground (only the pads did in round 3)."""
    poses = _contact_poses("gripper_mesh", seed=3)
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=_pose_prepare(poses), hold_pose=True)
    print(f"\ngripper meshes on the table / ground, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) > 4
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_finger_link_meshes_on_the_cube(torch_cuda):
    """the two finger-link meshes (their full hulls, exact separating-axis test, one contact each) against
    the cube -- contacts between the same two bodies as the pad-cube contacts, with the mesh-cube pair's own parameters."""
    poses = _finger_mesh_poses()
    def prepare(ora):
        s = ora.get_state()
        s["qpos"][:] = poses; s["qpos_lag"] = s["qpos"].copy()
        s["ctrl"][:, :6] = poses[:, :6]; s["ctrl"][:, 6] = poses[:, 6] / 0.7
        ora.set_state(**s)
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=prepare, hold_pose=True)
    print(f"\nfinger-link meshes on the cube, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) >= 2
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_substeps_gripper_base_mesh_on_the_cube(torch_cuda):
    """the gripper base's mesh (mycobot280_main.xml:171-175; it rides on link6) against the cube -- a contact between
    the cube and the ARM, which the cooperative solve takes as one more generic row (round 2's class-wise solve could not afford it)."""
    poses = _finger_mesh_poses(count=128, seed=4, meshes=("gripper_base",))
    def prepare(ora):
        s = ora.get_state()
        s["qpos"][:] = poses; s["qpos_lag"] = s["qpos"].copy()
        s["ctrl"][:, :6] = poses[:, :6]; s["ctrl"][:, 6] = poses[:, 6] / 0.7
        ora.set_state(**s)
    worst, ncon = _substep_run(torch_cuda, 128, 200, prepare=prepare, hold_pose=True)
    print(f"\ngripper-base mesh on the cube, 200 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert max(ncon) >= 2
    assert worst["obs"] < 1e-10 and worst["qpos"] < 1e-10 and worst["qvel"] < 1e-6


def test_cube_edges_parallel_to_the_table_edges(torch_cuda):
    """Regression (round 2): a cube rocking on the table by 3e-4 rad about y has its y edges parallel to the table's.  With
    |A_i x B_j| taken as sqrt(1 - C^2), rounding (C = 1 - 1e-16) made a 1e-8 `length`, and the axis built from that noise beat the
    face axes: the four table contacts were replaced by one contact without a normal and the cube fell freely for a sub-step.
    The state is the one the fault was found in (tests/golden/cube_parallel_edge_state.npz: inputs + the oracle's output)."""
    import os
    from tests.common import make_pair, sync_oracle_to, step_errors
    z = np.load(os.path.join(os.path.dirname(__file__), "golden", "cube_parallel_edge_state.npz"))
    n = 64
    envs, ora = make_pair(n, has_object=True, controller_type="joint", reward_type="dense", seed=5, frame_skip=1, max_episode_steps=10 ** 9)
    envs.reset(seed=5); ora.reset(seed=5)
    s = ora.get_state()
    for k in s: s[k][:] = z["pre_" + k]
    ora.set_state(**s)
    sync_oracle_to(envs, ora)
    a = np.tile(z["action"], (n, 1)).astype(np.float32)
    step_errors(envs, ora, a)
    st, so = envs.get_state(), ora.get_state()
    from tests.common import load_json
    tab = load_json("mycobot280"); gcube = tab["geom_name"].index("object0")
    d0 = ora.data(0); raw = d0.get("contact", (64, 28)); nc = int(d0.get("ncon", (1,), np.int32)[0])
    pairs = [tuple(int(x) for x in raw[c, 26:28].copy().view(np.int32)[1:3]) for c in range(nc)]
    assert sum(1 for g1, g2 in pairs if g1 == 1 and g2 == gcube) == 4             # the cube keeps its four table contacts (+ 4 pad-table, + the finger / gear links' since round 4)
    assert np.abs(so["qpos"][0] - z["post_qpos"]).max() < 1e-12                   # the oracle still gives the recorded answer (re-recorded in round 4: mesh contacts joined the state)
    assert np.abs(st["qpos"].cpu().numpy().T - so["qpos"]).max() < 1e-12
    assert np.abs(st["qvel"].cpu().numpy().T - so["qvel"]).max() < 1e-9
    envs.close()


def test_substeps_cube_tumbling_onto_table(torch_cuda):
    """Cubes dropped from 3 cm with random attitude and spin: vertex, edge and face contacts, make/break events."""
    def prepare(ora):
        s = ora.get_state()
        rng = np.random.default_rng(11)
        n = s["qpos"].shape[0]
        q = rng.normal(size=(n, 4)); q /= np.linalg.norm(q, axis=1, keepdims=True)
        s["qpos"][:, 14] = 0.24; s["qpos"][:, 15:19] = q
        s["qvel"][:, 12:15] = rng.normal(size=(n, 3)) * 0.1; s["qvel"][:, 15:18] = rng.normal(size=(n, 3)) * 5.0
        s["qpos_lag"] = s["qpos"].copy()
        ora.set_state(**s)
    worst, ncon = _substep_run(torch_cuda, 128, 500, prepare=prepare)
    print(f"\ntumbling cube, 500 sub-steps x 128 envs: {worst}, contact counts seen {sorted(ncon)}")
    assert len(ncon) >= 3
    assert worst["obs"] < 1e-12 and worst["qpos"] < 2e-12 and worst["qvel"] < 1e-9       # measured 5.5e-15, 2.0e-14, 1.0e-11


def test_env_steps_with_object(torch_cuda):
    from tests.common import make_pair, make_oracle, sync_oracle_to, step_errors, twin_errors, assert_within_oracle_sensitivity
    n = 128
    for controller in ("joint", "IK"):
        envs, ora = make_pair(n, has_object=True, controller_type=controller, reward_type="sparse", seed=2)
        twin = make_oracle(n, has_object=True, controller_type=controller, reward_type="sparse", seed=2)
        envs.reset(seed=2); ora.reset(seed=2); twin.reset(seed=2)
        rng = np.random.default_rng(8); prng = np.random.default_rng(1)
        errs, terrs = [], []
        for t in range(55):
            sync_oracle_to(envs, ora)
            state = ora.get_state()
            a = rng.uniform(-1, 1, (n, 7)).astype(np.float32)
            e, flags_equal, o = step_errors(envs, ora, a)
            assert flags_equal
            errs.append(e)
            if controller == "IK": terrs.append(twin_errors(twin, state, a, o, prng))
        if controller == "IK": assert_within_oracle_sensitivity(errs, terrs, "[pnp IK env-step]")
        errs = np.concatenate(errs)
        print(f"\n[{controller}] PickAndPlace env-steps from identical state: median {np.median(errs):.2e} p99 {np.quantile(errs, 0.99):.2e}")
        if controller == "joint": assert np.median(errs) < 1e-13 and errs.max() < 1e-8      # measured: median 9e-16, p99 2e-13
        else: assert np.median(errs) < 2e-10      # measured: median 1.7e-12; the tails (finger pads meeting the table) are bounded above
        envs.close()


def _grasp_state(ora, n):
    """Oracle state with the cube between the open finger pads at the fetch keyframe and the gripper commanded shut."""
    from tests.common import load_json
    tab = load_json("mycobot280")
    key = tab["keys"][0]
    s = ora.get_state()
    d0 = ora.data(0)
    d0.set_state(qpos=key["qpos"]); d0.forward()
    gn = tab["geom_name"]; gx = d0.get("geom_xpos", (48, 3))
    mid = 0.5 * (gx[gn.index("right_finger_layer")] + gx[gn.index("left_finger_layer")])
    rng = np.random.default_rng(7)
    q = np.tile(np.asarray(key["qpos"], dtype=float), (n, 1))
    q[:, 12:15] = mid + rng.normal(size=(n, 3)) * 0.002
    quat = np.tile([1.0, 0, 0, 0], (n, 1)) + rng.normal(size=(n, 4)) * 0.05
    q[:, 15:19] = quat / np.linalg.norm(quat, axis=1, keepdims=True)
    s["qpos"] = q; s["qpos_lag"] = q.copy(); s["qvel"][:] = 0
    s["ctrl"] = np.tile(np.asarray(key["ctrl"], dtype=float), (n, 1)); s["ctrl"][:, 6] = 1.0
    ora.set_state(**s)


def test_substeps_through_a_grasp(torch_cuda):
    """Pads close on the cube: pad-cube contacts couple robot and cube (coupled Newton, Schur complement)."""
    from tests.common import make_pair, sync_oracle_to, step_errors
    n = 64
    kw = dict(has_object=True, controller_type="joint", reward_type="dense", seed=5, frame_skip=1, max_episode_steps=10 ** 9)
    envs, ora = make_pair(n, **kw)
    envs.reset(seed=5); ora.reset(seed=5)
    _grasp_state(ora, n)
    a = np.tile(np.concatenate([ora.get_state()["ctrl"][0, :6], [1.0]]).astype(np.float32), (n, 1))
    a = np.clip(a, -1, 1)
    worst = dict(obs=0.0, qpos=0.0, qvel=0.0); ncon_seen = set(); iters = set()
    for t in range(300):
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal
        st, so = envs.get_state(), ora.get_state()
        worst["obs"] = max(worst["obs"], e.max())
        worst["qpos"] = max(worst["qpos"], np.abs(st["qpos"].cpu().numpy().T - so["qpos"]).max())
        worst["qvel"] = max(worst["qvel"], np.abs(st["qvel"].cpu().numpy().T - so["qvel"]).max())
        for i in range(0, n, 4):
            ncon_seen.add(int(ora.data(i).get("ncon", (1,), np.int32)[0])); iters.add(int(ora.data(i).get("solver_iter", (1,), np.int32)[0]))
    print(f"\ngrasp, 300 sub-steps x {n} envs: {worst}; contact counts {sorted(ncon_seen)}; oracle Newton iterations {sorted(iters)}")
    assert max(ncon_seen) >= 4 and max(iters) >= 2
    assert worst["obs"] < 2e-12 and worst["qpos"] < 2e-12 and worst["qvel"] < 1e-9       # measured 1.6e-14, 1.3e-14, 8.0e-12
    envs.close()


def test_reward_shaping_through_a_grasp(torch_cuda):
    """stage_rewards: reach / grasp / lift stages against the oracle while the pads close on the cube."""
    from tests.common import make_pair, sync_oracle_to, step_errors
    n = 64
    kw = dict(has_object=True, controller_type="joint", reward_type="reward_shaping", seed=5, frame_skip=4, max_episode_steps=10 ** 9)
    envs, ora = make_pair(n, **kw)
    envs.reset(seed=5); ora.reset(seed=5)
    _grasp_state(ora, n)
    a = np.clip(np.tile(np.concatenate([ora.get_state()["ctrl"][0, :6], [1.0]]).astype(np.float32), (n, 1)), -1, 1)
    rewards = []
    for t in range(60):
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, a)
        assert flags_equal and e.max() < 1e-9
        rewards.append(o["reward"].copy())
    rewards = np.concatenate(rewards)
    print(f"\nshaped rewards seen: min {rewards.min():.2f} max {rewards.max():.2f}; grasp/lift stage fraction {(rewards >= 50).mean():.2f}")
    assert rewards.max() >= 50 and rewards.min() < 50            # both the reach stage and the grasp / lift stages occurred
    envs.close()


def test_domain_randomisation_matches_oracle(torch_cuda):
    """Per-reset cube mass / friction scales (build-defined R3): same Philox draws, same physics as the oracle."""
    from tests.common import make_pair, sync_oracle_to, step_errors
    n = 128
    dr = {"mass": (0.5, 2.0), "friction": (0.5, 1.5)}
    envs, ora = make_pair(n, has_object=True, controller_type="joint", reward_type="dense", seed=9, domain_randomization=dr)
    envs.reset(seed=9); ora.reset(seed=9)
    s = envs.get_state()["dr_scale"].cpu().numpy()
    assert s[0].min() >= 0.5 and s[0].max() <= 2.0 and s[1].min() >= 0.5 and s[1].max() <= 1.5 and s[0].std() > 0.1
    rng = np.random.default_rng(1)
    for t in range(55):                                  # crosses the TimeLimit reset: new scales are drawn on both sides
        sync_oracle_to(envs, ora)
        e, flags_equal, o = step_errors(envs, ora, rng.uniform(-1, 1, (n, 7)).astype(np.float32))
        assert flags_equal and np.median(e) < 1e-13 and e.max() < 1e-8
    s2 = envs.get_state()["dr_scale"].cpu().numpy()
    assert not np.array_equal(s, s2)
    envs.close()
