"""Shared helpers of the parity tests: build the HIP env and the CPU oracle with one configuration."""
from __future__ import annotations

import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ASSETS = os.path.join(ROOT, "mycobotgym_amd", "assets")


@pytest.fixture(scope="module")
def torch_cuda(built):
    """torch, on a machine with a GPU.  A GPU test file takes it with `from tests.common import torch_cuda  # noqa: F401`: pytest finds a
    fixture imported into the module; `built` is conftest.py's."""
    import torch
    assert torch.cuda.is_available(), "GPU tests need a visible MI355X"
    return torch


def table_name(has_object=False, mesh_inertia="legacy", mocap=False):
    return ("mycobot280" + ("_mocap" if mocap else "") + ("" if has_object else "_reach")
            + ("_exactmesh" if mesh_inertia == "exact" else ""))


def load_json(name):
    with open(os.path.join(ASSETS, name + ".json")) as f:
        return json.load(f)


def soften_gains(tab, scale=0.1):
    """A contractive variant of the model: actuator velocity gains scaled so that h*kv/M < 1 (the reference's own
    gains make explicit Euler an unstable map, see DESIGN.md 'Parity and chaos').  Test-only."""
    tab = json.loads(json.dumps(tab))
    for a in tab["actuators"]:
        a["biasprm"][2] *= scale
    return tab


def perturbed_table(name, seed=0):
    """A deterministic perturbation of built-in table `name` (mycobot280, mycobot280_reach, mycobot280_mocap) that moves numbers every kernel
    family reads: a 5 mm flange spacer (polytopes of the flange and the gripper base, the gripper's bodies, the EEF site, the mocap weld
    point), arm links +-1-2 mm, mass x U(0.9, 1.1) with the inertia alike and the CoM +-1 mm, damping / armature x U(0.8, 1.2), arm joint
    ranges 5 % narrower, servo gains x U(0.95, 1.05), a cube of half-size 12 mm on a table 4 mm higher, pads 0.5 mm larger, cube friction
    x 1.2, mesh friction x 0.9, the EEF site +-1 mm.  Every change keeps specialize's structural asserts.  Test-only."""
    tab = json.loads(json.dumps(load_json(name)))
    rng = np.random.default_rng(seed)
    bi, gname = tab["body_name"].index, tab["geom_name"]
    sign = lambda: float(rng.choice([-1.0, 1.0]))
    tab["body_pos"][bi("flange")][0] += 0.005
    for b in ("link2", "link3", "link4", "link5", "link6"):
        for k in range(3):
            tab["body_pos"][bi(b)][k] += sign() * rng.uniform(0.001, 0.002)
    for b in range(tab["nbody"]):
        if tab["body_mass"][b] <= 0:
            continue
        f = rng.uniform(0.9, 1.1)
        tab["body_mass"][b] *= f
        tab["body_inertia"][b] = [f * x for x in tab["body_inertia"][b]]
        if tab["body_name"][b] != "object0":                       # the cube stays centred (and axis-aligned: body_iquat untouched)
            tab["body_ipos"][b] = [x + rng.uniform(-0.001, 0.001) for x in tab["body_ipos"][b]]
    tab["dof_damping"] = [x * rng.uniform(0.8, 1.2) for x in tab["dof_damping"]]
    tab["dof_armature"] = [x * rng.uniform(0.8, 1.2) for x in tab["dof_armature"]]
    for j in range(6):                                             # the arm's hinges: 5 % narrower about the centre
        lo, hi = tab["jnt_range"][j]
        c, h = 0.5 * (lo + hi), 0.5 * (hi - lo)
        tab["jnt_range"][j] = [c - 0.95 * h, c + 0.95 * h]
    for a in tab["actuators"]:                                     # position servos: gainprm[0] = kp, biasprm = (0, -kp, -kv)
        fp, fv = rng.uniform(0.95, 1.05), rng.uniform(0.95, 1.05)
        a["gainprm"][0] *= fp; a["biasprm"][1] *= fp; a["biasprm"][2] *= fv
    if "object0" in gname:
        gc = gname.index("object0")
        old = tab["geom_size"][gc][2]
        tab["geom_size"][gc] = [0.012, 0.012, 0.012]
        tab["geom_friction"][gc] = [1.2 * x for x in tab["geom_friction"][gc]]
        tab["body_pos"][bi("table")][2] += 0.004
        dz = 0.004 + (0.012 - old)                                  # the cube still rests on the table top
        tab["body_pos"][bi("object0")][2] += dz
        qadr = tab["jnt_qposadr"][tab["jnt_name"].index("object0:joint")]
        tab["qpos0"][qadr + 2] += dz
    for g in ("right_finger_layer", "left_finger_layer"):
        if g in gname:
            tab["geom_size"][gname.index(g)] = [x + 0.0005 for x in tab["geom_size"][gname.index(g)]]
    for g in range(tab["ngeom"]):
        if tab["geom_type"][g] == 7:
            tab["geom_friction"][g] = [0.9 * x for x in tab["geom_friction"][g]]
    s = tab["site_name"].index("EEF")
    tab["site_pos"][s] = [x + sign() * 0.001 for x in tab["site_pos"][s]]
    return tab


def make_oracle(n, has_object=False, controller_type="joint", fetch_env=False, reward_type="dense", seed=0,
                env_id_offset=0, mesh_inertia="legacy", frame_skip=20, control_steps=5, max_episode_steps=50,
                target_in_the_air=True, distance_threshold=0.01, auto_reset=True, n_threads=None, table=None,
                domain_randomization=None, block_gripper=False, weld_rule="common", contact_rule="mujoco", initial=None):
    """`initial`: (qpos, qvel, ctrl, initial_gripper_xpos, height_offset) to use instead of vec_env.initial_state's."""
    from oracle import pyoracle as po
    from mycobotgym_amd.vec_env import initial_state
    mocap = controller_type == "mocap"
    hidden = (not has_object) and reward_type == "reward_shaping"      # Reach keeps the cube, hidden (mycobot.py:475-481)
    tab = table if table is not None else load_json(table_name(has_object or hidden, mesh_inertia, mocap))
    if hidden:
        tab = json.loads(json.dumps(tab))
        tab["geom_size"][tab["geom_name"].index("object0")] = [0.0, 0.0, 0.0]        # self.model.geom_size[object_id] = 0
    has_cube = has_object or hidden
    # the build's scoped collision set: pairs involving the cube
    model = po.OracleModel(tab, enable_contact=has_cube, scope_geom=tab["geom_name"].index("object0") if has_cube else -1)
    if weld_rule == "mujoco" or contact_rule == "keyframe":
        # study switches: rule[0] = 1 rotational weight on the weld's rows 3-5; rule[3] = 2 Rpy = 4 mu^2 R (the keyframes' rest height)
        model._set_i("rule", [1 if weld_rule == "mujoco" else 0, 0, 0, 2 if contact_rule == "keyframe" else 0, 0, 0, 0, 0])
    qpos, qvel, ctrl, igx, height = initial if initial is not None else initial_state(has_cube, fetch_env, mesh_inertia, mocap, table=table)
    ctrl = ctrl[7 - tab["nu"]:]                  # the oracle's ctrl has the model's nu entries (mocap model: the finger only)
    cfg = po.EnvConfig()
    cfg.n_envs = n; cfg.has_object = int(has_object)
    cfg.controller = {"joint": 0, "IK": 1, "mocap": 2}[controller_type]; cfg.fetch_env = int(fetch_env)
    cfg.tcp_body = tab["body_name"].index("gripper_tcp")
    if mocap:
        mb = tab["body_mocap"].index(True)
        pose = list(tab["body_pos"][mb]) + list(tab["body_quat"][mb])
        if fetch_env:
            key = (table if table is not None else load_json(table_name(True, mesh_inertia, True)))["keys"][0]
            pose = list(key["mpos"]) + list(key["mquat"])
        for k, v in enumerate(pose): cfg.init_mocap[k] = v
    cfg.reward_type = {"sparse": 0, "dense": 1, "reward_shaping": 2}[reward_type]
    cfg.frame_skip = frame_skip; cfg.control_steps = control_steps; cfg.max_episode_steps = max_episode_steps
    cfg.target_in_the_air = int(target_in_the_air); cfg.auto_reset = int(auto_reset)
    cfg.eef_site = tab["site_name"].index("EEF")
    cfg.obj_site = tab["site_name"].index("object0") if has_cube else -1
    cfg.obj_jnt = tab["jnt_name"].index("object0:joint") if has_object else -1
    cfg.grip_jnt[0] = tab["jnt_name"].index("robot0:right_gear_joint")
    cfg.grip_jnt[1] = tab["jnt_name"].index("robot0:left_gear_joint")
    cfg.block_gripper = int(block_gripper)
    cfg.finger_jnt[0] = tab["jnt_name"].index("right_finger_joint"); cfg.finger_jnt[1] = tab["jnt_name"].index("left_finger_joint")
    cfg.n_threads = n_threads or min(os.cpu_count() or 1, 16)
    cfg.pad_geom[0] = cfg.pad_geom[1] = cfg.obj_geom = -1
    if has_cube:
        cfg.pad_geom[0] = tab["geom_name"].index("right_finger_layer"); cfg.pad_geom[1] = tab["geom_name"].index("left_finger_layer")
        cfg.obj_geom = tab["geom_name"].index("object0")
    cfg.distance_threshold = distance_threshold; cfg.height_offset = height
    for k, v in enumerate(qpos): cfg.init_qpos[k] = v
    for k, v in enumerate(qvel): cfg.init_qvel[k] = v
    for k, v in enumerate(ctrl): cfg.init_ctrl[k] = v
    cfg.seed = seed; cfg.env_id_offset = env_id_offset
    if domain_randomization:
        cfg.dr_enable = 1
        cfg.dr_mass_range[0], cfg.dr_mass_range[1] = domain_randomization.get("mass", (1.0, 1.0))
        cfg.dr_friction_range[0], cfg.dr_friction_range[1] = domain_randomization.get("friction", (1.0, 1.0))
    return po.OracleEnvs(model, cfg)


def make_pair(n, device="cuda:0", table=None, **kw):
    """HIP engine + CPU oracle with one configuration.  `table`: optional modified model table for both (the engine specialises it,
    polytopes and initial state included: MyCobotVecEnv(table=...))."""
    from mycobotgym_amd import MyCobotVecEnv
    okw = dict(kw)
    envs = MyCobotVecEnv(n, device=device, has_object=kw.pop("has_object", False), table=table, **kw)
    ora = make_oracle(n, table=table, **okw)
    return envs, ora


def step_errors(envs, ora, actions):
    """Step both; per-env max abs error over observation / achieved goal / reward, whether terminated, truncated, is_success and the
    finished episodes' lengths all agree, plus the oracle outputs."""
    import torch
    obs, rew, term, trunc, info = envs.step(torch.as_tensor(actions))
    o = ora.step(actions)
    e = np.abs(obs["observation"].cpu().numpy() - o["obs"]).max(axis=1)
    e = np.maximum(e, np.abs(obs["achieved_goal"].cpu().numpy() - o["achieved"]).max(axis=1))
    e = np.maximum(e, np.abs(rew.cpu().numpy() - o["reward"]))
    # goals come from the Philox reset draws: they must agree bit for bit, also right after an auto-reset
    assert np.array_equal(obs["desired_goal"].cpu().numpy(), o["desired"]), "desired_goal differs (reset draws)"
    flags_equal = (np.array_equal(term.cpu().numpy(), o["terminated"].astype(bool))
                   and np.array_equal(trunc.cpu().numpy(), o["truncated"].astype(bool)))
    # is_success, and the finished episodes' length (Monitor's "l"), are integers: they agree exactly whenever the flags do
    done = o["terminated"].astype(bool) | o["truncated"].astype(bool)
    flags_equal = (flags_equal and np.array_equal(info["is_success"].cpu().numpy(), o["is_success"].astype(bool))
                   and np.array_equal(info["episode"]["l"].cpu().numpy()[done], o["ep_length"][done]))
    return e, flags_equal, o


def sync_state(envs, s):
    """Copy a state of the oracle (its get_state(), live or recorded; not modified) into the HIP engine."""
    ctrl = s["ctrl"]
    if ctrl.shape[1] < 7:           # mocap model: one actuator (the fingers) = the engine's ctrl slot 6
        ctrl = np.concatenate([np.zeros((ctrl.shape[0], 7 - ctrl.shape[1])), ctrl], axis=1)
    envs.set_state(qpos=s["qpos"].T.copy(), qvel=s["qvel"].T.copy(), ctrl=ctrl.T.copy(), warm=s["warm"].T.copy(),
                   qpos_lag=s["qpos_lag"].T.copy(), goal=s["goal"].T.copy(), elapsed=s["elapsed"].copy(), episode=s["episode"].copy())


def sync_oracle_to(envs, ora):
    """Copy the oracle's state into the HIP engine (both then continue from identical state)."""
    sync_state(envs, ora.get_state())


def compare_step(envs, ora, actions, keys=("obs", "achieved", "desired", "reward")):
    """Step both with the same float32 actions; return the max abs error over obs / goals / reward and assert
    that the integer outputs agree exactly."""
    import torch
    obs, rew, term, trunc, info = envs.step(torch.as_tensor(actions))
    o = ora.step(actions)
    got = {"obs": obs["observation"], "achieved": obs["achieved_goal"], "desired": obs["desired_goal"], "reward": rew}
    err = 0.0
    for k in keys:
        err = max(err, float(np.abs(got[k].cpu().numpy() - o[k]).max()))
    assert np.array_equal(term.cpu().numpy(), o["terminated"].astype(bool))
    assert np.array_equal(trunc.cpu().numpy(), o["truncated"].astype(bool))
    assert np.array_equal(info["is_success"].cpu().numpy(), o["is_success"].astype(bool))
    done = o["terminated"].astype(bool) | o["truncated"].astype(bool)
    if done.any():
        f = info["final_observation"]
        err = max(err, float(np.abs(f["observation"].cpu().numpy()[done] - o["final_obs"][done]).max()))
        assert np.array_equal(info["episode"]["l"].cpu().numpy()[done], o["ep_length"][done])
    return err


def twin_errors(twin, state, actions, o_ref, prng, eps=1e-14, cols=None):
    """The oracle's own sensitivity: a second oracle steps from `state` (the reference's state before its step) with qpos
    perturbed by +-eps; returns its per-env max abs observation difference from the reference's outputs `o_ref`.

    `cols` (an index or slice of qpos columns, e.g. slice(0, 12) for the robot's joints): perturb only these.  A cube at its reset height
    sits at distance ~0 from the table top, so +-1e-14 on its z switches its four table contacts on or off and the twin differs by
    g h^2 = 3.9e-5 after ONE sub-step: a property of the resting cube, not of the controller under test, which would inflate any bound taken
    relative to the twin.  The default perturbs every column, as before."""
    s = dict(state)
    p = eps * np.sign(prng.normal(size=state["qpos"].shape))
    if cols is not None:
        keep = np.zeros(state["qpos"].shape[1], bool); keep[cols] = True
        p[:, ~keep] = 0.0
    s["qpos"] = state["qpos"] + p
    twin.set_state(**s)
    ot = twin.step(actions)
    return np.abs(ot["obs"] - o_ref["obs"]).max(axis=1)


def assert_within_oracle_sensitivity(e_hip, e_twin, what="", factor=10.0):
    """Chaotic env-steps (100 sub-steps of the stiff servos, contact make / break): HIP-vs-oracle error quantiles must not exceed
    `factor` x the oracle-vs-perturbed-oracle quantiles of the same states."""
    e_hip, e_twin = np.concatenate(e_hip), np.concatenate(e_twin)
    q = lambda e: np.array([np.median(e), np.quantile(e, 0.9), np.quantile(e, 0.99)])
    qh, qt = q(e_hip), q(e_twin)
    print(f"\n{what} quantiles (median p90 p99 | max): hip-vs-oracle " + " ".join(f"{x:.2e}" for x in qh) + f" | {e_hip.max():.2e};  "
          "oracle-vs-oracle+1e-14 " + " ".join(f"{x:.2e}" for x in qt) + f" | {e_twin.max():.2e}")
    assert np.all(qh <= factor * qt + 1e-13), (what, qh, qt)


def bits(x):
    """The array's own bits as unsigned integers of its item size: what a bit-for-bit comparison compares (nan payloads and -0 included)."""
    x = np.ascontiguousarray(x)
    return x.view({1: np.uint8, 4: np.uint32, 8: np.uint64}[x.dtype.itemsize])
