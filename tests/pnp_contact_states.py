"""Contact states of PickAndPlace for the IK and mocap controllers, made by the CPU oracle alone (no GPU), once per process.

Two kinds of start state, the same for the CPU conditions (tests/test_pnp_contact_states_cpu.py) and the GPU comparisons
(tests/test_gpu_pnp_controllers_on_contacts.py):

* pose families: the rejection-sampled poses of tests/test_gpu_pickandplace.py (arm meshes and gripper meshes on the table / the ground,
  finger-link meshes and arm links on the cube), searched on the controller's own model table (the mocap model has no arm servos and a
  weld), 72 of each: two workgroups of 32 environments and a ragged one of 8.  Velocities zero, lagged pose = pose.
* random-policy states: what 45 env-steps of a uniform random policy reach under the controller itself, picked by what the oracle's contact
  list holds: first the environments whose list the cap of 16 entries cut, then those with a mesh geom in the list, then some without.

Nothing here is mutated after it is built (the arrays are read-only): the tests copy what they change."""
from __future__ import annotations

import functools

import numpy as np

from tests.common import load_json, make_oracle

FAMILIES = ("mesh", "gripper_mesh", "finger_cube", "link_cube")
CUBE_FAMILIES = ("finger_cube", "link_cube")          # the cube is part of the pose (all 19 qpos columns); the others leave it at rest
N_POSES = 72                                          # 32 + 32 + 8: two full workgroups and a ragged one
CONTROLLERS = {"IK": ("IK", False), "fetch-IK": ("IK", True), "mocap": ("mocap", False), "fetch-mocap": ("mocap", True)}
N_COLLECT = {"IK": 256, "mocap": 512}
MESH = 7                                              # geom_type of a mesh geom


def model_table(controller_type):
    return load_json("mycobot280_mocap" if controller_type == "mocap" else "mycobot280")


def engine_kw(name, frame_skip=1, control_steps=1, seed=3):
    """Keyword arguments of tests.common.make_pair / make_oracle for controller `name` (a key of CONTROLLERS)."""
    controller, fetch = CONTROLLERS[name]
    return dict(has_object=True, controller_type=controller, fetch_env=fetch, reward_type="dense", seed=seed, frame_skip=frame_skip,
                control_steps=control_steps, max_episode_steps=10 ** 9)


def _frozen(a):
    a = np.ascontiguousarray(a)
    a.flags.writeable = False
    return a


@functools.lru_cache(maxsize=None)
def pose_family(family, mocap=False):
    """N_POSES qpos rows [N_POSES, 19] of pose family `family`, searched on the mocap model's table if `mocap`."""
    from tests.test_gpu_pickandplace import _contact_poses, _finger_mesh_poses, _link_cube_poses
    kw = dict(table=model_table("mocap")) if mocap else {}
    if family == "mesh": poses = _contact_poses("mesh", N_POSES, seed=1, **kw)
    elif family == "gripper_mesh": poses = _contact_poses("gripper_mesh", N_POSES, seed=3, **kw)
    elif family == "finger_cube": poses = _finger_mesh_poses(N_POSES, **kw)
    elif family == "link_cube": poses = _link_cube_poses(N_POSES, **kw)
    else: raise KeyError(family)
    assert poses.shape == (N_POSES, 19)
    return _frozen(poses)


def put_poses(ora, family, poses):
    """Install a pose family in oracle `ora` (after its reset): the robot's 12 joints (and the cube, for the cube families), zero velocity,
    lagged pose = pose, servo targets = the pose.  Works on the mocap model too, whose ctrl has the finger's column only."""
    s = ora.get_state()
    if family in CUBE_FAMILIES: s["qpos"][:] = poses
    else: s["qpos"][:, :12] = poses[:, :12]
    s["qpos_lag"] = s["qpos"].copy()
    s["qvel"][:] = 0
    if s["ctrl"].shape[1] == 7: s["ctrl"][:, :6] = poses[:, :6]
    s["ctrl"][:, -1] = poses[:, 6] / 0.7
    ora.set_state(**s)


def contact_census(ora):
    """Per environment of `ora`, from the contact list of its last collision pass: (a mesh geom is in the list, the cap cut the list,
    number of entries)."""
    tab = ora.model.table
    mesh = np.array([t == MESH for t in tab["geom_type"]])
    has = np.zeros(ora.n, bool); cut = np.zeros(ora.n, bool); ncon = np.zeros(ora.n, np.int32)
    for i in range(ora.n):
        d = ora.data(i)
        ncon[i] = int(d.get("ncon", (1,), np.int32)[0])
        raw = d.get("contact", (64, 28))
        for c in range(ncon[i]):
            ids = raw[c, 26:28].copy().view(np.int32)
            if mesh[int(ids[1])] or mesh[int(ids[2])]: has[i] = True
        cut[i] = int(d.get("ndrop", (1,), np.int32)[0]) > 0
    return has, cut, ncon


def list_sizes(ora):
    """Entries of every environment's contact list at `ora`'s last collision pass."""
    return np.array([int(ora.data(i).get("ncon", (1,), np.int32)[0]) for i in range(ora.n)])


def oracle_ndrop_at(controller_type, qpos):
    """Contacts the cap cuts at positions `qpos` [n, 19] themselves (an OracleEnvs' own lists are those of the lagged pose)."""
    from oracle import pyoracle as po
    tab = model_table(controller_type)
    d = po.OracleData(po.OracleModel(tab, enable_contact=True, scope_geom=tab["geom_name"].index("object0")))
    out = np.zeros(len(qpos), np.int64)
    for i, q in enumerate(qpos):
        d.set_state(qpos=q, qvel=np.zeros(tab["nv"])); d.forward()
        out[i] = int(d.get("ndrop", (1,), np.int32)[0])
    return out


@functools.lru_cache(maxsize=None)
def random_policy_states(name):
    """States a uniform random policy reaches in 45 env-steps under controller `name`, collected by the oracle.  Returns a dict: `state`
    (the oracle's state arrays of the picked environments, elapsed = 0), `mesh` (picked environments with a mesh contact or a cut list),
    `cut` (picked environments whose list the cap cut) and `census` (counts over ALL collected environments)."""
    controller, fetch = CONTROLLERS[name]
    n = N_COLLECT[controller]
    ora = make_oracle(n, has_object=True, controller_type=controller, fetch_env=fetch, reward_type="dense", seed=3)
    ora.reset(seed=3)
    rng = np.random.default_rng(99)
    for t in range(45):
        a = rng.uniform(-1, 1, (n, ora.act_dim)).astype(np.float32)
        if controller == "mocap" and ora.act_dim == 8:
            a[:, 3:7] = (np.array([0.70710678, 0, 0, 0.70710678]) + 0.3 * rng.normal(size=(n, 4))).astype(np.float32)
        ora.step(a)
    has, cut, ncon = contact_census(ora)
    st = ora.get_state()
    first_cut = np.nonzero(cut)[0][:16]
    rest = np.setdiff1d(np.nonzero(has | cut)[0], first_cut)[: 48 - len(first_cut)]
    without = np.nonzero(~(has | cut))[0][:24]
    pick = np.concatenate([first_cut, rest, without])
    state = {k: _frozen(v[pick]) for k, v in st.items()}
    state["elapsed"] = _frozen(np.zeros(len(pick), np.int32))
    census = dict(n=n, mesh=int(has.sum()), cut=int(cut.sum()), ncon_max=int(ncon.max()),
                  finite=bool(np.isfinite(st["qpos"]).all() and np.isfinite(st["qvel"]).all()), qvel_max=float(np.abs(st["qvel"]).max()))
    return dict(state=state, mesh=_frozen((has | cut)[pick]), cut=_frozen(cut[pick]), census=census)


def put_state(ora, state):
    ora.set_state(**{k: v.copy() for k, v in state.items()})


def draw_actions(rng, ora):
    """Moderate actions for the comparisons: U(-0.3, 0.3); the 8-dim mocap action's quaternion is gripper_tcp's current one from the oracle
    (the orientation is held: a random far orientation is a violent weld)."""
    a = rng.uniform(-0.3, 0.3, (ora.n, ora.act_dim)).astype(np.float32)
    if ora.act_dim == 8:
        tab = ora.model.table
        tcp = tab["body_name"].index("gripper_tcp")
        for i in range(ora.n):
            a[i, 3:7] = ora.data(i).get("xquat", (tab["nbody"], 4))[tcp]
    return a
