"""``MyCobotVecEnv`` -- N MyCobot environments stepped in lockstep on one MI355X.

Host-side mirror of the reference's ``MyCobotEnv`` (/root/reference/mycobotgym/envs/mycobot.py:27-514):
same constructor keywords, observation Dict {observation, achieved_goal, desired_goal} (float64), Box(-1,1)
float32 actions, ``step -> (obs, reward, terminated, truncated, info)``, ``compute_reward`` on batched goals,
wrapped in the registration's TimeLimit(50) (mycobotgym/__init__.py:34) and batched with Gymnasium
``VectorEnv`` semantics (auto-reset; ``info["final_observation"]`` / ``info["_final_observation"]``).

Everything numeric happens in the HIP library behind ``include/mcg.h``; this file only owns device buffers
(PyTorch tensors) and hands their addresses across the C ABI.  No CPU fallback: without the library or without
a GPU the constructor raises.
"""
from __future__ import annotations

import ctypes as C
import json
import os
from typing import Optional

import numpy as np
import torch

from . import _abi, _devbuf
from .registry import MAX_EPISODE_STEPS, spec as _spec
from .spaces import Box, Dict, batch_box

_ASSETS = os.path.join(os.path.dirname(os.path.abspath(__file__)), "assets")
_CONTROLLERS = {"joint": _abi.CTRL_JOINT, "IK": _abi.CTRL_IK, "mocap": _abi.CTRL_MOCAP}
_REWARDS = {"sparse": _abi.REWARD_SPARSE, "dense": _abi.REWARD_DENSE, "reward_shaping": _abi.REWARD_SHAPING}


def load_table(has_object: bool, mesh_inertia: str = "legacy", mocap: bool = False) -> dict:
    """Compiled model table: mycobot280.xml (joint / IK) or mycobot280_mocap.xml (mocap controller), mycobot.py:47-58."""
    name = ("mycobot280" + ("_mocap" if mocap else "") + ("" if has_object else "_reach")
            + ("_exactmesh" if mesh_inertia == "exact" else ""))
    from .model.mjcf import load_model
    return load_model(os.path.join(_ASSETS, name + ".json"))


def initial_state(has_object: bool, fetch_env: bool, mesh_inertia: str = "legacy", mocap: bool = False, table: Optional[dict] = None):
    """(init_qpos, init_qvel, init_ctrl, initial_gripper_xpos, height_offset): what ``_env_setup`` and the
    constructor snapshot (mycobot.py:78-82, 450-472).  Non-fetch: qpos0 / zero ctrl; fetch: keyframe 0.
    ``init_ctrl`` always has the engine's 7 slots; the mocap model's single (finger) actuator is slot 6.
    ``table``: a compiled model table (``load_model`` output) to take all of it from instead of the built-in tables."""
    from .model.specialize import initial_gripper_xpos
    if table is not None:
        return _table_initial_state(table, has_object, fetch_env, mesh_inertia, mocap)
    full = load_table(True, mesh_inertia, mocap)
    tab = full if has_object else load_table(False, mesh_inertia, mocap)
    nq, nv = tab["nq"], tab["nv"]
    if fetch_env:
        key = full["keys"][0]
        qpos = np.asarray(key["qpos"], dtype=np.float64)[:nq].copy()
        qvel = np.asarray(key["qvel"], dtype=np.float64)[:nv].copy()
        ctrl = np.zeros(7); kc = np.asarray(key["ctrl"], dtype=np.float64)
        ctrl[7 - len(kc):] = kc
        height = float(key["qpos"][14])            # z of site object0 after mj_resetDataKeyframe + mj_forward
    else:
        qpos = np.asarray(tab["qpos0"], dtype=np.float64).copy()
        qvel = np.zeros(nv); ctrl = np.zeros(7)
        height = float(full["qpos0"][14])
    igx = initial_gripper_xpos(tab, qpos)
    return qpos, qvel, ctrl, igx, height


def _table_initial_state(table: dict, has_object: bool, fetch_env: bool, mesh_inertia: str, mocap: bool):
    """initial_state of one given table: its qpos0 (or keyframe 0), the EEF site and the z of site object0 by its own kinematics.  A table
    without the cube (Reach) has no object0 site: its height_offset, which Reach does not read, is the built-in one."""
    from .model.mjcf import _np_model
    from .model.refdyn import kinematics
    from .model.specialize import initial_gripper_xpos
    tab = _np_model(table)
    nq, nv = (19, 18) if has_object else (12, 12)            # the engine's state: the cube's free joint with PickAndPlace only
    if fetch_env:
        key = tab["keys"][0]
        qfull = np.asarray(key["qpos"], dtype=np.float64)[:tab["nq"]].copy()
        qvel = np.asarray(key["qvel"], dtype=np.float64)[:nv].copy()
        ctrl = np.zeros(7); kc = np.asarray(key["ctrl"], dtype=np.float64)
        ctrl[7 - len(kc):] = kc
    else:
        qfull = np.asarray(tab["qpos0"], dtype=np.float64).copy()
        qvel = np.zeros(nv); ctrl = np.zeros(7)
    if len(qfull) < nq:
        raise ValueError(f"the table has {len(qfull)} qpos entries; this configuration needs {nq} (PickAndPlace needs the cube)")
    igx = initial_gripper_xpos(tab, qfull)
    if "object0" in tab["site_name"]:
        height = float(kinematics(tab, qfull)["site_xpos"][tab["site_name"].index("object0")][2])
    else:
        height = initial_state(has_object, fetch_env, mesh_inertia, mocap)[4]
    return qfull[:nq], qvel, ctrl, igx, height


def load_scene(path: Optional[str] = None) -> dict:
    """The compiled scene (tools/compile_scene.py): the world cameras, the body cameras, the light, the colours."""
    with open(path or os.path.join(_ASSETS, "scene.json")) as f:
        return json.load(f)


def validate_scenes(scenes: torch.Tensor, num_envs: Optional[int] = None) -> None:
    """What ``mcg_render`` checks of a scene on the host, for every row of a scene table (float64 [N, 40], any device): ``cam_mat``
    orthonormal to 1e-9, ``fovy`` in (0, 180), ``light_dir`` a unit vector to 1e-9, the colours in [0, 1], everything finite.  Raises
    ``ValueError`` naming the first bad row.  The kernel draws any row safely; a bad one gives a bad picture of its environment."""
    A = _abi
    if not (isinstance(scenes, torch.Tensor) and scenes.dtype == torch.float64 and scenes.dim() == 2
            and scenes.shape[1] == A.SCENE_ENV_DOUBLES and (num_envs is None or scenes.shape[0] == num_envs)):
        raise ValueError(f"scenes: expected a float64 tensor [{'N' if num_envs is None else num_envs}, {A.SCENE_ENV_DOUBLES}]")
    R = scenes[:, A.SCENE_CAM_MAT:A.SCENE_CAM_MAT + 9].reshape(-1, 3, 3)
    eye = torch.eye(3, dtype=torch.float64, device=scenes.device)
    fovy, light, rgb = scenes[:, A.SCENE_FOVY], scenes[:, A.SCENE_LIGHT_DIR:A.SCENE_LIGHT_DIR + 3], scenes[:, A.SCENE_RGB:A.SCENE_PAD]
    problems = (          # (a comparison with a NaN is false: every test is written so that a NaN fails it)
        ("a value that is not finite", ~torch.isfinite(scenes).all(dim=1)),
        ("cam_mat not orthonormal to 1e-9", ~((R.transpose(1, 2) @ R - eye).abs().amax(dim=(1, 2)) <= 1e-9)),
        ("fovy outside (0, 180)", ~((fovy > 0.0) & (fovy < 180.0))),
        ("light_dir not a unit vector to 1e-9", ~((light.norm(dim=1) - 1.0).abs() <= 1e-9)),
        ("a colour outside [0, 1]", ~((rgb >= 0.0) & (rgb <= 1.0)).all(dim=1)))
    bad = torch.stack([b for _, b in problems])                 # [5, N]
    if bool(bad.any()):
        row = int(torch.nonzero(bad.any(dim=0))[0])
        why = [text for (text, _), b in zip(problems, bad[:, row].tolist()) if b]
        raise ValueError(f"scenes: row {row}: " + "; ".join(why))


class MyCobotVecEnv:
    metadata = {"render_modes": ["rgb_array", "depth_array"], "render_fps": 25}      # mycobot.py:28

    def __init__(self, num_envs: int, has_object: bool = True, block_gripper: bool = False, control_steps: int = 5,
                 controller_type: str = "IK", obj_range: float = 0.1, target_in_the_air: bool = True,
                 distance_threshold: float = 0.01, fetch_env: bool = False, reward_type: str = "sparse",
                 frame_skip: int = 20, max_episode_steps: int = MAX_EPISODE_STEPS, device="cuda:0", seed: int = 0,
                 env_id_offset: int = 0, auto_reset: bool = True, mesh_inertia: str = "legacy",
                 domain_randomization: Optional[dict] = None, model_path: Optional[str] = None,
                 image_obs: bool = False, model: Optional["_abi.McgModel"] = None, weld_rule: str = "common", contact_rule: str = "mujoco",
                 table: Optional[dict] = None, polytopes: Optional[np.ndarray] = None, **unused):
        """``table``: a compiled model table (``mjcf.load_model`` output) to run instead of the built-in model: it is specialised, its
        collision polytopes go to the engine with it, and the initial state (qpos, gripper position, height offset) is its own.
        ``model`` / ``polytopes``: a raw ``mcg_model`` block and the polytope block specialised with it (NULL: the built-in one)."""
        if image_obs:
            raise NotImplementedError("image observations (-v1 ids, MyCobotImgEnv) are a class of their own: MyCobotImgVecEnv "
                                      "(make() picks it for the -v1 ids)")
        if controller_type == "delta_joint":
            raise NotImplementedError("delta_joint has no branch in the reference's step() (SURVEY D-10)")
        if controller_type not in _CONTROLLERS:
            raise ValueError(f"controller_type must be one of mocap, IK, joint, delta_joint; got {controller_type!r}")
        if reward_type not in _REWARDS:
            raise ValueError(f"unknown reward_type {reward_type!r}")
        if controller_type == "joint" and fetch_env:
            raise AssertionError("Joint controller not supported for Fetch env")        # mycobot.py:96
        self.device = torch.device(device)
        if self.device.type != "cuda":
            raise _abi.McgError("MyCobotVecEnv runs on an AMD GPU only (device='cuda:N'); there is no CPU path")
        self._lib = _abi.load()
        if not torch.cuda.is_available():
            raise _abi.McgError("no GPU visible to PyTorch-ROCm; MyCobotVecEnv has no CPU path")
        if model_path is not None:          # the registry's kwarg (mycobotgym/__init__.py:12): only the built-in, precompiled assets exist here
            want = f"mycobot280{'_mocap' if controller_type == 'mocap' else ''}.xml"
            if os.path.basename(str(model_path)) != want:
                raise ValueError(f"model_path {model_path!r}: this engine runs the precompiled {want} only (compile another MJCF with "
                                 "tools/compile_model.py and pass the table as table=...)")
        self.num_envs = int(num_envs)
        self.has_object, self.fetch_env = bool(has_object), bool(fetch_env)
        # Reach + reward_shaping keeps the (hidden) cube in the physics: stage_rewards reads it (mycobot.py:402-448, 475-481)
        self.hidden_object = (not self.has_object) and reward_type == "reward_shaping"
        self.controller_type, self.reward_type = controller_type, reward_type
        self.distance_threshold = float(distance_threshold)
        self.frame_skip, self.control_steps = int(frame_skip), int(control_steps)
        self.max_episode_steps = int(max_episode_steps)
        self.obj_range = obj_range

        mocap = controller_type == "mocap"
        if table is not None:
            if model is not None or polytopes is not None:
                raise ValueError("table= specialises its own model and polytope blocks: do not pass model= or polytopes= with it")
            from .model.mjcf import _np_model
            from .model.specialize import specialize
            spec = specialize(_np_model(table), weld_rule=weld_rule, contact_rule=contact_rule)
            model = _abi.McgModel.from_spec(spec)
            polytopes = spec.get("polytopes")          # absent from a table without the cube (Reach): the kernels collide nothing there
        qpos, qvel, ctrl, igx, height = initial_state(self.has_object or self.hidden_object, self.fetch_env, mesh_inertia, mocap, table=table)
        self.initial_gripper_xpos, self.height_offset = igx, height
        cfg = _abi.McgConfig()
        cfg.n_envs = self.num_envs; cfg.has_object = int(self.has_object)
        cfg.controller = _CONTROLLERS[controller_type]; cfg.fetch_env = int(self.fetch_env)
        cfg.reward_type = _REWARDS[reward_type]; cfg.frame_skip = self.frame_skip
        cfg.control_steps = self.control_steps; cfg.max_episode_steps = self.max_episode_steps
        cfg.target_in_the_air = int(target_in_the_air); cfg.auto_reset = int(auto_reset)
        cfg.block_gripper = int(block_gripper)
        cfg.distance_threshold = self.distance_threshold; cfg.height_offset = height
        for k in range(3): cfg.initial_gripper_xpos[k] = igx[k]
        for k, v in enumerate(qpos): cfg.init_qpos[k] = v
        for k, v in enumerate(qvel): cfg.init_qvel[k] = v
        for k, v in enumerate(ctrl): cfg.init_ctrl[k] = v
        if domain_randomization:
            cfg.dr_enable = 1
            cfg.dr_mass_range[0], cfg.dr_mass_range[1] = domain_randomization.get("mass", (1.0, 1.0))
            cfg.dr_friction_range[0], cfg.dr_friction_range[1] = domain_randomization.get("friction", (1.0, 1.0))
        cfg.seed = int(seed) & (2 ** 64 - 1); cfg.env_id_offset = int(env_id_offset)
        self._cfg = cfg
        if model is None and (weld_rule != "common" or contact_rule != "mujoco"):
            # weld_rule "mujoco": the mocap weld with MuJoCo's recalled row weights (rotational rows softer); contact_rule "keyframe": the
            # pyramid regulariser that reproduces the cube's rest height of the reference's keyframes (include/mcg.h: contact_rpy)
            from .model.specialize import specialize
            spec = specialize(load_table(True, mesh_inertia, mocap), weld_rule=weld_rule, contact_rule=contact_rule)
            model = _abi.McgModel.from_spec(spec)
            if polytopes is None:
                polytopes = spec["polytopes"]      # the block that goes with the model
        if model is None:     # built-in block; a caller-supplied mcg_model (tests, custom robots) overrides it
            model = _abi.McgModel()
            variant = (1 if mesh_inertia == "exact" else 0) + (2 if mocap else 0)     # 2, 3: mocap body + weld (mycobot280_mocap.xml)
            _abi.check(self._lib.mcg_default_model(variant, C.byref(model)), "mcg_default_model")
        self._model = model
        self._h = C.c_void_p()
        dev_index = self.device.index if self.device.index is not None else torch.cuda.current_device()
        # polytopes None: the built-in collision tables; the array must outlive mcg_create only (the engine copies it)
        poly = None if polytopes is None else np.ascontiguousarray(np.asarray(polytopes, dtype=np.float64).reshape(-1))
        _abi.check(self._lib.mcg_create(C.byref(cfg), C.byref(model), None if poly is None else poly.ctypes.data,
                                        0 if poly is None else len(poly), dev_index, C.byref(self._h)), "mcg_create")
        self.obs_dim = self._lib.mcg_obs_dim(self._h)
        self.action_dim = self._lib.mcg_action_dim(self._h)
        self.nq, self.nv = self._lib.mcg_nq(self._h), self._lib.mcg_nv(self._h)

        # spaces (mycobot.py:108-110, 117-130)
        self.single_action_space = Box(-1.0, 1.0, (self.action_dim,), np.float32)
        self.single_observation_space = Dict({
            "desired_goal": Box(-np.inf, np.inf, (3,), np.float64),
            "achieved_goal": Box(-np.inf, np.inf, (3,), np.float64),
            "observation": Box(-np.inf, np.inf, (self.obs_dim,), np.float64)})
        self.action_space = batch_box(self.single_action_space, self.num_envs)
        self.observation_space = Dict({k: batch_box(v, self.num_envs) for k, v in self.single_observation_space.spaces.items()})

        n, D, dev = self.num_envs, self.obs_dim, self.device
        # flags are torch.bool buffers the kernel fills with 0/1 bytes: no conversion kernels on the step path
        f64 = dict(dtype=torch.float64, device=dev); u8 = dict(dtype=torch.bool, device=dev)
        self._buf = {
            "obs": torch.zeros(n, D, **f64), "achieved_goal": torch.zeros(n, 3, **f64),
            "desired_goal": torch.zeros(n, 3, **f64), "reward": torch.zeros(n, **f64),
            "terminated": torch.zeros(n, **u8), "truncated": torch.zeros(n, **u8), "is_success": torch.zeros(n, **u8),
            "final_obs": torch.zeros(n, D, **f64), "final_achieved": torch.zeros(n, 3, **f64),
            "final_desired": torch.zeros(n, 3, **f64), "ep_return": torch.zeros(n, **f64),
            "ep_length": torch.zeros(n, dtype=torch.int32, device=dev)}
        self._out = _abi.McgStepOut(**{k: v.data_ptr() for k, v in self._buf.items()})
        self._closed = False
        self._needs_reset = True

    # ------------------------------------------------------------------------------------------- Gymnasium API
    _stream = _devbuf.DeviceBuffer._stream

    def _obs(self):
        b = self._buf
        return {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}

    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None, mask: Optional[torch.Tensor] = None):
        """-> (obs dict of device tensors [N, ...], {}).  ``seed`` re-keys the reset RNG (env i uses stream i)."""
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if m.shape != (self.num_envs,):
                raise ValueError("mask must have shape (num_envs,)")
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_reset(self._h, None if m is None else C.c_void_p(m.data_ptr()),
                                           int(seed is not None), C.c_uint64((seed or 0) & (2 ** 64 - 1)),
                                           C.byref(self._out), self._stream()), "mcg_reset")
        self._needs_reset = False
        return self._obs(), {}

    def step(self, actions, copy: bool = True):
        """actions: float32 [N, A] (device tensor; numpy / CPU tensors are copied over).
        -> (obs, reward[N], terminated[N] bool, truncated[N] bool, info).  Like the reference (mycobot.py:280-282) the returned
        arrays are fresh copies; ``copy=False`` hands out the engine's output buffers instead, which the next call overwrites
        (``step_async`` is the raw, packaging-free variant).  The sparse reward is float32, dense / shaped float64 (mycobot.py:293-298)."""
        if self._needs_reset:
            raise RuntimeError("Cannot call env.step() before calling env.reset()")     # OrderEnforcing [RECALL]
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device).contiguous()
        if a.shape != (self.num_envs, self.action_dim):
            raise ValueError(f"actions must have shape {(self.num_envs, self.action_dim)}, got {tuple(a.shape)}")
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_step(self._h, C.c_void_p(a.data_ptr()), C.byref(self._out), self._stream()), "mcg_step")
        b = {k: v.clone() for k, v in self._buf.items()} if copy else self._buf
        if self.reward_type == "sparse":
            b = dict(b, reward=b["reward"].float())
        terminated, truncated = b["terminated"], b["truncated"]
        done = truncated          # truncated = is_success | time-limit, so it already covers terminated (D-4)
        info = {"is_success": b["is_success"],
                "final_observation": {"observation": b["final_obs"], "achieved_goal": b["final_achieved"],
                                      "desired_goal": b["final_desired"]},
                "_final_observation": done,
                "episode": {"r": b["ep_return"], "l": b["ep_length"]}, "_episode": done}
        obs = {"observation": b["obs"], "achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}
        return obs, b["reward"], terminated, truncated, info

    def step_async(self, actions: torch.Tensor) -> dict:
        """Launch one step on the current stream and return the raw output buffers (no Python-side packaging).
        `actions` must already be a contiguous float32 [N, A] tensor on this device."""
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_step(self._h, C.c_void_p(actions.data_ptr()), C.byref(self._out), self._stream()), "mcg_step")
        return self._buf

    def compute_reward(self, achieved_goal, desired_goal, info=None):
        """Batched GoalEnv reward (mycobot.py:289-298); sparse is returned as float32 like the reference."""
        if self.reward_type == "reward_shaping":
            raise NotImplementedError("reward_shaping depends on simulator state, not on the goals alone")
        ag = torch.as_tensor(achieved_goal, dtype=torch.float64, device=self.device).contiguous()
        dg = torch.as_tensor(desired_goal, dtype=torch.float64, device=self.device).contiguous()
        assert ag.shape == dg.shape                                                 # utils.py:25
        out = torch.empty(ag.shape[:-1], dtype=torch.float64, device=self.device)
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_compute_reward(C.c_void_p(ag.data_ptr()), C.c_void_p(dg.data_ptr()), out.numel(),
                                                    _REWARDS[self.reward_type], self.distance_threshold,
                                                    C.c_void_p(out.data_ptr()), self._stream()), "mcg_compute_reward")
        return out.float() if self.reward_type == "sparse" else out

    # ------------------------------------------------------------------------------------- state (tests, checkpoints)
    def _state_bufs(self):
        n, dev = self.num_envs, self.device
        f64 = dict(dtype=torch.float64, device=dev)
        return {"qpos": torch.zeros(self.nq, n, **f64), "qvel": torch.zeros(self.nv, n, **f64),
                "ctrl": torch.zeros(7, n, **f64), "warm": torch.zeros(self.nv, n, **f64),
                "qpos_lag": torch.zeros(self.nq, n, **f64), "goal": torch.zeros(3, n, **f64),
                "elapsed": torch.zeros(n, dtype=torch.int32, device=dev),
                "episode": torch.zeros(n, dtype=torch.int32, device=dev),
                "dr_scale": torch.ones(2, n, **f64), "ep_return": torch.zeros(n, **f64),
                "ep_length": torch.zeros(n, dtype=torch.int32, device=dev)}

    def get_state(self) -> dict:
        """SoA tensors [dim, N] (the engine's layout): qpos qvel ctrl warm qpos_lag goal elapsed episode dr_scale, the running
        episode statistics ep_return / ep_length, and `seed` (the base seed of the reset streams, a one-element int64 tensor): everything a
        freshly constructed engine needs to continue this one's trajectories, auto-resets included."""
        s = self._state_bufs()
        st = _abi.McgState(**{k: v.data_ptr() for k, v in s.items()})
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_get_state(self._h, C.byref(st), self._stream()), "mcg_get_state")
        seed = int(self._lib.mcg_get_seed(self._h))
        s["seed"] = torch.tensor([seed - 2 ** 64 if seed >= 2 ** 63 else seed], dtype=torch.int64)     # uint64 carried in an int64 tensor
        return s

    def set_state(self, **state):
        if state.get("seed") is not None:
            _abi.check(self._lib.mcg_set_seed(self._h, C.c_uint64(int(torch.as_tensor(state["seed"]).reshape(-1)[0]) & (2 ** 64 - 1))), "mcg_set_seed")
        keep = {}
        for k, ref in self._state_bufs().items():
            if k in state and state[k] is not None:
                t = torch.as_tensor(state[k], dtype=ref.dtype, device=self.device).contiguous()
                if t.shape != ref.shape:
                    raise ValueError(f"{k}: expected shape {tuple(ref.shape)}, got {tuple(t.shape)}")
                keep[k] = t
        st = _abi.McgState(**{k: v.data_ptr() for k, v in keep.items()})
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_set_state(self._h, C.byref(st), self._stream()), "mcg_set_state")
            torch.cuda.current_stream(self.device).synchronize()    # `keep` must outlive the copy kernel
        self._needs_reset = False

    state_dict = get_state

    def load_state_dict(self, sd):
        self.set_state(**sd)

    def time_steps(self, actions, steps: int) -> float:
        """Milliseconds for `steps` back-to-back step kernels, measured with HIP events on the launch stream."""
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device).contiguous()
        ms = C.c_float()
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_time_steps(self._h, C.c_void_p(a.data_ptr()), C.byref(self._out), int(steps),
                                                self._stream(), C.byref(ms)), "mcg_time_steps")
        return float(ms.value)

    # ------------------------------------------------------------------------------------------------- pictures
    def _scene(self, camera: str, scene: Optional[dict]):
        """-> (McgScene, body, znear): a world camera (body -1, no near plane) or one of ``scene["body_cameras"]``, stated in the frame
        of the engine body it rides on."""
        if scene is None:
            if not hasattr(self, "_default_scene"):
                self._default_scene = load_scene()
            scene = self._default_scene
        mounted = scene.get("body_cameras", {})
        if camera in scene["cameras"]:
            return _abi.McgScene.from_dict(scene, camera), -1, 0.0
        if camera in mounted:
            cam = mounted[camera]
            return _abi.McgScene.from_camera(scene, cam), int(cam["body"]), float(cam["znear"])
        raise ValueError(f"unknown camera {camera!r}; the scene has the world cameras {sorted(scene['cameras'])} and the body cameras "
                         f"{sorted(mounted)}")

    def render_into(self, out: dict, camera: str = "sideview", samples: int = 1, show_goal: bool = True,
                    mask: Optional[torch.Tensor] = None, scene: Optional[dict] = None, znear: Optional[float] = None,
                    scenes: Optional[torch.Tensor] = None, validate: Optional[bool] = None):
        """Raw form of ``render``: ``out`` maps any of rgb (uint8 [N, H, W, 3]), gray (uint8 [N, H, W]), depth (float32 [N, H, W]),
        geom (int8 [N, H, W]) to contiguous device tensors of one H, W, which the kernel fills (where ``mask`` is set); enqueued on the
        current stream, not synchronised.  ``camera``: a world camera or a body camera of the scene (``gripper_camera_rgb``: it rides on
        the flange, its pose follows each environment's arm).  ``znear``: the near plane in metres, in place of the camera's own (a
        world camera has none: 0).

        ``scenes``: a scene table, a contiguous float64 device tensor [N, 40] (``randomize_scenes``, or rows made with
        ``_abi.scene_row``): environment e is drawn with the camera, field of view, light and colours of row e, stated in the frame
        ``camera`` rides in; of ``camera`` itself the carrier body and the near plane are used, of ``scene`` the target's size.
        ``validate`` (default: True with ``scenes``): check the rows first (``validate_scenes``; it synchronises)."""
        want = {"rgb": (torch.uint8, 3), "gray": (torch.uint8, None), "depth": (torch.float32, None), "geom": (torch.int8, None)}
        hw = None
        for k, t in out.items():
            if k not in want:
                raise ValueError(f"unknown output {k!r}; known: {sorted(want)}")
            dt, last = want[k]
            shape_ok = t.dim() == (4 if last else 3) and t.shape[0] == self.num_envs and (last is None or t.shape[3] == last)
            if not (shape_ok and t.dtype == dt and t.is_contiguous() and t.device == self._buf["obs"].device):
                raise ValueError(f"{k}: expected a contiguous {dt} device tensor [N, H, W{', 3' if last else ''}]")
            if hw is not None and tuple(t.shape[1:3]) != hw:
                raise ValueError("the outputs differ in height / width")
            hw = tuple(t.shape[1:3])
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if m.shape != (self.num_envs,):
                raise ValueError("mask must have shape (num_envs,)")
        ro = _abi.McgRenderOut(**{k: t.data_ptr() for k, t in out.items()})
        sc, body, cam_znear = self._scene(camera, scene)
        znear = cam_znear if znear is None else float(znear)
        h, w = hw if hw is not None else (0, 0)
        mp = None if m is None else C.c_void_p(m.data_ptr())
        if scenes is not None:
            self._check_table(scenes, "scenes")
            if validate is None or validate:
                validate_scenes(scenes, self.num_envs)
        with torch.cuda.device(self.device):
            if scenes is not None:
                _abi.check(self._lib.mcg_render_scenes(self._h, C.c_void_p(scenes.data_ptr()), sc.target_half, body, znear, int(w), int(h),
                                                       int(samples), int(bool(show_goal)), mp, C.byref(ro), self._stream()),
                           "mcg_render_scenes")
            elif body < 0 and znear == 0.0:
                _abi.check(self._lib.mcg_render(self._h, C.byref(sc), int(w), int(h), int(samples), int(bool(show_goal)), mp, C.byref(ro),
                                                self._stream()), "mcg_render")
            else:
                _abi.check(self._lib.mcg_render_mounted(self._h, C.byref(sc), body, znear, int(w), int(h), int(samples),
                                                        int(bool(show_goal)), mp, C.byref(ro), self._stream()), "mcg_render_mounted")
        return out

    def render(self, camera: str = "sideview", width: int = 480, height: int = 480, samples: int = 1, mode: str = "rgb_array",
               mask: Optional[torch.Tensor] = None, scene: Optional[dict] = None, show_goal: bool = True,
               scenes: Optional[torch.Tensor] = None, validate: Optional[bool] = None):
        """All environments as ``camera`` sees them: ``mode="rgb_array"`` -> uint8 [N, H, W, 3], ``"depth_array"`` -> float32 [N, H, W]
        (distance along the viewing axis, +inf = sky); device tensors.  The target site is drawn at the goal, as the reference's
        ``_render_callback`` does (mycobot.py:308-311).  ``samples``: s x s rays per pixel, box-averaged; ``mask``: draw these environments
        only (the others' images are zero); ``scene``: a compiled scene other than the built-in one (tools/compile_scene.py);
        ``scenes`` / ``validate``: one scene per environment, as ``render_into`` takes it."""
        if mode not in self.metadata["render_modes"]:
            raise ValueError(f"mode must be one of {self.metadata['render_modes']}, got {mode!r}")
        n, dev = self.num_envs, self.device
        if mode == "rgb_array":
            out = {"rgb": torch.zeros(n, int(height), int(width), 3, dtype=torch.uint8, device=dev)}
        else:
            out = {"depth": torch.zeros(n, int(height), int(width), dtype=torch.float32, device=dev)}
        self.render_into(out, camera=camera, samples=samples, show_goal=show_goal, mask=mask, scene=scene, scenes=scenes, validate=validate)
        return out["rgb" if mode == "rgb_array" else "depth"]

    def _check_table(self, t, name: str):
        want = (self.num_envs, _abi.SCENE_ENV_DOUBLES)
        if not (isinstance(t, torch.Tensor) and t.dtype == torch.float64 and tuple(t.shape) == want and t.is_contiguous()
                and t.device == self._buf["obs"].device):
            raise ValueError(f"{name}: expected a contiguous float64 device tensor {list(want)}")

    def randomize_scenes(self, ranges: dict, camera: str = "sideview", cam_slot: int = 0, scene: Optional[dict] = None,
                         mask: Optional[torch.Tensor] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """A scene table, float64 [N, 40], for ``render_into(..., camera=camera, scenes=table)``: ``camera``'s base scene jittered per
        environment and per episode (``mcg_scene_randomize``).  ``ranges``: keyed by the fields of ``mcg_scene_rand`` -- ``cam_pos`` (m) and
        ``cam_rot`` (rad, a rotation vector): half ranges, one number or three; ``fovy_scale``, ``light_ambient_scale``,
        ``light_diffuse_scale``, ``head_scale``: (lo, hi); ``light_tilt`` (rad); ``rgb``: a half range, one number or a dict by colour
        class (ground, table, cube, target, mesh, sky); a missing key means no jitter.  The draw is keyed by (seed, global environment
        id, episode, draw index), like the goals and the physics randomisation: a table is a function of the engine's state.  Light and
        colours are the same for every ``cam_slot`` (0..7) of an environment, the camera's own jitter differs between slots.  ``mask``:
        the rows to draw (the others of ``out`` stay as they are; without ``out`` they are the base scene's); enqueued, not synchronised."""
        base = self._scene(camera, scene)[0]
        rr = _abi.McgSceneRand.from_dict(ranges)
        m = None
        if mask is not None:
            m = mask.to(device=self.device, dtype=torch.uint8).contiguous()
            if m.shape != (self.num_envs,):
                raise ValueError("mask must have shape (num_envs,)")
        if out is None:
            out = torch.as_tensor(_abi.scene_row(base), device=self.device).repeat(self.num_envs, 1).contiguous()
        self._check_table(out, "out")
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_scene_randomize(self._h, C.byref(base), C.byref(rr), int(cam_slot), None if m is None else C.c_void_p(m.data_ptr()),
                                                     C.c_void_p(out.data_ptr()), self._stream()), "mcg_scene_randomize")
        return out

    def counters(self, clear: bool = False) -> dict:
        """Event counters of the engine (include/mcg.h: mcg_counters); synchronises the device."""
        c = _abi.McgCounters()
        _abi.check(self._lib.mcg_get_counters(self._h, C.byref(c), int(clear)), "mcg_get_counters")
        return {n: int(getattr(c, n)) for n, _ in c._fields_}

    def debug_contacts(self) -> dict:
        """TEST / DEBUG: the collision pass of the current state as the kernels see it (mcg_debug_contacts): per env the number of
        list entries, the contacts the cap cut off, and per entry dist, pos[3], normal[3], pair type, multiplicity, D."""
        n = self.num_envs
        count = torch.zeros(n, dtype=torch.int32, device=self.device); dropped = torch.zeros_like(count)
        data = torch.zeros(n, _abi.MAXCON, 10, dtype=torch.float64, device=self.device)
        _abi.check(self._lib.mcg_debug_contacts(self._h, count.data_ptr(), dropped.data_ptr(), data.data_ptr(), self._stream()), "mcg_debug_contacts")
        torch.cuda.synchronize(self.device)
        return {"count": count, "dropped": dropped, "dist": data[:, :, 0], "pos": data[:, :, 1:4], "normal": data[:, :, 4:7],
                "type": data[:, :, 7].to(torch.int32), "mult": data[:, :, 8], "D": data[:, :, 9]}

    def close(self):
        if not self._closed and getattr(self, "_h", None):
            torch.cuda.synchronize(self.device)
            self._lib.mcg_destroy(self._h)
            self._closed = True

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class MyCobotImgVecEnv(MyCobotVecEnv):
    """Mirror of the reference's ``MyCobotImgEnv`` (mycobot.py:517-545): the observation is the picture alone -- uint8 [N, 1, S, S], camera
    ``sideview``, grayscale as ``preprocess_frame`` makes it (utils.py:580-595) -- not a Dict; ``achieved_goal`` / ``desired_goal`` travel
    in ``info``.

    ``camera``: a world camera's or a body camera's name (``"gripper_camera_rgb"``: the wrist view), or a tuple of names: the observation
    is then uint8 [N, C, S, S], one channel per camera in the order given, at the cost of one launch per camera (the channels are
    planes of one [C, N, S, S] buffer, which the kernel fills in place; the observation is its [N, C, S, S] view).

    The reference's ``_get_obs`` calls the renderer directly, not ``render()``: the target site is NOT moved to the goal in its observations
    and stays at its MJCF position (SURVEY D-15).  ``show_goal=True`` draws it at the goal instead.

    ``visual_randomization``: None, or a dict of ranges as ``randomize_scenes`` takes it, optionally with ``"cameras": {name: overrides}``:
    every environment is drawn with its own camera pose, field of view, light and colours, redrawn for every episode.  One scene table
    per camera (``cam_slot`` = the camera's place in the tuple: light and colours agree between the cameras of an environment); the
    tables are drawn after ``reset()`` and, in ``step()``, for the finished environments after their reset, so ``final_observation``
    shows the finished episode's own scene; ``set_state`` / ``load_state_dict`` redraw them: they are a function of the state (seed,
    episode), ``state_dict()`` does not carry them.  None: the calls made are those made without this keyword.

    Auto-reset: the picture of the pre-reset state is ``info["final_observation"]``, and the step kernel's own auto-reset would have
    overwritten that state.  So the engine runs with ``auto_reset=0``; a step renders, resets the finished environments with the masked
    ``mcg_reset`` (the same per-environment random streams as the in-kernel reset) and draws those again."""

    def __init__(self, num_envs: int, *args, camera: str = "sideview", image_size: int = 64, samples: int = 2, show_goal: bool = False,
                 scene: Optional[dict] = None, auto_reset: bool = True, image_obs: bool = True,
                 visual_randomization: Optional[dict] = None, **kwargs):
        if kwargs.get("reward_type", "sparse") == "reward_shaping":
            raise ValueError("the reference registers no image variant for reward_shaping (mycobotgym/__init__.py:37-39)")
        self._img_auto_reset = bool(auto_reset)
        super().__init__(num_envs, *args, auto_reset=False, image_obs=False, **kwargs)
        self.camera, self.image_size, self.samples, self.show_goal = camera, int(image_size), int(samples), bool(show_goal)
        self._cameras = (camera,) if isinstance(camera, str) else tuple(camera)
        if not self._cameras:
            raise ValueError("camera: a name or a non-empty tuple of names")
        self._img_scene = scene
        for cam in self._cameras:
            self._scene(cam, scene)                # an unknown camera fails here, not at the first step
        s, c = self.image_size, len(self._cameras)
        self.single_observation_space = Box(0, 255, (c, s, s), np.uint8)         # mycobot.py:543-545
        self.observation_space = batch_box(self.single_observation_space, self.num_envs)
        # one contiguous [N, S, S] plane per camera; the observation is the [N, C, S, S] view of the planes
        self._img = torch.zeros(c, self.num_envs, s, s, dtype=torch.uint8, device=self.device).permute(1, 0, 2, 3)
        self._final_img = torch.zeros(c, self.num_envs, s, s, dtype=torch.uint8, device=self.device).permute(1, 0, 2, 3)
        # visual randomisation: one scene table per camera (cam_slot = its place in the tuple), a function of the engine's state
        self._vr_ranges, self._vr_tables = None, None
        if visual_randomization is not None:
            if len(self._cameras) > _abi.SCENE_RAND_CAM_SLOTS:
                raise ValueError(f"visual_randomization: at most {_abi.SCENE_RAND_CAM_SLOTS} cameras")
            common = {k: v for k, v in visual_randomization.items() if k != "cameras"}
            per_cam = visual_randomization.get("cameras", {})
            if set(per_cam) - set(self._cameras):
                raise ValueError(f"visual_randomization['cameras']: {sorted(set(per_cam) - set(self._cameras))} not among {self._cameras}")
            self._vr_ranges = [dict(common, **per_cam.get(cam, {})) for cam in self._cameras]
            for r in self._vr_ranges:
                _abi.McgSceneRand.from_dict(r)             # an unknown key fails here
            self._vr_tables = [torch.as_tensor(_abi.scene_row(self._scene(cam, scene)[0]), device=self.device).repeat(self.num_envs, 1).contiguous()
                               for cam in self._cameras]

    @property
    def channels(self) -> int:
        """Channels of the observation: one per camera."""
        return len(self._cameras)

    def _redraw_scenes(self, mask: Optional[torch.Tensor] = None):
        """The scene tables of the current episodes (where ``mask`` is set)."""
        if self._vr_tables is None:
            return
        for c, cam in enumerate(self._cameras):
            self.randomize_scenes(self._vr_ranges[c], camera=cam, cam_slot=c, scene=self._img_scene, mask=mask, out=self._vr_tables[c])

    def _draw(self, dst: torch.Tensor, mask: Optional[torch.Tensor] = None):
        for c, cam in enumerate(self._cameras):
            if self._vr_tables is None:
                self.render_into({"gray": dst[:, c]}, camera=cam, samples=self.samples, show_goal=self.show_goal, mask=mask,
                                 scene=self._img_scene)
            else:       # (the draw kernel's own rows: not validated)
                self.render_into({"gray": dst[:, c]}, camera=cam, samples=self.samples, show_goal=self.show_goal, mask=mask,
                                 scene=self._img_scene, scenes=self._vr_tables[c], validate=False)

    def set_state(self, **state):
        super().set_state(**state)
        self._redraw_scenes()             # the tables are a function of (seed, episode): a checkpoint does not carry them

    def _goal_info(self, b: dict) -> dict:
        return {"achieved_goal": b["achieved_goal"], "desired_goal": b["desired_goal"]}

    def reset(self, *, seed: Optional[int] = None, options: Optional[dict] = None, mask: Optional[torch.Tensor] = None):
        super().reset(seed=seed, options=options, mask=mask)
        self._redraw_scenes(mask)
        self._draw(self._img, mask)
        return self._img.clone(), self._goal_info({k: v.clone() for k, v in self._obs().items()})

    def step(self, actions, copy: bool = True):
        """-> (image uint8 [N, 1, S, S], reward, terminated, truncated, info); info carries achieved_goal / desired_goal (after the
        auto-reset where done), is_success, final_observation (the picture of the finished episode's last state) / _final_observation,
        final_info-style episode statistics as the state engine's."""
        if self._needs_reset:
            raise RuntimeError("Cannot call env.step() before calling env.reset()")
        a = torch.as_tensor(actions, dtype=torch.float32, device=self.device).contiguous()
        if a.shape != (self.num_envs, self.action_dim):
            raise ValueError(f"actions must have shape {(self.num_envs, self.action_dim)}, got {tuple(a.shape)}")
        with torch.cuda.device(self.device):
            _abi.check(self._lib.mcg_step(self._h, C.c_void_p(a.data_ptr()), C.byref(self._out), self._stream()), "mcg_step")
        b = self._buf
        # what the step itself decided, before the reset below rewrites the observation buffers
        step_out = {k: b[k].clone() for k in ("reward", "terminated", "truncated", "is_success", "ep_return", "ep_length")}
        done = step_out["truncated"]          # truncated = is_success | time-limit: covers terminated (D-4)
        self._draw(self._img)
        final_img = self._final_img
        final_goals = {"achieved_goal": b["achieved_goal"].clone(), "desired_goal": b["desired_goal"].clone()}
        if self._img_auto_reset:
            final_img.copy_(self._img)
            m = done.to(torch.uint8)
            with torch.cuda.device(self.device):      # resets the finished environments only; rewrites their rows of obs / goals
                _abi.check(self._lib.mcg_reset(self._h, C.c_void_p(m.data_ptr()), 0, C.c_uint64(0), C.byref(self._out), self._stream()),
                           "mcg_reset")
            self._redraw_scenes(m)        # after final_img: the finished episode's last picture shows its own scene
            self._draw(self._img, m)
        reward = step_out["reward"].float() if self.reward_type == "sparse" else step_out["reward"]
        info = {"is_success": step_out["is_success"],
                # (the reset kernel re-derives every environment's goals from the state: keep the step's own where nothing was reset)
                "achieved_goal": torch.where(done[:, None], b["achieved_goal"], final_goals["achieved_goal"]),
                "desired_goal": torch.where(done[:, None], b["desired_goal"], final_goals["desired_goal"]),
                "final_observation": final_img.clone() if copy else final_img, "_final_observation": done,
                "final_achieved_goal": final_goals["achieved_goal"], "final_desired_goal": final_goals["desired_goal"],
                "episode": {"r": step_out["ep_return"], "l": step_out["ep_length"]}, "_episode": done}
        return (self._img.clone() if copy else self._img), reward, step_out["terminated"], step_out["truncated"], info

    def step_async(self, actions: torch.Tensor) -> dict:
        raise NotImplementedError("the image environment's step is several launches (step, render, masked reset, render): use step()")


def env_class(env_id: str):
    """The class ``make`` constructs for a registered id: ``MyCobotImgVecEnv`` for the 20 ``-v1`` ids, ``MyCobotVecEnv`` for the 30 ``-v0``."""
    return MyCobotImgVecEnv if _spec(env_id)["image_obs"] else MyCobotVecEnv


def make(env_id: str, num_envs: int = 1, **kwargs) -> MyCobotVecEnv:
    """``gymnasium.make``-style factory over the reference's id table, vectorised."""
    kw = _spec(env_id)
    kw.update(kwargs)
    image_obs = kw.pop("image_obs")
    return (MyCobotImgVecEnv if image_obs else MyCobotVecEnv)(num_envs, **kw)
