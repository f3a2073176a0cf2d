"""ctypes mirror of ``include/mcg.h`` and loader of the in-tree HIP library.

The library is the product: if it is missing or cannot be loaded this module raises --
there is no CPU or PyTorch fallback anywhere in the package.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
# MCG_LIB selects another build of the same library (kernel A/B timing, tools/ab_bench.py); default: the in-tree one
LIB_PATH = os.environ.get("MCG_LIB") or os.path.join(_HERE, "libmycobot_hip.so")

MCG_OK, MCG_ERR_ARG, MCG_ERR_HIP, MCG_ERR_UNSUPPORTED = 0, 1, 2, 3
CTRL_JOINT, CTRL_IK, CTRL_MOCAP = 0, 1, 2
ABI_VERSION = 8
MAXCON, NMESH = 16, 14
REWARD_SPARSE, REWARD_DENSE, REWARD_SHAPING = 0, 1, 2

d = C.c_double


class McgBody(C.Structure):
    _fields_ = [("r", d * 3), ("mass", d), ("mc", d * 3), ("inertia", d * 6), ("armature", d), ("damping", d), ("hull_rad", d)]


class McgModel(C.Structure):
    _fields_ = [
        ("timestep", d),
        ("base_pos", d * 3), ("base_mat", d * 9), ("gravity_base", d * 3),
        ("body", (d * 16) * 13),          # mcg_body[13], see McgBody for the layout of one row
        ("cube_damping", d * 6),
        ("jnt_range", (d * 2) * 12),
        ("limit_par", (d * 10) * 12),
        ("limit_diag", d * 12),
        ("eq_anchor1", (d * 3) * 2), ("eq_anchor2", (d * 3) * 2),
        ("eq_par", (d * 10) * 3), ("eq_diag", d * 3),
        ("act_gain", d * 7), ("act_bias", (d * 3) * 7), ("act_ctrlrange", (d * 2) * 7),
        ("act_forcerange", (d * 2) * 7), ("tendon_coef", d * 2),
        ("site_eef", d * 3),
        ("cube_half", d * 3), ("table_pos", d * 3), ("table_half", d * 3), ("pad_box", (d * 6) * 2),
        ("contact_par", (d * 15) * 7),
        ("contact_diag", (d * 2) * 5),
        ("mesh_box", (d * 6) * NMESH), ("mesh_mult", d), ("mesh_fric", d), ("pair_tran", d * (5 + 2 * NMESH)),
        ("geom_friction0", d * 3),
        ("base_quat", d * 4), ("weld_on", d), ("weld_par", d * 10), ("weld_diag", d * 2), ("weld_anchor", d * 3),
        ("weld_relpos", d * 3), ("weld_relquat", d * 4), ("weld_torquescale", d),
        ("target0", d * 3),
        ("contact_rpy", d),
    ]

    @classmethod
    def from_spec(cls, spec: dict) -> "McgModel":
        """Fill from ``mycobotgym_amd.model.specialize.specialize`` output."""
        m = cls()
        for name, ctype in cls._fields_:
            if name not in spec:
                continue                       # cube fields of a Reach-only table stay zero
            v = np.ascontiguousarray(np.asarray(spec[name], dtype=np.float64))
            if ctype is d:
                setattr(m, name, float(v.reshape(-1)[0]))
            else:
                dst = np.ctypeslib.as_array(getattr(m, name))
                dst[...] = v.reshape(dst.shape)
        return m


class McgConfig(C.Structure):
    _fields_ = [
        ("n_envs", C.c_int32), ("has_object", C.c_int32), ("controller", C.c_int32), ("fetch_env", C.c_int32),
        ("reward_type", C.c_int32), ("frame_skip", C.c_int32), ("control_steps", C.c_int32),
        ("max_episode_steps", C.c_int32), ("target_in_the_air", C.c_int32), ("auto_reset", C.c_int32),
        ("dr_enable", C.c_int32), ("block_gripper", C.c_int32),
        ("distance_threshold", d), ("height_offset", d), ("initial_gripper_xpos", d * 3),
        ("init_qpos", d * 19), ("init_qvel", d * 18), ("init_ctrl", d * 7),
        ("dr_mass_range", d * 2), ("dr_friction_range", d * 2),
        ("seed", C.c_uint64), ("env_id_offset", C.c_int64),
    ]


class McgCounters(C.Structure):
    _fields_ = [(n, C.c_uint64) for n in ("reset_cap_hits", "bad_state_resets", "contacts_dropped", "coupled_env_substeps")]


class McgStepOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in (
        "obs", "achieved_goal", "desired_goal", "reward", "terminated", "truncated", "is_success",
        "final_obs", "final_achieved", "final_desired", "ep_return", "ep_length")]


class McgState(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("qpos", "qvel", "ctrl", "warm", "qpos_lag", "goal", "elapsed", "episode", "dr_scale",
                                          "ep_return", "ep_length")]


class McgScene(C.Structure):
    """One camera + light + colours (include/mcg.h: mcg_scene); ``from_dict`` fills it from a compiled scene (assets/scene.json)."""
    _fields_ = [("cam_pos", d * 3), ("cam_mat", d * 9), ("fovy", d), ("light_dir", d * 3), ("light_ambient", d), ("light_diffuse", d),
                ("head_ambient", d), ("head_diffuse", d), ("rgb_ground", d * 3), ("rgb_table", d * 3), ("rgb_cube", d * 3),
                ("rgb_target", d * 3), ("rgb_mesh", d * 3), ("rgb_sky", d * 3), ("target_half", d * 3)]

    @classmethod
    def from_dict(cls, scene: dict, camera: str) -> "McgScene":
        if camera not in scene["cameras"]:
            raise ValueError(f"unknown camera {camera!r}; the scene has {sorted(scene['cameras'])}")
        return cls.from_camera(scene, scene["cameras"][camera])

    @classmethod
    def from_camera(cls, scene: dict, cam: dict) -> "McgScene":
        """``cam``: pos, mat, fovy -- a world camera, or a body camera (``scene["body_cameras"]``) stated in its carrier body's frame."""
        s = cls()
        vals = {"cam_pos": cam["pos"], "cam_mat": np.asarray(cam["mat"], dtype=np.float64).reshape(-1), "light_dir": scene["light"]["dir"],
                "target_half": scene["target_half"]}
        vals.update({"rgb_" + k: v for k, v in scene["rgb"].items()})
        for k, v in vals.items():
            dst = getattr(s, k)
            for j, x in enumerate(v):
                dst[j] = float(x)
        s.fovy = float(cam["fovy"])
        s.light_ambient, s.light_diffuse = float(scene["light"]["ambient"]), float(scene["light"]["diffuse"])
        s.head_ambient, s.head_diffuse = float(scene["headlight"]["ambient"]), float(scene["headlight"]["diffuse"])
        return s


class McgRenderOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("rgb", "gray", "depth", "geom")]


# one row of a scene table (include/mcg.h: MCG_SCENE_*): camera, light, shading coefficients and colours of one environment
SCENE_ENV_DOUBLES = 40
SCENE_CAM_POS, SCENE_CAM_MAT, SCENE_FOVY, SCENE_LIGHT_DIR = 0, 3, 12, 13
SCENE_LIGHT_AMBIENT, SCENE_LIGHT_DIFFUSE, SCENE_HEAD_AMBIENT, SCENE_HEAD_DIFFUSE = 16, 17, 18, 19
SCENE_RGB, SCENE_PAD = 20, 38
SCENE_RAND_CAM_SLOTS = 8
RGB_CLASSES = ("ground", "table", "cube", "target", "mesh", "sky")       # the order of a row's colours, and of mcg_scene_rand.rgb


class McgSceneRand(C.Structure):
    """Ranges of mcg_scene_randomize (include/mcg.h: mcg_scene_rand); ``from_dict``: missing keys mean no jitter."""
    _fields_ = [("cam_pos", d * 3), ("cam_rot", d * 3), ("fovy_scale", d * 2), ("light_tilt", d), ("light_ambient_scale", d * 2),
                ("light_diffuse_scale", d * 2), ("head_scale", d * 2), ("rgb", d * 6)]

    @classmethod
    def from_dict(cls, ranges: dict) -> "McgSceneRand":
        known = {n for n, _ in cls._fields_}
        if set(ranges) - known:
            raise ValueError(f"unknown range(s) {sorted(set(ranges) - known)}; known: {sorted(known)}")
        r = cls()
        for name in ("cam_pos", "cam_rot"):       # a half range: one number for the three components, or three
            v = np.broadcast_to(np.asarray(ranges.get(name, 0.0), dtype=np.float64), (3,))
            for j in range(3):
                getattr(r, name)[j] = float(v[j])
        for name in ("fovy_scale", "light_ambient_scale", "light_diffuse_scale", "head_scale"):
            lo, hi = ranges.get(name, (1.0, 1.0))
            getattr(r, name)[0], getattr(r, name)[1] = float(lo), float(hi)
        r.light_tilt = float(ranges.get("light_tilt", 0.0))
        rgb = ranges.get("rgb", 0.0)
        if isinstance(rgb, dict):
            if set(rgb) - set(RGB_CLASSES):
                raise ValueError(f"rgb: unknown colour class(es) {sorted(set(rgb) - set(RGB_CLASSES))}; known: {list(RGB_CLASSES)}")
            rgb = [rgb.get(k, 0.0) for k in RGB_CLASSES]
        v = np.broadcast_to(np.asarray(rgb, dtype=np.float64), (6,))
        for j in range(6):
            r.rgb[j] = float(v[j])
        return r


def scene_row(scene, camera=None) -> np.ndarray:
    """One row of a scene table, float64 [40]: of an ``McgScene``, or of a compiled scene dict and ``camera`` (a world or body camera's
    name, or a camera dict pos / mat / fovy).  A row is the head of ``mcg_scene`` (everything before ``target_half``) and two zeros."""
    if not isinstance(scene, McgScene):
        if isinstance(camera, dict):
            cam = camera
        elif camera in scene["cameras"]:
            cam = scene["cameras"][camera]
        elif camera in scene.get("body_cameras", {}):
            cam = scene["body_cameras"][camera]
        else:
            raise ValueError(f"unknown camera {camera!r}")
        scene = McgScene.from_camera(scene, cam)
    row = np.zeros(SCENE_ENV_DOUBLES)
    row[:SCENE_PAD] = np.frombuffer(bytes(scene), dtype=np.float64)[:SCENE_PAD]
    return row


def scene_from_row(row, target_half=None):
    """Inverse of ``scene_row``: -> (camera dict pos / mat / fovy, scene dict light / headlight / rgb), the shapes the compiled scene has
    (a body camera's pos / mat stay in its carrier's frame).  ``target_half`` is not part of a row: given, it goes into the scene dict."""
    r = np.asarray(row, dtype=np.float64).reshape(-1)
    if r.shape != (SCENE_ENV_DOUBLES,):
        raise ValueError(f"a row has {SCENE_ENV_DOUBLES} doubles, got {r.shape}")
    cam = {"pos": r[SCENE_CAM_POS:SCENE_CAM_POS + 3].tolist(), "mat": r[SCENE_CAM_MAT:SCENE_CAM_MAT + 9].reshape(3, 3).tolist(),
           "fovy": float(r[SCENE_FOVY])}
    scene = {"light": {"dir": r[SCENE_LIGHT_DIR:SCENE_LIGHT_DIR + 3].tolist(), "ambient": float(r[SCENE_LIGHT_AMBIENT]),
                       "diffuse": float(r[SCENE_LIGHT_DIFFUSE])},
             "headlight": {"ambient": float(r[SCENE_HEAD_AMBIENT]), "diffuse": float(r[SCENE_HEAD_DIFFUSE])},
             "rgb": {k: r[SCENE_RGB + 3 * j:SCENE_RGB + 3 * j + 3].tolist() for j, k in enumerate(RGB_CLASSES)}}
    if target_half is not None:
        scene["target_half"] = [float(x) for x in target_half]
    return cam, scene


class McgHerBuf(C.Structure):
    """The replay buffer's device memory and shape (include/mcg.h: mcg_her_buf); the caller owns every pointer."""
    _fields_ = [("records", C.c_void_p), ("t_run", C.c_void_p), ("last_obs", C.c_void_p), ("last_achieved", C.c_void_p),
                ("counters", C.c_void_p), ("n_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("capacity", C.c_int32),
                ("max_episode_steps", C.c_int32), ("reward_type", C.c_int32), ("distance_threshold", d)]


class McgHerBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "achieved", "desired", "next_obs", "next_achieved", "action", "reward", "done", "index")]


def her_record_dtype(obs_dim: int, act_dim: int) -> np.dtype:
    """One record of the replay ring as a numpy structured dtype (include/mcg.h: the layout above mcg_her_buf)."""
    fields = [("achieved", "<f8", (3,)), ("next_achieved", "<f8", (3,)), ("desired", "<f8", (3,)),
              ("obs", "<f4", (obs_dim,)), ("next_obs", "<f4", (obs_dim,)), ("action", "<f4", (act_dim,)), ("reward", "<f4"),
              ("t_in_ep", "<i4"), ("ep_len", "<i4"), ("terminated", "u1")]
    used = np.dtype(fields).itemsize
    return np.dtype(fields + [("pad", "u1", ((used + 15) // 16 * 16 - used,))])


class McgRolloutBuf(C.Structure):
    """The rollout buffer's device memory, shape and discounting (include/mcg.h: mcg_rollout_buf); the caller owns every pointer."""
    _fields_ = ([(n, C.c_void_p) for n in ("records", "reward", "value", "episode_start", "advantage", "returns", "last_obs", "last_goals",
                                           "last_start")]
                + [("n_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_steps", C.c_int32), ("gamma", d), ("gae_lambda", d)])


class McgRolloutBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "achieved", "desired", "action", "old_value", "old_log_prob", "advantage", "returns", "index")]


def rollout_record_dtype(obs_dim: int, act_dim: int) -> np.dtype:
    """One record of the rollout buffer as a numpy structured dtype (include/mcg.h: the layout above mcg_rollout_buf)."""
    fields = [("obs", "<f4", (obs_dim,)), ("achieved", "<f4", (3,)), ("desired", "<f4", (3,)), ("action", "<f4", (act_dim,)), ("log_prob", "<f4")]
    used = np.dtype(fields).itemsize
    return np.dtype(fields + [("pad", "u1", ((used + 15) // 16 * 16 - used,))])


class McgRolloutImgBuf(C.Structure):
    """The picture rollout buffer's device memory, shape and discounting (include/mcg.h: mcg_rollout_img_buf); the caller owns every pointer."""
    _fields_ = ([(n, C.c_void_p) for n in ("pixels", "records", "reward", "value", "episode_start", "advantage", "returns", "last_start")]
                + [("n_envs", C.c_int32), ("channels", C.c_int32), ("size", C.c_int32), ("act_dim", C.c_int32), ("n_steps", C.c_int32),
                   ("gamma", d), ("gae_lambda", d)])


class McgRolloutImgBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pix", "pix_f32", "action", "old_value", "old_log_prob", "advantage", "returns", "index")]


def rollout_img_record_dtype(act_dim: int) -> np.dtype:
    """One record of the picture rollout buffer as a numpy structured dtype (include/mcg.h: the layout above mcg_rollout_img_buf)."""
    fields = [("action", "<f4", (act_dim,)), ("log_prob", "<f4")]
    used = np.dtype(fields).itemsize
    return np.dtype(fields + [("pad", "u1", ((used + 15) // 16 * 16 - used,))])


class McgReplayImgBuf(C.Structure):
    """The picture replay buffer's device memory and shape (include/mcg.h: mcg_replay_img_buf); the caller owns every pointer."""
    _fields_ = ([(n, C.c_void_p) for n in ("pixels", "finals", "final_time", "records", "counters")]
                + [(n, C.c_int32) for n in ("n_envs", "channels", "size", "act_dim", "capacity", "max_episode_steps")])


class McgReplayImgBatch(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("pix", "next_pix", "pix_f32", "next_pix_f32", "action", "reward", "done", "index")]


REPLAY_IMG_TERMINATED, REPLAY_IMG_TIMEOUT, REPLAY_IMG_NO_NEXT = 1, 2, 4      # a record's flags


def replay_img_record_dtype(act_dim: int) -> np.dtype:
    """One record of the picture replay buffer as a numpy structured dtype (include/mcg.h: the layout above mcg_replay_img_buf)."""
    fields = [("action", "<f4", (act_dim,)), ("reward", "<f4"), ("flags", "<u4")]
    used = np.dtype(fields).itemsize
    return np.dtype(fields + [("pad", "u1", ((used + 15) // 16 * 16 - used,))])


POLICY_TANH, POLICY_RELU = 0, 1


class McgPolicy(C.Structure):
    """The policy's weights and shape (include/mcg.h: mcg_policy); the caller owns the blob."""
    _fields_ = [("blob", C.c_void_p), ("n_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_pi", C.c_int32),
                ("n_vf", C.c_int32), ("pi_width", C.c_int32 * 3), ("vf_width", C.c_int32 * 3), ("activation", C.c_int32),
                ("blob_floats", C.c_int64)]


class McgPolicyOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("action", "value", "log_prob", "mean", "noise")]


class McgPolicyEvalOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("value", "log_prob", "entropy")]


LOSS_PPO, LOSS_A2C = 0, 1


class McgPolicyHyper(C.Structure):
    """The loss's hyper-parameters under SB3's names (include/mcg.h: mcg_policy_hyper)."""
    _fields_ = [("loss_kind", C.c_int32), ("normalize_advantage", C.c_int32), ("clip_range", C.c_float), ("ent_coef", C.c_float),
                ("vf_coef", C.c_float)]


SAC_CRITIC, SAC_CRITIC_TARGET = 0, 1


class McgSac(C.Structure):
    """SAC's three blobs and shape (include/mcg.h: mcg_sac); the caller owns the blobs."""
    _fields_ = [("actor", C.c_void_p), ("critic", C.c_void_p), ("critic_target", C.c_void_p), ("n_envs", C.c_int32), ("obs_dim", C.c_int32),
                ("act_dim", C.c_int32), ("n_pi", C.c_int32), ("pi_width", C.c_int32 * 3), ("n_qf", C.c_int32), ("qf_width", C.c_int32 * 3),
                ("activation", C.c_int32), ("actor_floats", C.c_int64), ("critic_floats", C.c_int64)]


class McgSacActOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("action", "log_prob", "mean", "log_std", "noise")]


class McgSacRows(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("obs", "achieved", "desired", "action")]


class McgSacTargetOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("target", "next_action", "next_log_prob", "next_q", "noise")]


class McgSacActorGradOut(C.Structure):
    """The optional intermediates of the actor loss (include/mcg.h: mcg_sac_actor_grad_out)."""
    _fields_ = [(n, C.c_void_p) for n in ("action", "noise", "q_pi", "dq_da")]


TD3_CRITIC, TD3_CRITIC_TARGET = 0, 1


class McgTd3(C.Structure):
    """TD3's / DDPG's four blobs and shape (include/mcg.h: mcg_td3); the caller owns the blobs."""
    _fields_ = [("actor", C.c_void_p), ("actor_target", C.c_void_p), ("critic", C.c_void_p), ("critic_target", C.c_void_p),
                ("n_envs", C.c_int32), ("obs_dim", C.c_int32), ("act_dim", C.c_int32), ("n_pi", C.c_int32), ("pi_width", C.c_int32 * 3),
                ("n_qf", C.c_int32), ("qf_width", C.c_int32 * 3), ("activation", C.c_int32), ("n_critics", C.c_int32),
                ("actor_floats", C.c_int64), ("critic_floats", C.c_int64)]


class McgTd3ActOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("action", "mean", "noise")]


class McgTd3TargetOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("target", "next_action", "next_q", "noise")]


class McgTd3ActorGradOut(C.Structure):
    """The optional intermediates of the actor loss (include/mcg.h: mcg_td3_actor_grad_out)."""
    _fields_ = [(n, C.c_void_p) for n in ("action", "q_pi", "dq_da")]


CNN_UINT8, CNN_FLOAT32 = 0, 1          # mcg_cnn_obs.dtype


class McgCnnPolicy(C.Structure):
    """The CNN policy's weights, scratch and shape (include/mcg.h: mcg_cnn_policy); the caller owns the blob and the scratch."""
    _fields_ = [("blob", C.c_void_p), ("scratch", C.c_void_p), ("n_envs", C.c_int32), ("channels", C.c_int32), ("image_size", C.c_int32),
                ("features_dim", C.c_int32), ("act_dim", C.c_int32), ("blob_floats", C.c_int64), ("scratch_floats", C.c_int64)]


class McgCnnObs(C.Structure):
    """Pictures [rows, C, S, S] where they lie (include/mcg.h: mcg_cnn_obs); the strides are in elements."""
    _fields_ = [("pixels", C.c_void_p), ("dtype", C.c_int32), ("env_stride", C.c_int64), ("chan_stride", C.c_int64)]


class McgCnnOut(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("action", "value", "log_prob", "mean", "noise", "features")]


GEOM_SKY, GEOM_GROUND, GEOM_TABLE, GEOM_CUBE, GEOM_TARGET, GEOM_MESH0 = -1, 0, 1, 2, 3, 4      # mcg_render_out.geom

EXPORTS = ("mcg_abi_version", "mcg_last_error", "mcg_default_model", "mcg_create", "mcg_destroy", "mcg_obs_dim",
           "mcg_action_dim", "mcg_nq", "mcg_nv", "mcg_reset", "mcg_step", "mcg_get_state", "mcg_set_state",
           "mcg_compute_reward", "mcg_time_steps", "mcg_get_seed", "mcg_set_seed", "mcg_get_counters", "mcg_debug_contacts",
           "mcg_render", "mcg_render_mounted", "mcg_render_scenes", "mcg_scene_randomize",
           "mcg_her_record_bytes", "mcg_her_start", "mcg_her_add", "mcg_her_sample",
           "mcg_rollout_record_bytes", "mcg_rollout_start", "mcg_rollout_add", "mcg_rollout_gae", "mcg_rollout_gather",
           "mcg_rollout_img_record_bytes", "mcg_rollout_img_start", "mcg_rollout_img_add", "mcg_rollout_img_gae", "mcg_rollout_img_carry",
           "mcg_rollout_img_gather", "mcg_rollout_img_carry_stacked", "mcg_rollout_img_gather_stacked",
           "mcg_replay_img_record_bytes", "mcg_replay_img_start", "mcg_replay_img_add", "mcg_replay_img_sample",
           "mcg_replay_img_sample_stacked", "mcg_frame_stack_push",
           "mcg_policy_blob_floats", "mcg_policy_forward",
           "mcg_policy_evaluate", "mcg_policy_grad_work_floats", "mcg_policy_grad", "mcg_policy_adam",
           "mcg_sac_blob_floats", "mcg_sac_act", "mcg_sac_q", "mcg_sac_target", "mcg_sac_polyak",
           "mcg_sac_grad_work_floats", "mcg_sac_critic_grad", "mcg_sac_actor_grad", "mcg_sac_alpha_step", "mcg_sac_adam",
           "mcg_td3_blob_floats", "mcg_td3_act", "mcg_td3_q", "mcg_td3_target", "mcg_td3_polyak",
           "mcg_td3_grad_work_floats", "mcg_td3_critic_grad", "mcg_td3_actor_grad", "mcg_selftest_bad_value",
           "mcg_selftest_factor_h",
           "mcg_cnn_blob_floats", "mcg_cnn_scratch_floats", "mcg_cnn_forward", "mcg_cnn_evaluate")

_lib = None


class McgError(RuntimeError):
    pass


def load():
    """dlopen the in-tree library; raise if it has not been built (``python -c 'import __graft_entry__ as g; g.build()'``)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise McgError(f"{LIB_PATH} is missing: build it with __graft_entry__.build() "
                       "(hipcc --offload-arch=gfx950); this package has no CPU fallback")
    L = C.CDLL(LIB_PATH)
    L.mcg_abi_version.restype = C.c_int
    L.mcg_last_error.restype = C.c_char_p
    L.mcg_default_model.argtypes = [C.c_int, C.POINTER(McgModel)]
    L.mcg_create.argtypes = [C.POINTER(McgConfig), C.POINTER(McgModel), C.c_void_p, C.c_int64, C.c_int, C.POINTER(C.c_void_p)]
    L.mcg_destroy.argtypes = [C.c_void_p]
    L.mcg_destroy.restype = None
    for f in ("mcg_obs_dim", "mcg_action_dim", "mcg_nq", "mcg_nv"):
        getattr(L, f).argtypes = [C.c_void_p]
    L.mcg_reset.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_uint64, C.POINTER(McgStepOut), C.c_void_p]
    L.mcg_step.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(McgStepOut), C.c_void_p]
    L.mcg_get_state.argtypes = [C.c_void_p, C.POINTER(McgState), C.c_void_p]
    L.mcg_set_state.argtypes = [C.c_void_p, C.POINTER(McgState), C.c_void_p]
    L.mcg_compute_reward.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_double, C.c_void_p, C.c_void_p]
    if hasattr(L, "mcg_get_seed"):        # absent only from pre-v3 builds selected through MCG_LIB for A/B timing
        L.mcg_get_seed.argtypes = [C.c_void_p]; L.mcg_get_seed.restype = C.c_uint64
        L.mcg_set_seed.argtypes = [C.c_void_p, C.c_uint64]
    if hasattr(L, "mcg_get_counters"):    # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_get_counters.argtypes = [C.c_void_p, C.POINTER(McgCounters), C.c_int]
        L.mcg_debug_contacts.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.mcg_time_steps.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(McgStepOut), C.c_int, C.c_void_p, C.POINTER(C.c_float)]
    if hasattr(L, "mcg_render"):          # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_render.argtypes = [C.c_void_p, C.POINTER(McgScene), C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p,
                                 C.POINTER(McgRenderOut), C.c_void_p]
    if hasattr(L, "mcg_render_mounted"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_render_mounted.argtypes = [C.c_void_p, C.POINTER(McgScene), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                         C.c_void_p, C.POINTER(McgRenderOut), C.c_void_p]
    if hasattr(L, "mcg_render_scenes"):   # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_render_scenes.argtypes = [C.c_void_p, C.c_void_p, C.POINTER(d * 3), C.c_int, C.c_double, C.c_int, C.c_int, C.c_int, C.c_int,
                                        C.c_void_p, C.POINTER(McgRenderOut), C.c_void_p]
        L.mcg_scene_randomize.argtypes = [C.c_void_p, C.POINTER(McgScene), C.POINTER(McgSceneRand), C.c_int, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
    if hasattr(L, "mcg_her_sample"):      # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_her_record_bytes.argtypes = [C.c_int, C.c_int]; L.mcg_her_record_bytes.restype = C.c_int64
        L.mcg_her_start.argtypes = [C.POINTER(McgHerBuf), C.POINTER(McgStepOut), C.c_void_p, C.c_void_p]
        L.mcg_her_add.argtypes = [C.POINTER(McgHerBuf), C.c_int64, C.c_void_p, C.POINTER(McgStepOut), C.c_void_p]
        L.mcg_her_sample.argtypes = [C.POINTER(McgHerBuf), C.c_int64, C.c_uint64, C.c_uint64, C.c_int, C.c_int, C.POINTER(McgHerBatch),
                                     C.c_void_p]
    if hasattr(L, "mcg_rollout_gather"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_rollout_record_bytes.argtypes = [C.c_int, C.c_int]; L.mcg_rollout_record_bytes.restype = C.c_int64
        L.mcg_rollout_start.argtypes = [C.POINTER(McgRolloutBuf), C.POINTER(McgStepOut), C.c_void_p, C.c_void_p]
        L.mcg_rollout_add.argtypes = [C.POINTER(McgRolloutBuf), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(McgStepOut),
                                      C.c_void_p]
        L.mcg_rollout_gae.argtypes = [C.POINTER(McgRolloutBuf), C.c_void_p, C.c_void_p]
        L.mcg_rollout_gather.argtypes = [C.POINTER(McgRolloutBuf), C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.POINTER(McgRolloutBatch),
                                         C.c_void_p]
    if hasattr(L, "mcg_rollout_img_gather"):  # absent only from older builds selected through MCG_LIB for A/B timing
        img = C.POINTER(McgRolloutImgBuf)
        L.mcg_rollout_img_record_bytes.argtypes = [C.c_int]; L.mcg_rollout_img_record_bytes.restype = C.c_int64
        L.mcg_rollout_img_start.argtypes = [img, C.c_int, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.mcg_rollout_img_add.argtypes = [img, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                          C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcg_rollout_img_gae.argtypes = [img, C.c_void_p, C.c_void_p]
        L.mcg_rollout_img_carry.argtypes = [img, C.c_int, C.c_void_p]
        L.mcg_rollout_img_gather.argtypes = [img, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64, C.POINTER(McgRolloutImgBatch), C.c_void_p]
    if hasattr(L, "mcg_rollout_img_gather_stacked"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_rollout_img_carry_stacked.argtypes = [C.POINTER(McgRolloutImgBuf), C.c_int, C.c_int, C.c_void_p]
        L.mcg_rollout_img_gather_stacked.argtypes = [C.POINTER(McgRolloutImgBuf), C.c_int, C.c_uint64, C.c_uint64, C.c_int64, C.c_int64,
                                                     C.POINTER(McgRolloutImgBatch), C.c_void_p]
    if hasattr(L, "mcg_replay_img_sample"):  # absent only from older builds selected through MCG_LIB for A/B timing
        rimg = C.POINTER(McgReplayImgBuf)
        L.mcg_replay_img_record_bytes.argtypes = [C.c_int]; L.mcg_replay_img_record_bytes.restype = C.c_int64
        L.mcg_replay_img_start.argtypes = [rimg, C.c_int64, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p]
        L.mcg_replay_img_add.argtypes = [rimg, C.c_int64, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_int64, C.c_int64,
                                         C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcg_replay_img_sample.argtypes = [rimg, C.c_int64, C.c_uint64, C.c_uint64, C.c_int, C.POINTER(McgReplayImgBatch), C.c_void_p]
    if hasattr(L, "mcg_frame_stack_push"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_replay_img_sample_stacked.argtypes = [C.POINTER(McgReplayImgBuf), C.c_int64, C.c_uint64, C.c_uint64, C.c_int, C.c_int,
                                                    C.POINTER(McgReplayImgBatch), C.c_void_p]
        L.mcg_frame_stack_push.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int64, C.c_int64,
                                           C.c_void_p, C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "mcg_policy_forward"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_policy_blob_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32)]
        L.mcg_policy_blob_floats.restype = C.c_int64
        L.mcg_policy_forward.argtypes = [C.POINTER(McgPolicy), C.POINTER(McgStepOut), C.c_uint64, C.c_uint64, C.c_int64, C.c_int,
                                         C.POINTER(McgPolicyOut), C.c_void_p]
    if hasattr(L, "mcg_policy_grad"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_policy_evaluate.argtypes = [C.POINTER(McgPolicy), C.POINTER(McgRolloutBatch), C.c_int64, C.POINTER(McgPolicyEvalOut), C.c_void_p]
        L.mcg_policy_grad_work_floats.argtypes = [C.POINTER(McgPolicy), C.c_int64]
        L.mcg_policy_grad_work_floats.restype = C.c_int64
        L.mcg_policy_grad.argtypes = [C.POINTER(McgPolicy), C.POINTER(McgRolloutBatch), C.c_int64, C.POINTER(McgPolicyHyper), C.c_void_p,
                                      C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcg_policy_adam.argtypes = [C.POINTER(McgPolicy), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, d, d, d, d, d, C.c_void_p,
                                      C.c_void_p]
    if hasattr(L, "mcg_sac_target"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_sac_blob_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64)]
        L.mcg_sac_blob_floats.restype = C.c_int64
        L.mcg_sac_act.argtypes = [C.POINTER(McgSac), C.POINTER(McgStepOut), C.c_uint64, C.c_uint64, C.c_int64, C.c_int, C.POINTER(McgSacActOut),
                                  C.c_void_p]
        L.mcg_sac_q.argtypes = [C.POINTER(McgSac), C.c_int, C.POINTER(McgSacRows), C.c_int64, C.c_void_p, C.c_void_p]
        L.mcg_sac_target.argtypes = [C.POINTER(McgSac), C.POINTER(McgHerBatch), C.c_int64, C.c_uint64, C.c_uint64, C.c_float, C.c_float,
                                     C.c_void_p, C.POINTER(McgSacTargetOut), C.c_void_p]
        L.mcg_sac_polyak.argtypes = [C.POINTER(McgSac), d, C.c_void_p]
    if hasattr(L, "mcg_sac_actor_grad"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_sac_grad_work_floats.argtypes = [C.POINTER(McgSac), C.c_int64]
        L.mcg_sac_grad_work_floats.restype = C.c_int64
        L.mcg_sac_critic_grad.argtypes = [C.POINTER(McgSac), C.POINTER(McgSacRows), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
        L.mcg_sac_actor_grad.argtypes = [C.POINTER(McgSac), C.POINTER(McgSacRows), C.c_int64, C.c_uint64, C.c_uint64, C.c_float, C.c_void_p,
                                         C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(McgSacActorGradOut), C.c_void_p]
        L.mcg_sac_alpha_step.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int64, d, d, d, d,
                                         C.c_void_p, C.c_void_p, C.c_void_p]
        L.mcg_sac_adam.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, d, d, d, d, C.c_void_p]
    if hasattr(L, "mcg_selftest_bad_value"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_selftest_bad_value.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(L, "mcg_selftest_factor_h"):  # likewise
        L.mcg_selftest_factor_h.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
    if hasattr(L, "mcg_td3_actor_grad"):  # absent only from older builds selected through MCG_LIB for A/B timing
        td3 = C.POINTER(McgTd3)
        L.mcg_td3_blob_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.POINTER(C.c_int32), C.c_int, C.POINTER(C.c_int32), C.c_int,
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
        L.mcg_td3_blob_floats.restype = C.c_int64
        L.mcg_td3_act.argtypes = [td3, C.POINTER(McgStepOut), C.c_uint64, C.c_uint64, C.c_int64, C.c_float, C.POINTER(McgTd3ActOut), C.c_void_p]
        L.mcg_td3_q.argtypes = [td3, C.c_int, C.POINTER(McgSacRows), C.c_int64, C.c_void_p, C.c_void_p]
        L.mcg_td3_target.argtypes = [td3, C.POINTER(McgHerBatch), C.c_int64, C.c_uint64, C.c_uint64, C.c_float, C.c_float, C.c_float,
                                     C.POINTER(McgTd3TargetOut), C.c_void_p]
        L.mcg_td3_polyak.argtypes = [td3, d, C.c_void_p]
        L.mcg_td3_grad_work_floats.argtypes = [td3, C.c_int64]
        L.mcg_td3_grad_work_floats.restype = C.c_int64
        L.mcg_td3_critic_grad.argtypes = [td3, C.POINTER(McgSacRows), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                          C.c_void_p]
        L.mcg_td3_actor_grad.argtypes = [td3, C.POINTER(McgSacRows), C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p,
                                         C.POINTER(McgTd3ActorGradOut), C.c_void_p]
    if hasattr(L, "mcg_cnn_forward"):  # absent only from older builds selected through MCG_LIB for A/B timing
        L.mcg_cnn_blob_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int]
        L.mcg_cnn_blob_floats.restype = C.c_int64
        L.mcg_cnn_scratch_floats.argtypes = [C.c_int, C.c_int, C.c_int, C.c_int, C.c_int64]
        L.mcg_cnn_scratch_floats.restype = C.c_int64
        L.mcg_cnn_forward.argtypes = [C.POINTER(McgCnnPolicy), C.POINTER(McgCnnObs), C.c_uint64, C.c_uint64, C.c_int64, C.c_int,
                                      C.POINTER(McgCnnOut), C.c_void_p]
        L.mcg_cnn_evaluate.argtypes = [C.POINTER(McgCnnPolicy), C.POINTER(McgCnnObs), C.c_void_p, C.c_int64, C.POINTER(McgPolicyEvalOut),
                                       C.c_void_p]
    _lib = L
    return L


def check(code: int, what: str = ""):
    if code != MCG_OK:
        msg = load().mcg_last_error().decode(errors="replace")
        raise McgError(f"{what} failed (code {code}): {msg}")
