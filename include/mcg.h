/*
 * mcg.h -- C ABI of the MI355X rollout engine for the MyCobotGym step()/reset() hot path.
 *
 * The reference has no FFI of its own: its hot path is MuJoCo driven from Python through the
 * Gymnasium Env protocol.  Each entry point below replaces one reference interface, batched over
 * N environments (citations relative to /root/reference):
 *
 *   mcg_create          MyCobotEnv.__init__ + _env_setup         mycobotgym/envs/mycobot.py:30-115, 450-481
 *                       (MuJoCo model compile is replaced by the precompiled mcg_model block)
 *   mcg_reset           MyCobotEnv.reset / reset_model / _sample_goal   mycobot.py:506-514, 207-243
 *   mcg_step            MyCobotEnv.step (controller branch joint | IK | mocap -> mujoco.mj_step x frame_skip -> _get_obs ->
 *                       _is_success / compute_reward / compute_terminated / compute_truncated)
 *                       mycobot.py:132-205, 245-298, 342-400; IKController mycobotgym/utils.py:499-556;
 *                       TimeLimit(50) from the registration mycobotgym/__init__.py:34; auto-reset as in
 *                       gymnasium.vector (info["final_observation"]) / SB3 VecEnv used by scripts/train.py:80-85
 *   mcg_compute_reward  MyCobotEnv.compute_reward on batched goals (HER)   mycobot.py:289-298, utils.py:24-26
 *   mcg_her_start / mcg_her_add / mcg_her_sample   SB3's HerReplayBuffer as the reference configures it (n_sampled_goal = 4, strategy
 *                       "future")   scripts/train.py:89-97
 *   mcg_rollout_start / mcg_rollout_add / mcg_rollout_gae / mcg_rollout_gather   SB3's RolloutBuffer as PPO / A2C use it (n_steps,
 *                       gamma, gae_lambda)   scripts/train.py:99-101
 *   mcg_rollout_img_start / _add / _gae / _carry / _gather   the same RolloutBuffer on the uint8 pictures MyCobotImgEnv observes
 *                       (PPO / A2C on the -v1 ids)   scripts/train.py:99-101, mycobot.py:517-545
 *   mcg_replay_img_start / _add / _sample   SB3's ReplayBuffer as SAC / TD3 / DDPG use it (scripts/train.py:62, 102-104) on the same
 *                       pictures, every picture stored once and a time-limit end kept apart from a termination
 *   mcg_replay_img_sample_stacked, mcg_frame_stack_push   SB3's VecFrameStack on those pictures: stacks rebuilt from the single-frame
 *                       ring when a batch is sampled, and the stack a policy acts on, updated in one launch per step
 *   mcg_rollout_img_carry_stacked / _gather_stacked   the same stacks for the on-policy buffer, rebuilt from its single stored frames
 *   mcg_get_state / mcg_set_state   direct access to data.qpos/qvel/ctrl/qacc_warmstart (set_joint_qpos etc.)
 *
 * Conventions: every pointer in the step/reset/state calls is DEVICE memory owned by the caller;
 * the engine owns its struct-of-arrays state.  Calls enqueue work on `stream` (a hipStream_t passed
 * as void*, NULL = default stream) and return without synchronising.  Return 0 = OK, otherwise an
 * MCG_ERR_* code with text in mcg_last_error().  A handle is bound to one device and is not
 * thread-safe; distinct handles are independent.  There is no CPU fallback: without a HIP device
 * mcg_create fails.
 */
#ifndef MCG_H
#define MCG_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MCG_ABI_VERSION 8
#define MCG_MAXCON 16          /* entries of an environment's contact list (MuJoCo has no cap; see mcg_counters.contacts_dropped) */
#define MCG_NMESH 14           /* collision polytopes of the mesh geoms */

enum { MCG_OK = 0, MCG_ERR_ARG = 1, MCG_ERR_HIP = 2, MCG_ERR_UNSUPPORTED = 3 };
enum { MCG_CTRL_JOINT = 0, MCG_CTRL_IK = 1, MCG_CTRL_MOCAP = 2 };   /* controller_type "joint" | "IK" | "mocap" */
enum { MCG_REWARD_SPARSE = 0, MCG_REWARD_DENSE = 1, MCG_REWARD_SHAPING = 2 };

/* Numeric model block (produced by mycobotgym_amd/model/specialize.py from the compiled MJCF).
   13 bodies: link1..6, right gear/finger, left gear/finger, right/left hinge, cube. */
typedef struct mcg_body {          /* 16 doubles = 128 B: one body's constants, contiguous for wide scalar loads */
  double r[3];                      /* body origin in its parent's frame */
  double mass, mc[3];               /* mass, mass * centre of mass (body frame, about the origin) */
  double inertia[6];                /* xx yy zz xy xz yz about the body origin */
  double armature, damping;         /* of the body's hinge (cube: unused, see cube_damping) */
  double hull_rad;                  /* robot bodies: largest distance from the body origin to a vertex of the mesh polytopes riding on it */
} mcg_body;

typedef struct mcg_model {
  double timestep;
  double base_pos[3], base_mat[9], gravity_base[3];
  mcg_body body[13];
  double cube_damping[6];
  double jnt_range[12][2];
  double limit_par[12][10];         /* K B d0 dmax width midpoint power 1/width 1/mid^(p-1) 1/(1-mid)^(p-1); refsafe applied */
  double limit_diag[12];            /* dof_invweight0 */
  double eq_anchor1[2][3], eq_anchor2[2][3];
  double eq_par[3][10], eq_diag[3];  /* connect right, connect left, joint coupling */
  double act_gain[7], act_bias[7][3], act_ctrlrange[7][2], act_forcerange[7][2], tendon_coef[2];
  double site_eef[3];               /* EEF site in the link6 frame */
  /* PickAndPlace only */
  double cube_half[3], table_pos[3], table_half[3], pad_box[2][6];
  double contact_par[7][15];        /* table-cube, right pad-cube, left pad-cube, table-right pad, table-left pad, table-mesh (condim 3),
                                       mesh-cube: the 10 solver numbers | friction[5].  The ground plane carries the table's
                                       (default) parameters; all mesh geoms are default geoms (asserted when the block is made). */
  double contact_diag[5][2];        /* summed body_invweight0 (translational, rotational) of the first five pairs */
  /* Convex-mesh collision (mycobot280_main.xml:105-247): the fourteen mesh geoms of the arm and the gripper -- link1..link6,
     flange, gripper_base, right gear / finger link, left gear / finger link, right / left hinge link -- against the ground plane, the
     table and the cube, on each mesh's collision polytope (within 1 mm of its convex hull; mycobotgym_amd/model/polytope.py), by an
     exact separating-axis test, one contact per pair (csrc/mcg_mesh.hpp).  The polytopes' vertex / face / edge tables are a separate
     block (mcg_create: `polytopes`). */
  double mesh_box[MCG_NMESH][6];    /* centre and half extents of the polytope's bounding box in the frame of the robot body it rides on
                                       (polytope m on body m for m < 6; flange, gripper_base on 5; then bodies 6..11): broad phase */
  double mesh_mult;                 /* identical colliding geoms per mesh (the reference attaches every mesh twice: 2) */
  double mesh_fric;                 /* the mesh geoms' own sliding friction (the cube's is re-scaled under domain randomisation, a pair
                                       takes the larger) */
  double pair_tran[5 + 2 * MCG_NMESH];   /* per pair type (csrc/mcg_cube.hpp: 0 static-cube, 1 / 2 pad-cube, 3 / 4 static-pad, 5 + m static-mesh m,
                                       19 + m mesh m-cube) the summed translational body_invweight0 of the two geoms' bodies */
  double geom_friction0[3];         /* sliding friction of the table, pad and cube geoms (re-mixed under domain randomisation) */
  /* mocap variant only (mycobot280_mocap.xml): weld between the mocap body and gripper_tcp */
  double base_quat[4];              /* orientation of the arm's base body: start of the xquat chain */
  double weld_on;                   /* 1 = the model carries the weld (and no arm actuators) */
  double weld_par[10];              /* solver numbers as in limit_par */
  double weld_diag[2];              /* diagApprox of the translational rows 0-2 and of the rotational rows 3-5.  Built-in models: the
                                       same (translational) weight on all six, which is what the reference's mocap keyframe supports
                                       (oracle/RULE_STUDY.md, K2); mj_diagApprox as recalled puts the rotational inverse weight on
                                       rows 3-5: specialize(..., weld_rule="mujoco") / MyCobotVecEnv(weld_rule="mujoco") */
  double weld_anchor[3];            /* weld point on the robot, link6 frame */
  double weld_relpos[3], weld_relquat[4], weld_torquescale;
  double target0[3];                /* MJCF position of site `target0`: what stage_rewards reads unless rendering (mycobot.py:422, 309-311) */
  double contact_rpy;               /* regulariser of a contact's pyramid rows, Rpy = contact_rpy * mu^2 * R(normal row).  2 = the rule as
                                       recalled from MuJoCo (built-in models); 4 = the one single change that reproduces the cube's rest
                                       height in the reference's keyframes (penetration 1.9e-5, mycobot280.xml:6; oracle/RULE_STUDY.md K1):
                                       specialize(..., contact_rule="keyframe") / MyCobotVecEnv(contact_rule="keyframe") */
} mcg_model;

typedef struct mcg_config {
  int32_t n_envs;
  int32_t has_object;          /* 0 = Reach, 1 = PickAndPlace                       (mycobot.py:33).  Reach with reward_type =
                                  MCG_REWARD_SHAPING keeps the cube as a hidden free body (geom and site size zero,
                                  mycobot.py:475-481): stage_rewards reads its site and contacts (mycobot.py:402-448) */
  int32_t controller;          /* MCG_CTRL_*                                       (mycobot.py:36) */
  int32_t fetch_env;           /*                                                  (mycobot.py:41) */
  int32_t reward_type;         /* MCG_REWARD_*                                     (mycobot.py:42) */
  int32_t frame_skip;          /* 20                                               (mycobot.py:43) */
  int32_t control_steps;       /* 5, IK only                                       (mycobot.py:35) */
  int32_t max_episode_steps;   /* 50, TimeLimit                                    (__init__.py:34) */
  int32_t target_in_the_air;   /*                                                  (mycobot.py:38) */
  int32_t auto_reset;          /* reset finished envs inside mcg_step */
  int32_t dr_enable;           /* per-reset domain randomisation (build-defined) */
  int32_t block_gripper;       /* zero the two finger joints after every step      (mycobot.py:34,300-306) */
  double distance_threshold;   /* 0.01                                             (mycobot.py:39) */
  double height_offset;        /* z of site object0 at the initial state           (mycobot.py:470-472) */
  double initial_gripper_xpos[3];   /* EEF site at the initial state               (mycobot.py:464-466) */
  double init_qpos[19], init_qvel[18], init_ctrl[7];   /* snapshot restored by reset (mycobot.py:80-82) */
  double dr_mass_range[2], dr_friction_range[2];
  uint64_t seed;
  int64_t env_id_offset;       /* global id of env 0 of this handle: RNG streams are keyed by global id */
} mcg_config;

/* Output block of mcg_step / mcg_reset; all device pointers, any may be NULL to skip.  D = mcg_obs_dim. */
typedef struct mcg_step_out {
  double* obs;            /* [N, D]  "observation" (after auto-reset where done) */
  double* achieved_goal;  /* [N, 3] */
  double* desired_goal;   /* [N, 3] */
  double* reward;         /* [N]     dense: -d (f64); sparse: -(d > thr) as in the reference's float32 */
  uint8_t* terminated;    /* [N] */
  uint8_t* truncated;     /* [N]     is_success | elapsed >= max_episode_steps */
  uint8_t* is_success;    /* [N] */
  double* final_obs;      /* [N, D]  pre-reset observation, valid where terminated|truncated */
  double* final_achieved; /* [N, 3] */
  double* final_desired;  /* [N, 3] */
  double* ep_return;      /* [N]     running episode return (Monitor's "r" where done) */
  int32_t* ep_length;     /* [N]     running episode length (Monitor's "l" where done) */
} mcg_step_out;

/* State arrays are struct-of-arrays [dim, N] (N fastest), the engine's native layout. */
typedef struct mcg_state {
  double* qpos;      /* [nq, N]   nq = 12 (Reach) | 19 (PickAndPlace) */
  double* qvel;      /* [nv, N]   nv = 12 | 18 */
  double* ctrl;      /* [7, N] */
  double* warm;      /* [nv, N]   qacc_warmstart */
  double* qpos_lag;  /* [nq, N]   qpos of the last forward pass: observations lag one sub-step (SURVEY D-1) */
  double* goal;      /* [3, N] */
  int32_t* elapsed;  /* [N] */
  int32_t* episode;  /* [N]       per-env episode counter (RNG stream position) */
  double* dr_scale;  /* [2, N]    domain-randomisation scales of the current episode: cube mass, sliding friction */
  double* ep_return; /* [N]       running return of the episode in flight (Monitor's "r" when it ends) */
  int32_t* ep_length;/* [N]       running length of the episode in flight (Monitor's "l") */
} mcg_state;

/* Event counters since mcg_create (or the last clearing read).  The first two are this engine's own bounds on things the reference
   leaves unbounded; none of them is expected to move in ordinary use. */
typedef struct mcg_counters {
  uint64_t reset_cap_hits;          /* a rejection loop of reset_model (mycobot.py:218-219, 232-233: unbounded `while`) gave up after 1000 draws */
  uint64_t bad_state_resets;        /* mj_checkPos / mj_checkVel / mj_checkAcc fired: a body's state was reset (per body, per event) */
  uint64_t contacts_dropped;        /* contacts cut off by the build's cap of MCG_MAXCON list entries per environment (MuJoCo has no such cap) */
  uint64_t coupled_env_substeps;    /* environment-sub-steps routed through the cooperative robot + cube solve (a contact reached the robot) */
} mcg_counters;

typedef struct mcg_env mcg_env;

int mcg_abi_version(void);
const char* mcg_last_error(void);
/* built-in model blocks: 0 = legacy mesh inertia (default), 1 = exact mesh inertia; 2, 3 = the same for the mocap variant */
int mcg_default_model(int variant, mcg_model* out);

/* polytopes: the mesh geoms' collision tables in the robot bodies' frames (layout: mycobotgym_amd/model/polytope.py: pack), n_polytopes
   doubles, host memory; NULL = the built-in tables of the reference's meshes.  A custom model goes with the block specialised with it
   (the polytopes move with the bodies they ride on).  With the cube in the physics (PickAndPlace, or Reach with reward_shaping) these
   are checked on the host, before any HIP call:
     MCG_ERR_ARG          the block's index: per mesh, all eight meta entries whole numbers in [0, n_polytopes], V >= 1, F, E >= 0,
                          Vpad, Fpad, Epad multiples of 64 with Fpad, Epad >= 64, counts within their pads, the arrays after the meta
                          region and inside the block;
     MCG_ERR_ARG          the block against the model: every vertex of mesh m inside mesh_box[m] and within body[].hull_rad of the body
                          it rides on (1e-12 slack);
     MCG_ERR_UNSUPPORTED  the model against the broad-phase gates of the kernels (csrc/mcg_cube.hpp: GATE_*): the gripper's reach from
                          the link6 origin (|r| summed along each chain plus hull_rad, or plus the pad's centre and half-diagonal) below
                          0.17 m, that reach plus |cube_half| below 0.2 m, each pad's half-diagonal below 0.02 m, |cube_half| below 0.05 m.
                          The message names the gate. */
int mcg_create(const mcg_config* cfg, const mcg_model* model /* NULL = variant 0 */, const double* polytopes, int64_t n_polytopes,
               int device, mcg_env** out);
void mcg_destroy(mcg_env* env);
int mcg_obs_dim(const mcg_env* env);
int mcg_action_dim(const mcg_env* env);
int mcg_nq(const mcg_env* env);
int mcg_nv(const mcg_env* env);

int mcg_reset(mcg_env* env, const uint8_t* mask /* [N] device or NULL = all */, int reseed, uint64_t seed,
              const mcg_step_out* out, void* stream);
int mcg_step(mcg_env* env, const float* actions /* [N, A] row-major, device */, const mcg_step_out* out, void* stream);
int mcg_get_state(mcg_env* env, const mcg_state* dst, void* stream);
int mcg_set_state(mcg_env* env, const mcg_state* src, void* stream);
/* base seed of the reset / domain-randomisation streams (changed by mcg_reset with reseed != 0): part of a checkpoint */
uint64_t mcg_get_seed(const mcg_env* env);
int mcg_set_seed(mcg_env* env, uint64_t seed);
int mcg_compute_reward(const double* achieved /* [n,3] device */, const double* desired, int n, int reward_type,
                       double threshold, double* out, void* stream);

/* Synchronises the device; copies the counters to host memory `out`; clears them when `clear` != 0. */
int mcg_get_counters(mcg_env* env, mcg_counters* out, int clear);

/* TEST / DEBUG: the collision pass (mj_collision restated, P4) of PickAndPlace on the CURRENT state, exported as the kernels see it.
   All device pointers.  count [N]: list entries; dropped [N]: contacts cut by the cap (or NULL); data [N, MCG_MAXCON, 10]: per entry dist,
   pos[3] (midpoint between the surfaces), normal[3] (geom1 -> geom2), pair type (csrc/mcg_cube.hpp PAIR_*), multiplicity (identical
   geoms the entry stands for), D (weight of its pyramid rows). */
int mcg_debug_contacts(mcg_env* env, int32_t* count, int32_t* dropped, double* data, void* stream);

/* Live timing of the step kernel on its own stream with HIP events (used by bench.py's roofline leg). */
int mcg_time_steps(mcg_env* env, const float* actions, const mcg_step_out* out, int steps, void* stream, float* ms_total);

/* ---- Rendering (MyCobotImgEnv / render(): mycobot.py:308-311, 517-545; cameras, light, colours: mycobot280_main.xml:7, 78-102, 258-268).
   A ray caster over the engine's own state: the ground plane, the table, cube and target boxes, and the fourteen mesh geoms as their
   collision polytopes (face planes, within 1 mm of the convex hulls).  Flat Lambert shading per face:
     rgb * (ambient + diffuse * max(0, n.(-light_dir)) + head_ambient + head_diffuse * max(0, n.(-ray))), clamped, to uint8 by round-half-up.
   Not drawn: base_link, the finger pads, the mocap body's guide geoms, the EEF site, specular light, the visual meshes' concavities.
   Visibility: surfaces are one-sided.  A convex geom whose entry point lies behind the camera or before the near plane is invisible
   along that ray, which goes on to the other geoms; so a camera inside a polytope does not see it (OpenGL's back-face culling on closed
   convex solids).  The reference's gripper camera (mycobot280_main.xml:161-166) sits inside the flange's polytope and looks out of it. */
typedef struct mcg_scene {   /* one camera + light + colours; all doubles */
  double cam_pos[3];         /* world position of the camera */
  double cam_mat[9];         /* row-major world <- camera; columns = the camera's x (right), y (up), z; it looks along -z */
  double fovy;               /* vertical field of view, degrees, in (0, 180) */
  double light_dir[3];       /* directional light: direction of travel (unit) */
  double light_ambient, light_diffuse;
  double head_ambient, head_diffuse;     /* headlight: travels along the ray */
  double rgb_ground[3], rgb_table[3], rgb_cube[3], rgb_target[3], rgb_mesh[3], rgb_sky[3];     /* in [0, 1] */
  double target_half[3];     /* half sizes of the target site's (world-aligned) box */
} mcg_scene;

typedef struct mcg_render_out {      /* device pointers, any may be NULL (not all) */
  uint8_t* rgb;    /* [N, H, W, 3] */
  uint8_t* gray;   /* [N, H, W]    0.114 R + 0.587 G + 0.299 B per sample (the reference's BGR2GRAY on an RGB frame, utils.py:591), box average */
  float*   depth;  /* [N, H, W]    distance along the camera's -z of the pixel-centre ray's hit; +inf = sky */
  int8_t*  geom;   /* [N, H, W]    -1 sky, 0 ground, 1 table, 2 cube, 3 target, 4 + m = mesh m (MCG_NMESH) */
} mcg_render_out;

/* Draws every environment (mask: those with a non-zero byte; the others' images are left untouched) as the given camera sees it.
   samples: s x s rays per pixel on a regular sub-grid, box-averaged (rgb, gray); depth and geom always come from the pixel-centre ray.
   target_at_goal != 0: the target box sits at the environment's goal (render(), mycobot.py:308-311), otherwise at mcg_model.target0
   (what the reference's image observations show).  The cube is drawn where it is visible in the reference: has_object only.
   Enqueues on `stream`, does not synchronise (but for an engine's first call, which uploads the face tables with a blocking copy: draw once
   before capturing a graph), writes no engine state.  Checked on the host before any HIP call (MCG_ERR_ARG): null
   handle / scene / out, all four outputs null, width or height outside 1..512, samples outside 1..4, cam_mat not orthonormal to
   1e-9, fovy outside (0, 180), a light_dir that is not a unit vector to 1e-9.  MCG_ERR_UNSUPPORTED: an engine created from a
   caller's model without a polytope block (its meshes are unknown). */
int mcg_render(mcg_env* env, const mcg_scene* scene, int width, int height, int samples, int target_at_goal,
               const uint8_t* mask /* [N] device or NULL = all */, const mcg_render_out* out, void* stream);

/* mcg_render with a camera that rides on a body and a near plane: scene->cam_pos and scene->cam_mat are read in the frame of engine body
   `body` (0..11 in the order of mcg_model.body; a body without a joint of its own, such as `flange`, is welded into its jointed
   ancestor: compose its offset into cam_pos / cam_mat, as tools/compile_scene.py does for scene["body_cameras"]), and the camera's
   world pose is composed per environment, in float64, from that body's pose in the environment's state.  body == -1: the world, which
   is mcg_render's meaning.  znear (metres): a hit of any geom whose depth along the camera's -z is below it is dropped for that ray,
   which goes on to the other geoms; 0 = no near plane.  mcg_render is this entry with body = -1, znear = 0.  Host checks as
   mcg_render's, plus (MCG_ERR_ARG): body outside -1..11, znear negative or not finite. */
int mcg_render_mounted(mcg_env* env, const mcg_scene* scene, int body, double znear, int width, int height, int samples,
                       int target_at_goal, const uint8_t* mask /* [N] device or NULL = all */, const mcg_render_out* out, void* stream);

/* ---- Per-environment scenes: camera, light and colours from a device table with one row per environment.
   A scene table is a device array double [N, MCG_SCENE_ENV_DOUBLES], row-major.  A row is the head of mcg_scene, in its order: */
#define MCG_SCENE_ENV_DOUBLES 40
#define MCG_SCENE_CAM_POS 0          /* [3]  in the carrier's frame: the world, or the engine body the camera rides on */
#define MCG_SCENE_CAM_MAT 3          /* [9]  row-major carrier <- camera, as mcg_scene.cam_mat */
#define MCG_SCENE_FOVY 12            /*      degrees */
#define MCG_SCENE_LIGHT_DIR 13       /* [3]  unit */
#define MCG_SCENE_LIGHT_AMBIENT 16
#define MCG_SCENE_LIGHT_DIFFUSE 17
#define MCG_SCENE_HEAD_AMBIENT 18
#define MCG_SCENE_HEAD_DIFFUSE 19
#define MCG_SCENE_RGB 20             /* [6][3] ground, table, cube, target, mesh, sky, each in [0, 1] */
#define MCG_SCENE_PAD 38             /* [2]  zero */
#define MCG_SCENE_RAND_CAM_SLOTS 8

/* mcg_render_mounted with environment e's camera, fovy, light, shading coefficients and colours taken from row e of `scenes`; `body`,
   `znear` and `target_half` are per call (all rows of one call describe the same named camera).  Host checks as mcg_render_mounted's
   (those of the scene's values excepted: the rows are device memory), plus a null table or target_half (MCG_ERR_ARG); before any HIP
   call.  The values of a row cannot be checked on the host: the kernel is safe for any bit pattern in a row -- no address and no loop
   bound depends on one -- and a bad row gives a bad picture of that environment and nothing else. */
int mcg_render_scenes(mcg_env* env, const double* scenes /* device [N, MCG_SCENE_ENV_DOUBLES] */, const double target_half[3], int body,
                      double znear, int width, int height, int samples, int target_at_goal,
                      const uint8_t* mask /* [N] device or NULL = all */, const mcg_render_out* out, void* stream);

/* Ranges of mcg_scene_randomize; all doubles.  A half range h draws from [-h, h]; a scale pair draws from [lo, hi]. */
typedef struct mcg_scene_rand {
  double cam_pos[3];                 /* half ranges, metres, in the carrier's frame */
  double cam_rot[3];                 /* half ranges of a rotation vector, radians */
  double fovy_scale[2];
  double light_tilt;                 /* largest tilt of the light's direction, radians, in [0, pi] */
  double light_ambient_scale[2];
  double light_diffuse_scale[2];
  double head_scale[2];              /* one factor for both headlight terms */
  double rgb[6];                     /* half range per colour class (ground, table, cube, target, mesh, sky), the same for its three channels */
} mcg_scene_rand;

/* Fills the rows of `scenes` (where mask is non-zero; the others are left as they are) with the base scene jittered per environment and
   per episode.  Uniforms: Philox4x32-10 keyed as every reset draw, by (seed, global environment id, episode, draw index), stream 2
   (0: goals, 1: mass and friction), the episode being the state's counter at the time of the call; so a table is a function of the
   state, does not depend on how environments are split over engines, and need not be checkpointed.  Draw d gives the pair (u0, u1);
   a mapped value is fma(hi - lo, u, lo).
     world block (the same for every camera of an environment)
       0      tilt = light_tilt * sqrt(u0), azimuth = 2 pi u1: light_dir = cos(tilt) d0 + sin(tilt) (cos(az) e1 + sin(az) e2),
              e1 = normalize(x^ x d0) (y^ for x^ where |d0.x| > 0.9), e2 = d0 x e1
       1      light_ambient scale, light_diffuse scale
       2      headlight scale (both terms), -
       3 + k  colour channels 2k and 2k + 1 of the row's 18 (k = 0..8): base + offset, clamped to [0, 1]
     camera block, draw 32 + 4 * cam_slot + ...
       0      dx, dy;  1  dz, fovy scale;  2  w_x, w_y;  3  w_z, -
       cam_pos = base + d; cam_mat = R(w) base, R(w) = I + a K + b K^2, K = [w]x, a = sin|w| / |w|, b = (1 - cos|w|) / |w|^2
       (a = 1, b = 1/2 below |w| = 1e-12); scales multiply the base's value.
   A zero offset, a zero tilt and a zero rotation vector leave the base's values as they are, signed zeros included: with all half
   ranges zero and all scales [1, 1] a row is the base scene bit for bit.  Host checks, before any HIP call (MCG_ERR_ARG):
   null handle / base / ranges / scenes, cam_slot outside 0..7, a range negative or not finite, a scale pair with lo <= 0 or lo > hi,
   base.fovy * fovy_scale[1] >= 180, light_tilt outside [0, pi], a base that fails mcg_render's checks of a scene. */
int mcg_scene_randomize(mcg_env* env, const mcg_scene* base, const mcg_scene_rand* ranges, int cam_slot /* 0..7 */,
                        const uint8_t* mask /* [N] device or NULL = all */, double* scenes /* device [N, MCG_SCENE_ENV_DOUBLES], out */,
                        void* stream);

/* ---- Hindsight replay buffer (SB3's HerReplayBuffer as scripts/train.py:89-97 uses it: goal_selection_strategy "future", on the
   engine's N lockstep environments).  Stateless on the C side: the caller owns all device memory and passes it per call; there is no
   handle.  The ring is time-major [capacity, N]: every environment writes slot pos = n_written % capacity on the same call, so
   n_written is a host integer and no call synchronises.  One record per (slot, env), mcg_her_record_bytes(D, A) bytes, contiguous:
     byte 0            double achieved[3], next_achieved[3], desired[3]     (float64: a recomputed reward is the engine's own number)
     byte 72           float  obs[D], next_obs[D], action[A], reward
     then              int32  t_in_ep   step index inside its episode (saturates at max_episode_steps in an over-long episode)
                       int32  ep_len    0 while the episode is in flight (or abandoned), back-filled into all its slots when it ends
                       uint8  terminated, 3 bytes zero
     zero padding to a multiple of 16 bytes.
   An episode is abandoned -- its slots keep ep_len 0 and are never sampled -- by mcg_her_start while it is in flight, or when it runs to
   max_episode_steps transitions without a done flag (a caller error; counted in counters[1]). */
typedef struct mcg_her_buf {        /* device pointers the caller owns, and the buffer's shape */
  void* records;                    /* [capacity, N] records; zero before the first call; 16-byte aligned */
  int32_t* t_run;                   /* [N]     transitions of the episode in flight */
  float* last_obs;                  /* [N, D]  observation the next transition starts from */
  double* last_achieved;            /* [N, 3] */
  uint64_t* counters;               /* [2]     samples that gave up (no valid transition in 256 draws), over-long episodes */
  int32_t n_envs, obs_dim, act_dim;
  int32_t capacity;                 /* slots; >= 2 * max_episode_steps: an episode must not overlap itself in the ring */
  int32_t max_episode_steps;        /* bound of every episode length, and of every loop over one */
  int32_t reward_type;              /* MCG_REWARD_*: how a relabelled reward is recomputed */
  double distance_threshold;
} mcg_her_buf;

typedef struct mcg_her_batch {      /* outputs of mcg_her_sample; device pointers, float32, any may be NULL.  B = batch */
  float* obs;            /* [B, D] */
  float* achieved;       /* [B, 3] */
  float* desired;        /* [B, 3]  also the next observation's desired goal; relabelled in a virtual sample */
  float* next_obs;       /* [B, D] */
  float* next_achieved;  /* [B, 3] */
  float* action;         /* [B, A] */
  float* reward;         /* [B]     stored (real sample) or recomputed under the new goal (virtual sample) */
  float* done;           /* [B]     the stored `terminated` (SB3's dones * (1 - timeouts)); not recomputed under the new goal */
  int32_t* index;        /* [B, 3]  slot, env, slot the new goal came from (-1 in a real sample); all -1 where the sample gave up */
} mcg_her_batch;

/* All three calls enqueue on `stream` and do not synchronise.  Checked on the host before any HIP call (MCG_ERR_ARG): a null struct or
   required pointer (every pointer of mcg_her_buf; obs and achieved_goal of `first`; actions and obs, achieved_goal, desired_goal,
   reward, terminated, truncated, final_obs, final_achieved, final_desired of `out`), n_envs / obs_dim / act_dim / max_episode_steps /
   batch < 1, capacity < 2 * max_episode_steps, n_virtual outside [0, batch], n_written < 0.  MCG_ERR_UNSUPPORTED: n_virtual > 0 with
   MCG_REWARD_SHAPING (that reward depends on simulator state, as for mcg_compute_reward). */
int64_t mcg_her_record_bytes(int obs_dim, int act_dim);      /* 0 where a dimension is < 1 */

/* An episode starts in the environments of `mask` (NULL = all) from the observation a reset wrote to `first`: last_obs, last_achieved
   and t_run = 0.  An episode that was in flight there is abandoned. */
int mcg_her_start(const mcg_her_buf* buf, const mcg_step_out* first, const uint8_t* mask /* [N] device or NULL */, void* stream);

/* One transition per environment into slot n_written % capacity; the caller then counts n_written up by one.  `out` is what mcg_step
   wrote for `actions`.  done = truncated | terminated; where done, the engine's obs / achieved_goal / desired_goal already belong to the
   next episode: the record's next_obs / next_achieved / desired are final_obs / final_achieved / final_desired there, and the episode's
   length is written into its t_run + 1 slots.  float64 -> float32 by round-to-nearest-even. */
int mcg_her_add(const mcg_her_buf* buf, int64_t n_written, const float* actions /* [N, A] device */, const mcg_step_out* out, void* stream);

/* A batch by the `future` strategy; W = min(n_written, capacity), pos = n_written % capacity.  Uniforms: Philox4x32-10 with counter
   (sample index k, (uint32)call, draw, 3 ^ ((uint32)(call >> 32) << 8)) and key `seed` (stream 3; 0-2: the reset draws), mapped to the
   pair (u0, u1) as every reset draw is.
     draw d = 0..255   slot s = min(W - 1, floor(u0 * W)), environment e = min(N - 1, floor(u1 * N)).  The slot's absolute time is
                       a = n_written - 1 - ((pos - 1 - s) mod capacity).  Valid iff ep_len > 0 and a - t_in_ep >= max(0, n_written -
                       capacity): the episode is complete and its first slot is not overwritten (an episode is overwritten from its
                       start).  Sample k takes the first valid pair: SB3's uniform choice among the valid transitions.  After 256
                       invalid draws it gives up: index -1, outputs zero, counters[0] counted up.
     draw 256          samples k >= batch - n_virtual (SB3's split, real samples first) are relabelled: the future step
                       f = min(ep_len - 1, t_in_ep + floor(u0 * (ep_len - t_in_ep))), current step included, as SB3's randint(t, len);
                       the new goal is next_achieved of slot (s + f - t_in_ep) mod capacity, the reward mcg_compute_reward's expression
                       on (the sample's next_achieved, the new goal) in float64.
   t_in_ep and ep_len are clamped to [0, max_episode_steps] where they are read: no address and no loop bound depends on a record's
   content otherwise, and a corrupt record gives a wrong sample and nothing else. */
int mcg_her_sample(const mcg_her_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch, int n_virtual,
                   const mcg_her_batch* out, void* stream);

/* ---- On-policy rollout buffer (SB3's RolloutBuffer as scripts/train.py:99-101 configures PPO / A2C with n_steps, on the engine's N
   lockstep environments): storage, the time-limit bootstrap, the advantage recursion (GAE) and the shuffled minibatch gather.
   Stateless on the C side, as mcg_her_*: the caller owns all device memory and passes it per call; there is no handle.  T = n_steps,
   N = n_envs; everything is time-major [T, N], as SB3's [buffer_size, n_envs], and the write position is a host integer.
   One record per (step, env), mcg_rollout_record_bytes(D, A) bytes, contiguous, float32 throughout:
     byte 0            float obs[D], achieved[3], desired[3]     the observation the action was taken from
     then              float action[A], log_prob
     zero padding to a multiple of 16 bytes.
   These fields are only ever read by the gather, so a sample is one contiguous run.  What the recursion reads or writes lies in planes
   [T, N] of their own (lane = environment, rows coalesced). */
typedef struct mcg_rollout_buf {    /* device pointers the caller owns (all required), and the buffer's shape */
  void* records;                    /* [T, N] records; 16-byte aligned */
  float* reward;                    /* [T, N]  the step's reward, plus gamma * final_values where the time limit ended the episode */
  float* value;                     /* [T, N]  the policy's value estimate of the observation the action was taken from */
  uint8_t* episode_start;           /* [T, N]  1 where that observation is the first of its episode */
  float* advantage;                 /* [T, N]  written by mcg_rollout_gae */
  float* returns;                   /* [T, N]  advantage + value */
  float* last_obs;                  /* [N, D]  observation the next transition starts from */
  float* last_goals;                /* [N, 6]  its achieved and desired goal */
  uint8_t* last_start;              /* [N]     1 where it is the first of its episode */
  int32_t n_envs, obs_dim, act_dim, n_steps;
  double gamma, gae_lambda;         /* in [0, 1] */
} mcg_rollout_buf;

typedef struct mcg_rollout_batch {  /* outputs of mcg_rollout_gather; device pointers, any may be NULL (not all).  B = count */
  float* obs;            /* [B, D] */
  float* achieved;       /* [B, 3] */
  float* desired;        /* [B, 3] */
  float* action;         /* [B, A] */
  float* old_value;      /* [B] */
  float* old_log_prob;   /* [B] */
  float* advantage;      /* [B] */
  float* returns;        /* [B] */
  int32_t* index;        /* [B]     flat index of the sample in SB3's swap_and_flatten order, env * T + step */
} mcg_rollout_batch;

/* All calls enqueue on `stream` and do not synchronise.  Checked on the host before any HIP call (MCG_ERR_ARG): a null struct or a null
   pointer in it; n_envs / obs_dim / act_dim / n_steps < 1; n_steps * n_envs >= 2^31; records not 16-byte aligned; gamma or gae_lambda
   not finite or outside [0, 1]; pos outside [0, n_steps); first < 0, count < 1 or first + count > n_steps * n_envs; a null actions /
   values / log_probs / last_values; a null mcg_step_out or mcg_rollout_batch; obs, achieved_goal, desired_goal of `first`; those and
   reward, terminated, truncated of `out`; all nine outputs of a batch null. */
int64_t mcg_rollout_record_bytes(int obs_dim, int act_dim);      /* 0 where a dimension is < 1 */

/* The environments of `mask` (NULL = all) continue from the observation a reset wrote to `first`: last_obs, last_goals, and
   last_start = 1.  float64 -> float32 by round-to-nearest-even. */
int mcg_rollout_start(const mcg_rollout_buf* buf, const mcg_step_out* first, const uint8_t* mask /* [N] device or NULL */, void* stream);

/* Step `pos` of the rollout; `out` is what mcg_step wrote for `actions`.  The record's obs / achieved / desired come from last_obs /
   last_goals, episode_start[pos] from last_start; action, log_prob and value are stored as given.  The reward is SB3's collect_rollouts
   bootstrap [RECALL: on_policy_algorithm.py; SB3 is not installed next to the reference]: r = (float)out.reward, and where
   truncated & !terminated (TimeLimit.truncated, as sb3_adapter.py states it) and final_values != NULL, r = r + (float)gamma *
   final_values[e], the product rounded before the sum.  Afterwards last_obs / last_goals are out.obs / achieved_goal / desired_goal
   (which already belong to the next episode where this one ended) and last_start = truncated | terminated.  final_obs is not read. */
int mcg_rollout_add(const mcg_rollout_buf* buf, int pos, const float* actions /* [N, A] device */, const float* values /* [N] */,
                    const float* log_probs /* [N] */, const float* final_values /* [N]: value of final_obs; or NULL */,
                    const mcg_step_out* out, void* stream);

/* SB3's compute_returns_and_advantage [RECALL: buffers.py] over the T stored steps, every operation in float32, rounded one by one
   (nothing fused), in this order: g32 = (float)gamma, c32 = (float)(gamma * gae_lambda) (the product in double), last = 0, and for
   t = T-1 .. 0, with start_next = episode_start[t+1], vn = value[t+1] (t = T-1: last_start, last_values):
     nnt   = 1.0f - (float)start_next
     delta = (reward[t] + (g32 * vn) * nnt) - value[t]
     last  = delta + (c32 * nnt) * last
     advantage[t] = last;  returns[t] = last + value[t] */
int mcg_rollout_gae(const mcg_rollout_buf* buf, const float* last_values /* [N] device */, void* stream);

/* Samples k = first .. first + count - 1 of epoch `epoch`'s permutation of the M = T * N stored transitions, into rows 0 .. count - 1 of
   the outputs.  A transition's flat index is i = env * T + step (SB3's swap_and_flatten).  The permutation is computed per sample, with
   no index array and no sort: a 4-round balanced Feistel network on b bits with cycle walking.
     b, h              b = the smallest even number >= 2 with 2^b >= M; h = b / 2; a value x splits into L = x >> h, R = x & (2^h - 1)
     round r = 0..3    (L, R) -> (R, L ^ F_r(R)),  F_r(R) = w0 & (2^h - 1), w0 = word 0 of Philox4x32-10 with counter
                       (R, (uint32)epoch, r, 4 ^ ((uint32)(epoch >> 32) << 8)) and key `seed` (stream 4; 0-2: the reset draws, 3: HER)
     walk              x = k; x = (L << h) | R after the four rounds; repeated until x < M: sample k is transition x.
   The network is a bijection of [0, 2^b), so the walk from a k < M comes back below M (a cycle closes) and the map k -> x is a
   bijection of [0, M); 2^b < 4 M, so a walk takes fewer than 4 passes in expectation.  No address depends on stored content. */
int mcg_rollout_gather(const mcg_rollout_buf* buf, uint64_t seed, uint64_t epoch, int64_t first, int64_t count,
                       const mcg_rollout_batch* out, void* stream);

/* ---- On-policy rollout buffer of pictures (the same SB3 RolloutBuffer, scripts/train.py:99-101, on what MyCobotImgEnv observes: the
   uint8 picture [C, S, S] alone).  Stateless as mcg_rollout_*; T = n_steps, N = n_envs, time-major, the write position a host integer.
   Pu = C * S * S bytes of a picture, channel-major as the environment holds it; P = Pu rounded up to a multiple of 16.
     pixels   uint8 [T + 1, N, P]: row t holds the picture the action of step t was taken from, row T the picture the next rollout
              continues from; bytes Pu .. P - 1 of every picture that a call writes are zero.  There is no carried last observation:
              mcg_rollout_img_start writes row `pos`, mcg_rollout_img_add(pos) writes the step's picture into row pos + 1, and
              mcg_rollout_img_carry copies row T (the write position) to row 0 between two rollouts.  An insertion reads and writes each pixel once.
     records  one per (step, env), mcg_rollout_img_record_bytes(A) bytes: float action[A], log_prob; zero padding to a multiple of 16.
     planes   reward, value, episode_start, advantage, returns [T, N] and last_start [N]: those of mcg_rollout_buf, by the same rules.
   A picture is passed as a base pointer and two strides in bytes: channel c of environment e is the S * S contiguous bytes at
   img + e * env_stride + c * chan_stride (the environment's [C, N, S, S] buffer: env_stride = S * S, chan_stride = N * S * S; a
   contiguous [N, C, S, S] tensor: env_stride = C * S * S, chan_stride = S * S).  It is read with 16-byte loads where img, both strides
   and S * S are multiples of 16, with 4-byte loads where they are multiples of 4, and byte by byte otherwise; the choice is made on
   the host, and every store to `pixels` is 16 bytes wide. */
typedef struct mcg_rollout_img_buf {  /* device pointers the caller owns (all required), and the buffer's shape */
  uint8_t* pixels;                  /* [T + 1, N, P]; 16-byte aligned */
  void* records;                    /* [T, N] records; 16-byte aligned */
  float* reward;                    /* [T, N]  as mcg_rollout_buf's */
  float* value;                     /* [T, N] */
  uint8_t* episode_start;           /* [T, N]  1 where the picture of row t is the first of its episode */
  float* advantage;                 /* [T, N]  written by mcg_rollout_img_gae */
  float* returns;                   /* [T, N] */
  uint8_t* last_start;              /* [N]     1 where the picture to continue from is the first of its episode */
  int32_t n_envs, channels, size, act_dim, n_steps;      /* channels <= 8, size <= 512 */
  double gamma, gae_lambda;         /* in [0, 1] */
} mcg_rollout_img_buf;

typedef struct mcg_rollout_img_batch {  /* outputs of mcg_rollout_img_gather; device pointers, any may be NULL (not all).  B = count */
  uint8_t* pix;          /* [B, Pu]  the picture as stored (no padding between rows) */
  float* pix_f32;        /* [B, Pu]  byte / 255 in float32, correctly rounded: bit for bit (float)b / 255.0f, SB3's obs.float() / 255 */
  float* action;         /* [B, A] */
  float* old_value;      /* [B] */
  float* old_log_prob;   /* [B] */
  float* advantage;      /* [B] */
  float* returns;        /* [B] */
  int32_t* index;        /* [B]     env * T + step, as mcg_rollout_batch's */
} mcg_rollout_img_batch;

/* All calls enqueue on `stream` and do not synchronise.  Checked on the host before any HIP call (MCG_ERR_ARG): a null struct or a null
   pointer in it; n_envs / channels / size / act_dim / n_steps < 1; channels > 8; size > 512; n_steps * n_envs >= 2^31; pixels or records
   not 16-byte aligned; gamma or gae_lambda not finite or outside [0, 1]; pos outside [0, n_steps) (mcg_rollout_img_start and
   mcg_rollout_img_carry: outside [0, n_steps]); first < 0, count < 1 or first + count > n_steps * n_envs; a null img / actions / values / log_probs / reward /
   terminated / truncated / last_values; a negative stride, or a channel stride below S * S while channels > 1; a null
   mcg_rollout_img_batch or all eight outputs of a batch null. */
int64_t mcg_rollout_img_record_bytes(int act_dim);               /* 0 where act_dim < 1 */

/* The environments of `mask` (NULL = all) continue from the picture a reset returned: it is written to row `pos` of pixels (the write
   position: 0 at the start of a rollout, n_steps after a full one, before the carry), and last_start = 1. */
int mcg_rollout_img_start(const mcg_rollout_img_buf* buf, int pos, const uint8_t* img, int64_t env_stride, int64_t chan_stride,
                          const uint8_t* mask /* [N] device or NULL */, void* stream);

/* Step `pos` of the rollout, one launch.  `img` is the picture the step returned (after an auto-reset: the next episode's first; the
   finished episode's last picture is never read) and goes to row pos + 1 of pixels; `reward` (float64), `terminated` and `truncated`
   are mcg_step_out's.  The record takes action and log_prob as given, its padding zeros.  The plane row is mcg_rollout_add's: value
   as given, episode_start[pos] = last_start, then last_start = truncated | terminated, and the reward r = (float)reward, and where
   truncated & !terminated and final_values != NULL, r = r + (float)gamma * final_values[e], the product rounded before the sum. */
int mcg_rollout_img_add(const mcg_rollout_img_buf* buf, int pos, const float* actions /* [N, A] device */, const float* values /* [N] */,
                        const float* log_probs /* [N] */, const float* final_values /* [N] or NULL */, const uint8_t* img,
                        int64_t env_stride, int64_t chan_stride, const double* reward /* [N] */, const uint8_t* terminated /* [N] */,
                        const uint8_t* truncated /* [N] */, void* stream);

/* mcg_rollout_gae's recursion on this buffer's planes: the same kernel, operation for operation. */
int mcg_rollout_img_gae(const mcg_rollout_img_buf* buf, const float* last_values /* [N] device */, void* stream);

/* Row `pos` of pixels (the write position: n_steps after a full rollout) to row 0, one launch: the picture the next rollout continues
   from; last_start stays as it is.  pos = 0: nothing to do, no launch. */
int mcg_rollout_img_carry(const mcg_rollout_img_buf* buf, int pos, void* stream);

/* Samples k = first .. first + count - 1 of epoch `epoch`, by the permutation of mcg_rollout_gather exactly (one implementation of
   the walk serves both): equal (seed, epoch, T, N) give equal `index`.  Sample k, transition x = env * T + step, takes the picture of
   row `step`, environment env.  All byte offsets are 64-bit; no address and no loop bound depends on stored content. */
int mcg_rollout_img_gather(const mcg_rollout_img_buf* buf, uint64_t seed, uint64_t epoch, int64_t first, int64_t count,
                           const mcg_rollout_img_batch* out, void* stream);

/* ---- Stacks of k = frame_stack frames (the frame stacking section below: slot s of a stack is channels s * C .. s * C + C - 1, slot
   k - 1 the newest) gathered from the single stored frames.  The struct and mcg_rollout_img_start / _add / _gae are unchanged and run
   on rows 0 .. T as before.  The contract of the two entries below: with frame_stack = k the caller guarantees k - 1 valid rows
   before `pixels` (rows -(k - 1) .. -1, N * P bytes each) and k - 1 valid rows before `episode_start` (N bytes each) -- the history:
   the last k - 1 pictures of the previous rollout and their flags -- and passes pointers to row 0, as always.
     flag of a row   row t of environment e is the first picture of its episode iff its flag is 1: episode_start[t, e] for t < pos
                     (t < 0: a history row), last_start[e] for row pos.
     stack(t)        slot k - 1 - i holds the picture of row t - i for i = 0, 1, ... up to and including the first row whose flag
                     is 1, at most k - 1 steps back; the older slots are zeros.

   The carry between two rollouts: pixel rows pos - (k - 1) .. pos go to rows -(k - 1) .. 0 and episode_start rows
   pos - (k - 1) .. pos - 1 to rows -(k - 1) .. -1, one launch; last_start stays as it is.  Source and destination overlap where
   pos < k (a short or an unfinished rollout): a lane owns one 16-byte position of one environment in all k rows, loads them all and
   only then stores, and likewise one lane per environment its k - 1 flag bytes.  pos = 0: nothing to do, no launch.
   frame_stack = 1 does what mcg_rollout_img_carry does.  Refused (MCG_ERR_ARG) beyond what mcg_rollout_img_carry refuses:
   frame_stack outside [1, 8]. */
int mcg_rollout_img_carry_stacked(const mcg_rollout_img_buf* buf, int pos, int frame_stack, void* stream);

/* mcg_rollout_img_gather with `pix` / `pix_f32` as stacks: the same permutation, planes, record and `index`; the rows of pix and
   pix_f32 are k * Pu long, and sample k, transition (env, step), takes stack(step) of a full rollout (pos = T).  A slot before the
   episode's start is written as zeros and its source is not read; every byte of the outputs given is written.  frame_stack = 1 gives
   mcg_rollout_img_gather's outputs bit for bit.  No address and no loop bound depends on stored content beyond the walk back: the
   k - 1 <= 7 flags of rows step, step - 1, ... of the sample's environment (their addresses depend on the permutation alone) are
   loaded together and tested up to the first 1.  All byte offsets are 64-bit.  Refused (MCG_ERR_ARG) beyond what
   mcg_rollout_img_gather refuses: frame_stack outside [1, 8]. */
int mcg_rollout_img_gather_stacked(const mcg_rollout_img_buf* buf, int frame_stack, uint64_t seed, uint64_t epoch, int64_t first,
                                   int64_t count, const mcg_rollout_img_batch* out, void* stream);

/* ---- Off-policy replay buffer of pictures (SB3's ReplayBuffer, which SAC, TD3 and DDPG train from, scripts/train.py:62, 102-104, on
   what MyCobotImgEnv observes: the uint8 picture [C, S, S] alone).  Stateless as mcg_her_* and mcg_rollout_img_*: the caller owns all
   device memory and passes it per call.  N = n_envs, K = capacity (transitions kept per environment), R = K + 1 rows,
   Tm = max_episode_steps, F = ceil(K / Tm) + 1 final rows; Pu, P and the way a picture is passed (base, env_stride, chan_stride; the
   three load widths) are mcg_rollout_img_*'s.  n_written is a host integer: the absolute time a of the next transition.
     pixels      uint8 [R, N, P]: row a % R holds the picture the action of transition a was taken from, row (a + 1) % R the picture the
                 step returned (after an auto-reset: the next episode's first).  Every picture is stored once; the next picture of a
                 slot is the following row.  Bytes Pu .. P - 1 of every picture that a call writes are zero.
     finals      uint8 [F, N, P] and final_time int64 [F, N] (the caller sets every final_time to -1 before the first call): where the
                 time limit alone ended an episode (truncated & !terminated, mcg_rollout_add's definition), the finished episode's
                 last picture goes to row (a / Tm) % F of finals and final_time there becomes a.  The engine sets `truncated` by the
                 time limit at elapsed >= Tm only and every reset zeroes elapsed, so two time-limit ends of one environment are at
                 least Tm steps apart and their a / Tm differ; the K newest transitions span at most ceil(K / Tm) + 1 values of
                 a / Tm: no final picture of a stored transition is overwritten.  A caller who breaks this (set_state(elapsed=...))
                 is caught by the stamp, not by a wrong picture.
     records     one per (row, env), mcg_replay_img_record_bytes(A) bytes: float action[A], float reward (the step's float64 rounded
                 to nearest even), uint32 flags, zeros to a multiple of 16.  Flags: 1 TERMINATED, 2 TIMEOUT (truncated &
                 !terminated), 4 NO_NEXT (a start in mid-episode overwrote the next picture: never sampled).
     counters    uint64 [2]: samples that gave up; timeout samples whose final picture had been overwritten. */
typedef struct mcg_replay_img_buf {   /* device pointers the caller owns (all required), and the buffer's shape */
  uint8_t* pixels;                  /* [K + 1, N, P]; 16-byte aligned */
  uint8_t* finals;                  /* [F, N, P]; 16-byte aligned */
  int64_t* final_time;              /* [F, N]; -1 before the first call */
  void* records;                    /* [K + 1, N] records; 16-byte aligned */
  uint64_t* counters;               /* [2] */
  int32_t n_envs, channels, size, act_dim, capacity, max_episode_steps;      /* channels <= 8, size <= 512 */
} mcg_replay_img_buf;

typedef struct mcg_replay_img_batch { /* outputs of mcg_replay_img_sample; device pointers, any may be NULL (not all).  B = batch */
  uint8_t* pix;          /* [B, Pu]  the picture the action was taken from, as stored (no padding between rows) */
  uint8_t* next_pix;     /* [B, Pu]  the picture the step led to */
  float* pix_f32;        /* [B, Pu]  byte / 255 in float32, correctly rounded: bit for bit (float)b / 255.0f, SB3's obs.float() / 255 */
  float* next_pix_f32;   /* [B, Pu] */
  float* action;         /* [B, A] */
  float* reward;         /* [B] */
  float* done;           /* [B]     1.0 where the transition ended its episode for good (SB3's dones * (1 - timeouts)) */
  int32_t* index;        /* [B, 3]  row, env, source of the next picture (0: pixels, 1: finals); -1, -1, -1 where the sample gave up */
} mcg_replay_img_batch;

/* All calls enqueue on `stream` and do not synchronise.  Checked on the host before any HIP call (MCG_ERR_ARG), each with its own
   message: a null struct or a null pointer in it; n_envs / channels / size / act_dim / capacity / max_episode_steps < 1; channels > 8;
   size > 512; (capacity + 1) * n_envs >= 2^31; pixels, finals or records not 16-byte aligned; n_written < 0 (mcg_replay_img_sample:
   n_written == 0, the buffer is empty); batch < 1; a null img / final_img / actions / reward / terminated / truncated; a negative
   stride, or a channel stride below S * S while channels > 1; a null mcg_replay_img_batch or all eight outputs of a batch null. */
int64_t mcg_replay_img_record_bytes(int act_dim);                /* 0 where act_dim < 1 */

/* The environments of `mask` (NULL = all) continue from the picture a reset returned: it is written to row n_written % R.  Where
   n_written >= 1, the record of transition n_written - 1 gets NO_NEXT unless it carries TERMINATED or TIMEOUT: a reset after an
   episode's end loses nothing, a reset in mid-episode loses that transition's next picture, so it is never sampled. */
int mcg_replay_img_start(const mcg_replay_img_buf* buf, int64_t n_written, const uint8_t* img, int64_t env_stride, int64_t chan_stride,
                         const uint8_t* mask /* [N] device or NULL */, void* stream);

/* Transition a = n_written of every environment, one launch; the caller then counts n_written up.  `img` is the picture the step
   returned and goes to row (a + 1) % R; the record of row a % R takes action, (float)reward and the flags; where TIMEOUT, `final_img`
   (the finished episode's last picture, info["final_observation"]; its own strides) goes to row (a / Tm) % F of finals and
   final_time there becomes a.  Every pixel is read once and written once. */
int mcg_replay_img_add(const mcg_replay_img_buf* buf, int64_t n_written, const float* actions /* [N, A] device */, const uint8_t* img,
                       int64_t env_stride, int64_t chan_stride, const uint8_t* final_img, int64_t final_env_stride,
                       int64_t final_chan_stride, const double* reward /* [N] */, const uint8_t* terminated /* [N] */,
                       const uint8_t* truncated /* [N] */, void* stream);

/* `batch` transitions, uniform over the W = min(n_written, K) newest of every environment that still have their next picture (SB3's
   uniform choice over stored transitions).  Uniforms are Philox4x32-10 exactly as mcg_her_sample takes them, on stream 5: counter
   (k, (uint32)call, draw, 5 ^ ((uint32)(call >> 32) << 8)), key `seed`.  Draw d = 0 .. 255 of sample k: j = min(W - 1, floor(u0 W)),
   a = n_written - W + j, e = min(N - 1, floor(u1 N)); the draw is valid iff the record of (a % R, e) has no NO_NEXT; the first valid
   draw is taken; after 256 invalid draws the sample gives up: index -1, outputs zeros, counters[0] counted.
   The picture is row a % R.  The next picture is row (a / Tm) % F of finals where the record has TIMEOUT and final_time there == a,
   and row (a + 1) % R of pixels otherwise.  done = 1.0 where TERMINATED, and where TIMEOUT with another stamp (counters[1] counted;
   another episode's picture is never handed out as the successor: the transition is treated as terminal), else 0.0.  Where
   TERMINATED, the next picture is the post-reset picture of row (a + 1) % R: its weight in a TD target is zero.
   No address and no loop bound depends on stored content beyond the two flag tests and the stamp compare; all byte offsets are 64-bit. */
int mcg_replay_img_sample(const mcg_replay_img_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch,
                          const mcg_replay_img_batch* out, void* stream);

/* ---- Frame stacking for the pictures (SB3's VecFrameStack, channels first: StackedObservations).  A frame is a whole stored picture of
   C channels, Pu = C * S * S bytes; a stack of k = frame_stack frames is [k * C, S, S], k * Pu bytes: slot s is channels
   s * C .. s * C + C - 1, slot k - 1 the newest.  After a reset the slots older than the episode are zeros.

   mcg_replay_img_sample with `observations` and `next_observations` as stacks, rebuilt from the single-frame ring: the k - 1 frames
   before row a are the k - 1 rows before it, so nothing is stored k times.  The struct, mcg_replay_img_start and mcg_replay_img_add
   are unchanged; a caller who wants K sampleable transitions passes capacity = K + k - 1 (R = K + k rows), and the entry samples over
   the W = min(n_written, capacity - (k - 1)) newest: every sampleable transition keeps its whole history in the ring, and none of the
   k - 1 older rows is ever a sample.  The rows of pix / next_pix / pix_f32 / next_pix_f32 of the batch are k * Pu long here.
     episode start   the picture of time t is the first of its episode iff t == 0 or the record of transition t - 1 carries any of
                     TERMINATED, TIMEOUT, NO_NEXT.
     stack(t)        slot k - 1 - i is the picture of time t - i (row (t - i) % R) for i = 0 .. d - 1, where d - 1 is the number of
                     steps one can walk back from t without crossing an episode start, capped at k - 1; older slots are zeros.
     a sample        the draws, the give-up, done, action, reward, index and both counters are mcg_replay_img_sample's, with W as
                     above.  pix = stack(a).  next_pix = stack(a + 1) -- after TERMINATED, and after a TIMEOUT whose final picture
                     was overwritten (done = 1, counters[1]), that is zeros and the next episode's first picture -- but where the
                     record has TIMEOUT and the stamp equals a: stack(a) shifted down one slot with the final picture in slot k - 1
                     (SB3's stacked terminal_observation).
   Every byte of the outputs given is written, the zero slots as zeros.  frame_stack == 1 gives mcg_replay_img_sample's outputs bit for
   bit.  No address and no loop bound depends on stored content beyond the two flag tests and the stamp compare of
   mcg_replay_img_sample and the walk back: the flags of the k - 1 <= 7 records before the sample's (their rows depend on the draw
   alone) are tested up to the first episode start.  All byte offsets are 64-bit.  Refused (MCG_ERR_ARG) beyond what mcg_replay_img_sample refuses: frame_stack outside [1, 8];
   capacity - (frame_stack - 1) < 1. */
int mcg_replay_img_sample_stacked(const mcg_replay_img_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch, int frame_stack,
                                  const mcg_replay_img_batch* out, void* stream);

/* The act-time half, SB3's StackedObservations.update with done = terminated | truncated; stateless, one launch on `stream`, no
   synchronisation.  `stack` is the caller's uint8 [N, k * Pu], contiguous, updated in place; `final_stack` (NULL: none; then final_img
   is not read) has the same shape.  `img` and `final_img` are pictures as mcg_rollout_img_* takes them (base, env_stride, chan_stride;
   the three load widths; the stacks are read and written at the narrowest width that they and the pictures allow).
     mask == NULL   a step.  final_stack[e] = the old stack shifted down one slot, then final_img[e] in the newest slot, for every
                    environment; stack[e] = the old stack shifted down one slot, the older slots zeros where done[e], then img[e] in
                    the newest slot.
     mask != NULL   a reset.  Where mask[e]: the older slots of stack[e] are zeros, its newest slot is img[e], and final_stack[e] as
                    above if given; the other environments are left as they are.  `done` is not read and may be NULL.
   A lane owns one 16-byte position of one environment's frame; it loads slots 1 .. k - 1, img and final_img at that position and only
   then stores, so the shift in place has no hazard between lanes, and every byte is read once and written once per output.
   Checked on the host before any HIP call (MCG_ERR_ARG), each with its own message: a null stack; n_envs / channels / size < 1;
   channels > 8; size > 512; frame_stack outside [1, 8]; n_envs * ceil(Pu / 16) >= 2^31; final_stack == stack; done and mask both null;
   a null img (final_img, where final_stack is given); a negative stride, or a channel stride below S * S while channels > 1. */
int mcg_frame_stack_push(uint8_t* stack, uint8_t* final_stack, int n_envs, int channels, int size, int frame_stack, const uint8_t* img,
                         int64_t env_stride, int64_t chan_stride, const uint8_t* final_img, int64_t final_env_stride,
                         int64_t final_chan_stride, const uint8_t* done /* [N] device */, const uint8_t* mask /* [N] device or NULL */,
                         void* stream);

/* ---- The actor-critic policy forward (SB3's MultiInputPolicy as PPO / A2C use it, scripts/train.py:99-101: for a Dict space of Boxes
   two MLPs without shared layers and a DiagGaussianDistribution).  Stateless: the caller owns the weights (one float32 device blob, laid
   out as mcg_policy.hip's head states and mycobotgym_amd/policy.py packs it) and the call number.  One launch on `stream`, no
   synchronisation.
     features   [achieved_goal(3), desired_goal(3), observation(D)] (SB3's CombinedExtractor: the keys in sorted order), each float64
                rounded to float32 (round to nearest even), read where the engine wrote them.
     trunks     n_pi / n_vf layers of pi_width / vf_width units, x -> act(W x + b), act = tanh or max(., 0); float32 throughout
                (v_mfma_f32_16x16x4_f32; the order of a sum over k is the kernel's).
     heads      mean = action_net(policy trunk) [N, A];  value = value_net(value trunk) [N].
     noise      eps [N, A]: Philox4x32-10, key `seed`, counter ((uint32)gid, (uint32)call, pair ^ ((uint32)(call >> 32) << 8),
                6 ^ ((uint32)(gid >> 32) << 8)), gid = env_id_offset + env, pair = 0 .. ceil(A / 2) - 1 (domain 6; 0-5: the reset, scene,
                HER, rollout and picture-replay draws).  The block's two 53-bit uniforms u0, u1 (as every draw here maps them) give
                eps[2 pair] = sqrt(-2 ln(1 - u0)) cos(2 pi u1) and eps[2 pair + 1] = sqrt(-2 ln(1 - u0)) sin(2 pi u1), evaluated in
                double and rounded to float32 once.  deterministic != 0: eps = 0, nothing is drawn.
     action     mean + exp(log_std) eps, evaluated in double from the float32 mean, log_std and eps and rounded once; not clipped
                (SB3 stores the unclipped action; mcg_step clips what it reads).  deterministic: the mean's bits.
     log_prob   sum over k of (-eps_k^2 / 2 - log_std_k - ln(2 pi) / 2) in float32.
   With action, log_prob, mean and noise all NULL the policy trunk is not evaluated (the value of a final observation).  A row of the
   outputs depends on its own environment alone; rows past n_envs of the last tile of 16 are not stored.
   Checked on the host before any HIP call (MCG_ERR_ARG, each with a message that names the field): a null struct; a null blob; n_envs,
   obs_dim or act_dim < 1; obs_dim > 4096; act_dim > 16; n_pi or n_vf outside [1, 3]; a width that is no multiple of 16 in [16, 256];
   an activation other than the two below; blob_floats != mcg_policy_blob_floats of the shape; a blob that is not 16-byte aligned; a
   null mcg_step_out or obs / achieved_goal / desired_goal in it; a null mcg_policy_out or all five outputs null. */
#define MCG_POLICY_TANH 0
#define MCG_POLICY_RELU 1

typedef struct mcg_policy {
  const float* blob;                /* device, 16-byte aligned, blob_floats floats */
  int32_t n_envs, obs_dim, act_dim;
  int32_t n_pi, n_vf;               /* hidden layers of the policy and the value trunk: 1..3 */
  int32_t pi_width[3], vf_width[3]; /* their widths: multiples of 16, at most 256 (entries from n_pi / n_vf on are not read) */
  int32_t activation;               /* MCG_POLICY_TANH or MCG_POLICY_RELU */
  int64_t blob_floats;              /* must equal mcg_policy_blob_floats of this shape */
} mcg_policy;

typedef struct mcg_policy_out {     /* device pointers, any may be NULL to skip (not all) */
  float* action;         /* [N, A] */
  float* value;          /* [N] */
  float* log_prob;       /* [N] */
  float* mean;           /* [N, A] */
  float* noise;          /* [N, A]  eps */
} mcg_policy_out;

/* Size of the blob in floats; 0 for a refused shape. */
int64_t mcg_policy_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_vf, const int32_t* vf_width);

/* `obs`: what mcg_reset / mcg_step wrote (obs, achieved_goal, desired_goal are read; a final observation goes into the same three
   fields).  `call`: the number of the sampling call, the caller's to count. */
int mcg_policy_forward(const mcg_policy* pol, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset,
                       int deterministic, const mcg_policy_out* out, void* stream);

/* ---- The policy update (the other half of PPO / A2C as SB3 runs them on that policy): evaluate_actions, the loss and its gradient
   with respect to every parameter, and clip-by-norm + Adam on the blob in place (mcg_policy_grad.hip).  Stateless, as everything here:
   the caller owns the blob, the gradient, the moments and the scratch; every call enqueues on `stream` and none synchronises.  The
   minibatch is float32, in the arrays mcg_rollout_gather writes; B = its rows, any value >= 1 (pol->n_envs is not read).
   All of it is deterministic: no floating-point atomics, every sum in an order fixed by the shape and B alone. */
typedef struct mcg_policy_eval_out {/* device pointers, any may be NULL to skip (not all) */
  float* value;          /* [B] */
  float* log_prob;       /* [B]  sum_k (-(a_k - mean_k)^2 / (2 sigma_k^2) - log_std_k - ln(2 pi) / 2) */
  float* entropy;        /* [B]  sum_k (1/2 + ln(2 pi) / 2 + log_std_k) */
} mcg_policy_eval_out;

/* SB3's evaluate_actions, forward only: obs, achieved, desired and action of `batch` are read (the other fields are not). */
int mcg_policy_evaluate(const mcg_policy* pol, const mcg_rollout_batch* batch, int64_t B, const mcg_policy_eval_out* out, void* stream);

#define MCG_LOSS_PPO 0
#define MCG_LOSS_A2C 1

typedef struct mcg_policy_hyper {   /* SB3's names; clip_range_vf is not built */
  int32_t loss_kind;                /* MCG_LOSS_PPO or MCG_LOSS_A2C */
  int32_t normalize_advantage;      /* != 0 and B > 1: adv <- (adv - mean) / (std + 1e-8), std the unbiased one (torch.std) */
  float clip_range;                 /* PPO's c, > 0 (A2C: not read) */
  float ent_coef, vf_coef;
} mcg_policy_hyper;

/* The loss of the minibatch and its gradient.  With ratio = exp(log_prob - old_log_prob):
     policy_loss   PPO: -mean(min(adv ratio, adv clamp(ratio, 1 - c, 1 + c)));  A2C: -mean(adv log_prob)
     value_loss    mean((returns - value)^2);     entropy_loss  -mean(entropy)
     loss          policy_loss + ent_coef entropy_loss + vf_coef value_loss
   obs, achieved, desired, action, old_log_prob, advantage and returns of `batch` are read (old_log_prob: PPO only).
   grad   [blob_floats], 16-byte aligned, in the blob's own layout: the gradient of the weight at blob position p is grad[p]; every
          padding position (head rows from A, or from 1 for the value head, up to 15; first-layer columns from D + 6 on; the log_std
          pad) is written as +0.0f.
   stats  [8]: loss, policy_loss, value_loss, entropy_loss, approx_kl = mean((ratio - 1) - ln ratio), clip_fraction =
          mean(|ratio - 1| > c), 0, 0 (A2C: approx_kl and clip_fraction are 0).
   work   scratch of work_floats >= mcg_policy_grad_work_floats(pol, B) floats, 16-byte aligned; its content before the call does not
          matter and nothing of it needs to be kept.
   Four launches: the advantage's mean and deviation (skipped where they are not used), the forward and backward pass per tile of 16
   samples, the weight gradients as partial blobs in `work`, their sum in index order. */
int64_t mcg_policy_grad_work_floats(const mcg_policy* pol, int64_t B);      /* 0 for a refused shape or B < 1 */
int mcg_policy_grad(const mcg_policy* pol, const mcg_rollout_batch* batch, int64_t B, const mcg_policy_hyper* hyper, float* work,
                    int64_t work_floats, float* grad, float* stats, void* stream);

/* Clip by global norm as torch's clip_grad_norm_, coef = min(1, max_grad_norm / (||grad||_2 + 1e-6)) (max_grad_norm <= 0: coef = 1;
   the norm over all blob_floats, in a fixed order, is written to norm_out [1] either way), then torch.optim.Adam's step without amsgrad
   or weight decay, elementwise on the blob (pol->blob is written), with g = coef grad:
     m <- beta1 m + (1 - beta1) g;   v <- beta2 v + (1 - beta2) g^2;   p <- p - (lr / (1 - beta1^step)) m / (sqrt(v) / sqrt(1 - beta2^step) + eps)
   The two bias corrections are computed on the host in double from `step` (>= 1).  grad is not changed.  grad, m, v: [blob_floats],
   16-byte aligned; padding positions keep g = m = v = 0 and so stay 0: the blob remains a valid blob.  Two launches. */
int mcg_policy_adam(const mcg_policy* pol, const float* grad, float* m, float* v, int64_t step, double lr, double beta1, double beta2,
                    double eps, double max_grad_norm, float* norm_out, void* stream);

/* ---- SAC's actor and twin critics, the gradient-free half (SB3's SACPolicy as scripts/train.py's default --algo SAC builds it with
   MultiInputPolicy for a Dict space of Boxes; mcg_sac.hip): the collection action, the twin-critic forward, the TD target of a replay
   batch as one launch, and the Polyak step.  Stateless, as everything here: the caller owns three float32 device blobs (actor,
   critic = qf0 then qf1, critic_target in the critic's layout; mcg_sac.hip's head states the layouts and mycobotgym_amd/sac_policy.py
   packs them) and the call numbers.  Every entry enqueues on `stream` and none synchronises.  Additive: MCG_ABI_VERSION stays 8.
   The rule, restated [RECALL: stable_baselines3/sac/policies.py, common/distributions.py, sac/sac.py; SB3 is not installed next to the
   reference]:
     features   [achieved_goal(3), desired_goal(3), observation(D)], as for mcg_policy_forward [RECALL: CombinedExtractor].
     actor      latent_pi: n_pi layers x -> act(W x + b), act = max(., 0) (SB3's default for SAC) or tanh; two linear heads on it, mu
                [A, H] and log_std [A, H] [RECALL: Actor.get_action_dist_params]; float32 throughout (v_mfma_f32_16x16x4_f32).
     log_std    clamped to [-20, 2] by fminf(fmaxf(., -20), 2) [RECALL: LOG_STD_MIN, LOG_STD_MAX]; the `log_std` output is the clamped one.
     noise      eps [., A]: Philox4x32-10 with mcg_policy_forward's counter layout, key `seed`, counter ((uint32)id, (uint32)call,
                pair ^ ((uint32)(call >> 32) << 8), dom ^ ((uint32)(id >> 32) << 8)), pair = 0 .. ceil(A / 2) - 1, and Box-Muller in
                double rounded to float32 once, as there.  mcg_sac_act: dom = 7, id = env_id_offset + env; mcg_sac_target: dom = 8,
                id = the sample's index in the batch.
     u          (float)((double)mu + exp((double)log_std) * (double)eps), rounded once; deterministic: u = mu, nothing is drawn and
                the noise is zeros.
     action     (float)tanh((double)u), rounded once [RECALL: SquashedDiagGaussianDistribution]; |action| <= 1.
     log_prob   sum over k of (-eps_k^2 / 2 - log_std_k - ln(2 pi) / 2) - sum over k of ln(1 - action_k^2 + 1e-6): the Gaussian term on
                the pre-squash u, as SB3's action_log_prob keeps it (at u = mu + sigma eps it is the noise's), the correction SB3's
                expression with its epsilon on the float32 action [RECALL: log_prob -= sum(log(1 - actions**2 + self.epsilon))].  Every
                term and the sum in double from the float32 log_std, eps and action, the four lanes of a row added in a fixed order,
                rounded to float32 once.
     critics    n_critics = 2 [RECALL: ContinuousCritic]: qf0 and qf1, n_qf layers of the same rule on cat(features, action), a scalar
                head each; critic_target is a second pair.
   Rows past the count of the last tile of 16 read the last row and store nothing; a row of the outputs depends on that row alone.
   Checked on the host before any HIP call (MCG_ERR_ARG, each with a message that names the field): a null mcg_sac; a null blob among
   those the entry touches (mcg_sac_act: actor; mcg_sac_q: the one `which` names; mcg_sac_target: actor and critic_target;
   mcg_sac_polyak: critic and critic_target), or one that is not 16-byte aligned; obs_dim or act_dim < 1; obs_dim > 4096; act_dim > 16;
   n_pi or n_qf outside [1, 3]; a width that is no multiple of 16 in [16, 256] (SB3's TD3 / DDPG default [400, 300] is this case); an
   activation other than MCG_POLICY_TANH / MCG_POLICY_RELU; actor_floats or critic_floats other than mcg_sac_blob_floats gives; and
   what each entry lists below. */
#define MCG_SAC_CRITIC 0
#define MCG_SAC_CRITIC_TARGET 1

typedef struct mcg_sac {
  const float* actor;               /* device, 16-byte aligned, actor_floats floats */
  const float* critic;              /* device, 16-byte aligned, critic_floats floats: qf0 then qf1 */
  float* critic_target;             /* likewise; written by mcg_sac_polyak alone */
  int32_t n_envs, obs_dim, act_dim; /* n_envs: rows of mcg_sac_act (the other entries take their rows per call) */
  int32_t n_pi, pi_width[3];        /* latent_pi: 1..3 layers, widths multiples of 16, at most 256 (entries from n_pi on are not read) */
  int32_t n_qf, qf_width[3];        /* each critic likewise */
  int32_t activation;               /* MCG_POLICY_TANH or MCG_POLICY_RELU */
  int64_t actor_floats, critic_floats;      /* must equal what mcg_sac_blob_floats gives for this shape */
} mcg_sac;

typedef struct mcg_sac_act_out {    /* device pointers, float32; all but action may be NULL to skip */
  float* action;         /* [N, A]  required */
  float* log_prob;       /* [N] */
  float* mean;           /* [N, A]  mu */
  float* log_std;        /* [N, A]  clamped */
  float* noise;          /* [N, A]  eps */
} mcg_sac_act_out;

typedef struct mcg_sac_rows {       /* device pointers, float32, all required: the fields of mcg_her_batch under the same names */
  const float* obs;      /* [B, D] */
  const float* achieved; /* [B, 3] */
  const float* desired;  /* [B, 3] */
  const float* action;   /* [B, A] */
} mcg_sac_rows;

typedef struct mcg_sac_target_out { /* device pointers, float32; all but target may be NULL to skip */
  float* target;         /* [B]     required */
  float* next_action;    /* [B, A]  a' */
  float* next_log_prob;  /* [B]     logp' */
  float* next_q;         /* [2, B]  the two target critics at (next_obs, a'), before the min */
  float* noise;          /* [B, A]  eps */
} mcg_sac_target_out;

/* actor_floats + critic_floats, and the two through the pointers (either may be NULL); 0, and zeros, for a refused shape. */
int64_t mcg_sac_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int64_t* actor_floats,
                            int64_t* critic_floats);

/* The collection action: `obs` is what mcg_reset / mcg_step wrote (float64, read in place and rounded to float32); `call` the number
   of the sampling call, the caller's to count.  One launch, one wave per tile of 16 environments.  Also refused: n_envs < 1 or
   >= 2^27; a null mcg_step_out or obs / achieved_goal / desired_goal in it; a null mcg_sac_act_out or a null action. */
int mcg_sac_act(const mcg_sac* sac, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset, int deterministic,
                const mcg_sac_act_out* out, void* stream);

/* Both critics of the blob `which` names on B rows: q[0 .. B) is qf0, q[B .. 2 B) is qf1.  One launch, one wave per (tile, critic).
   Also refused: `which` other than the two above; B < 1 or >= 2^27; a null mcg_sac_rows or field of it; a null q. */
int mcg_sac_q(const mcg_sac* sac, int which, const mcg_sac_rows* rows, int64_t B, float* q /* [2, B] */, void* stream);

/* SB3's target line [RECALL: SAC.train] as one launch:
     a', logp' = actor.action_log_prob(next_obs);  next_q = min(critic_target(next_obs, a')) - alpha logp';
     target = reward + (1 - done) gamma next_q
   in float32 as   next_q = fmaf(-alpha, logp', fminf(q0, q1));   target = fmaf((1 - done) * gamma, next_q, reward)   (the product
   rounded to float32 before the fmaf).  alpha = (float)exp((double)*log_ent_coef), read on the device, where log_ent_coef is not
   NULL (SB3's ent_coef = "auto"); otherwise the host's ent_coef.  Read of `batch`, as mcg_her_sample wrote it: next_obs,
   next_achieved, desired (also the next observation's goal), reward and done.  A row that mcg_her_sample gave up on (index -1, all
   zeros) is computed like any other: its target is that of the all-zero transition, and the caller who samples with no check masks
   it by `index`.  Also refused: B < 1 or >= 2^27; a null batch or one of the five fields; gamma outside [0, 1]; with a null
   log_ent_coef an ent_coef that is negative or not finite; a null mcg_sac_target_out or a null target. */
int mcg_sac_target(const mcg_sac* sac, const mcg_her_batch* batch, int64_t B, uint64_t seed, uint64_t call, float gamma, float ent_coef,
                   const float* log_ent_coef /* [1] device or NULL */, const mcg_sac_target_out* out, void* stream);

/* critic_target <- (1 - tau) critic_target + tau critic, elementwise over the critic_floats of the blob, as
     t <- (float) fma(tau, (double) c, (1.0 - tau) * (double) t)
   with 1.0 - tau formed on the host in double, the product rounded to double, the fma rounded once, and one rounding to float32: no
   contraction setting of a compiler changes a bit.  A padding position, +0.0 in both, stays +0.0.  tau = 1 is special-cased as the copy
   t <- c, bit for bit whatever t held (a target with non-finite elements is repaired; a critic's -0.0 stays -0.0).  For tau < 1 the
   expression stands as written: a non-finite c or t gives a non-finite t (tau = 0 too: 0 * inf), and a sum of zeros comes out +0.0.
   Also refused: tau outside [0, 1]; critic == critic_target. */
int mcg_sac_polyak(const mcg_sac* sac, double tau, void* stream);

/* ---- SAC's update, the gradient half (mcg_sac_grad.hip): one gradient step of SB3's SAC.train [RECALL: sac/sac.py; SB3 is not
   installed next to the reference] is, in this order, because each step reads what an earlier one wrote:
     alpha = exp(log_ent_coef), the value before this step's alpha update (ent_coef = "auto"; else the constant)
     y = mcg_sac_target(batch)                                           (before anything writes log_ent_coef)
     critic_loss = 0.5 (mean((q0 - y)^2) + mean((q1 - y)^2)) on (obs, action); mcg_sac_critic_grad, mcg_sac_adam on `critic`
                   (SB3's SAC clips no gradients)
     a, logp = actor(obs), fresh noise; actor_loss = mean(alpha logp - min(q0(obs, a), q1(obs, a))) through the critic as just
                   updated, a constant here: no critic weight gradient is formed; mcg_sac_actor_grad, mcg_sac_adam on `actor`
     ent_coef_loss = -mean(log_ent_coef (logp + target_entropy)), logp the actor step's; mcg_sac_alpha_step ("auto" only)
     mcg_sac_polyak every target_update_interval steps.
   Stateless, as everything here: the caller owns the gradients, the moments and the scratch; every entry enqueues on `stream` and
   none synchronises.  Float32 on v_mfma_f32_16x16x4_f32 in tiles of 16 samples; deterministic: no atomics, every sum in an order that
   the shape and B alone fix.  Additive: MCG_ABI_VERSION stays 8.
   The actor loss's derivative at the heads, per component, with a = tanh(u), s = 1 - a^2 and the log_std before the clamp:
     d/du       = (alpha 2 a s / (s + 1e-6) - dQ/da s) / B      (the squash correction's term and the chosen critic's)
     d/dmu      = d/du
     d/dlog_std = d/du exp(log_std) eps - alpha / B, and 0 where the clamp acts (log_std < -20 or > 2)
   The Gaussian term -eps^2 / 2 - log_std - ln(2 pi) / 2 is written in eps, which rsample holds fixed: its own derivative is zero
   apart from -log_std, the -alpha / B above.  The terms are formed in double from the float32 values and rounded once.  The min's
   choice per sample is c = (q1 < q0); dQ/da is critic c's alone.
   The noise: mcg_sac_act's counter layout and Box-Muller with dom = 9, id = the sample's index in the batch, call = the caller's count
   of actor-loss calls.
   Checked on the host before any launch, as for the entries above (the kernels get bare pointers): the mcg_sac and the blobs an entry
   touches; null or misaligned (16 bytes) work, grad, m, v; B < 1 or >= 2^27; work_floats below mcg_sac_grad_work_floats; step < 1; and
   what each entry lists. */
int64_t mcg_sac_grad_work_floats(const mcg_sac* sac, int64_t B);          /* scratch of both gradient entries; 0 for a refused shape or B */

/* The critic loss and its gradient over the whole critic blob.  `rows`: obs, achieved, desired, action [B, .]; y [B]: the TD target.
   grad   [critic_floats], 16-byte aligned, in the blob's own layout (the first layer's feature tiles and action tiles where the blob
          keeps them); every padding position (feature columns from D + 6, action columns from A, head rows from 1) is written +0.0f.
   stats  [8]: [0] critic_loss, [4] mean(q0), [5] mean(q1), [7] 0 are written; the others are left.
   work   scratch, 16-byte aligned; its content before the call does not matter.
   Reads `critic` alone of the blobs.  Three launches: a wave per (tile, critic), the dW blocks per part, the sum in part order. */
int mcg_sac_critic_grad(const mcg_sac* sac, const mcg_sac_rows* rows, const float* y, int64_t B, float* work, int64_t work_floats,
                        float* grad, float* stats, void* stream);

typedef struct mcg_sac_actor_grad_out {     /* device pointers, float32; any may be NULL to skip (the struct's pointer too) */
  float* action;         /* [B, A]  a = tanh(u) of the actor-loss draw */
  float* noise;          /* [B, A]  eps */
  float* q_pi;           /* [2, B]  both critics at (obs, a) */
  float* dq_da;          /* [B, A]  the chosen critic's dQ/da */
} mcg_sac_actor_grad_out;

/* The actor loss and its gradient with respect to the actor blob alone.  `rows`: obs, achieved, desired (action is not read).
   alpha = (float)exp((double)*log_ent_coef), read on the device, where log_ent_coef is not NULL; otherwise ent_coef (finite, >= 0).
   grad      [actor_floats], 16-byte aligned, the blob's layout; padding (feature columns from D + 6, head rows from A) is +0.0f.
   logp_out  [B], required: the draw's log-prob, which mcg_sac_alpha_step reads.
   stats     [1] actor_loss, [3] alpha, [6] mean(logp) are written; the others are left.
   Reads `actor` and `critic`; writes neither, nor critic_target.  Three launches: a workgroup of two waves per tile (both the actor,
   wave q critic q and its dQ/da, wave 0 the head and the actor's backward pass), the dW blocks per part, the sum in part order. */
int mcg_sac_actor_grad(const mcg_sac* sac, const mcg_sac_rows* rows, int64_t B, uint64_t seed, uint64_t call, float ent_coef,
                       const float* log_ent_coef /* [1] device or NULL */, float* work, int64_t work_floats, float* grad,
                       float* logp_out, float* stats, const mcg_sac_actor_grad_out* out, void* stream);

/* ent_coef_loss = -mean(log_ent_coef (logp + target_entropy)) and its gradient g = -mean(logp + target_entropy): the mean in double
   in a fixed tree, rounded to float32 once; then torch.optim.Adam's rule (as mcg_policy_adam's, no clip) on the one float with g.
   lr = 0 makes it the gradient alone: log_ent_coef, m and v are not written (m and v may be NULL then).  grad_out [1] and stats [8]
   (only [2], ent_coef_loss, is written) may be NULL.  One launch.  Also refused: a null log_ent_coef or logp; lr < 0 or not finite;
   betas outside [0, 1); eps < 0; a target_entropy that is not finite. */
int mcg_sac_alpha_step(float* log_ent_coef, const float* logp, int64_t B, float target_entropy, float* m, float* v, int64_t step,
                       double lr, double beta1, double beta2, double eps, float* grad_out, float* stats, void* stream);

/* torch.optim.Adam's step without amsgrad or weight decay on a bare blob of `floats` floats, elementwise, as mcg_policy_adam's rule
   with no clip and with 1 - beta1, 1 - beta2 formed on the host in double and rounded to float32 once, as torch passes them; padding
   positions keep g = m = v = 0 and stay +0.0.  blob, grad, m, v: 16-byte aligned.  One launch.  Also refused:
   floats < 1 or >= 2^31; lr < 0 or not finite; betas outside [0, 1); eps < 0. */
int mcg_sac_adam(float* blob, const float* grad, float* m, float* v, int64_t floats, int64_t step, double lr, double beta1, double beta2,
                 double eps, void* stream);

/* ---- TD3 and DDPG (SB3's TD3Policy as scripts/train.py's --algo TD3 / DDPG builds it with MultiInputPolicy for a Dict space of
   Boxes; mcg_td3.hip, mcg_td3_grad.hip): a deterministic actor with a target copy, n_critics = 2 (TD3) or 1 (DDPG) critics with a
   target copy.  Stateless: the caller owns four float32 device blobs, the call numbers and both step counts.  Every entry enqueues on
   `stream` and none synchronises.  Additive: MCG_ABI_VERSION stays 8.
   The rule, restated [RECALL: stable_baselines3/td3/policies.py, td3/td3.py; SB3 is not installed next to the reference]:
     features   as for mcg_sac_act.
     actor      actor.mu = Sequential(Linear, act, ..., Linear(A), Tanh): n_pi layers x -> act(W x + b), one linear head z [A], and
                mean = (float)tanh((double)z), rounded once; float32 otherwise (v_mfma_f32_16x16x4_f32).  actor_target: a second one.
     critics    qf0 (and qf1 where n_critics = 2) on cat(features, action), as SAC's; critic_target a second set.
     noise      eps as mcg_sac_act draws it (the same counter layout and Box-Muller, rounded to float32 once), with dom = 10 and
                id = env_id_offset + env for mcg_td3_act, dom = 11 and id = the sample's index for mcg_td3_target; scaled in float32
                as sigma * eps, the product rounded once.  sigma == 0: the noise is +0.0f and nothing is drawn; the caller's call
                number advances all the same, so that switching sigma does not shift later draws.
     one step   n_updates += 1;  n = clamp(sigma eps, -c, c);  a' = clamp(actor_target(next_obs) + n, -1, 1);
                y = r + (1 - done) gamma min_k critic_target_k(next_obs, a')                                      mcg_td3_target
                critic_loss = sum_k mean((q_k(obs, a) - y)^2): dq_k = 2 (q_k - y) / B; Adam on `critic`           mcg_td3_critic_grad, mcg_sac_adam
                every policy_delay-th step: actor_loss = -mean(qf0(obs, actor(obs))) through qf0 alone, as just updated, a constant
                here; Adam on `actor` with the count of actor updates as its step;                                mcg_td3_actor_grad, mcg_sac_adam
                then critic_target and actor_target step towards critic and actor by tau                          mcg_td3_polyak
   Rows past the count of the last tile of 16 read the last row and store nothing; a row of the outputs depends on that row alone.
   Checked on the host before any HIP call (MCG_ERR_ARG, each with a message that names the field): a null mcg_td3; a null blob among
   those the entry touches (mcg_td3_act: actor; mcg_td3_q: the one `which` names; mcg_td3_target: actor_target and critic_target;
   mcg_td3_polyak: all four; mcg_td3_critic_grad: critic; mcg_td3_actor_grad: actor and critic), or one that is not 16-byte aligned;
   obs_dim or act_dim < 1; obs_dim > 4096; act_dim > 16; n_pi or n_qf outside [1, 3]; a width that is no multiple of 16 in [16, 256]
   (SB3's TD3 / DDPG default [400, 300] is this case); n_critics other than 1 or 2; an activation other than MCG_POLICY_TANH /
   MCG_POLICY_RELU; actor_floats or critic_floats other than mcg_td3_blob_floats gives; and what each entry lists below. */
#define MCG_TD3_CRITIC 0
#define MCG_TD3_CRITIC_TARGET 1

typedef struct mcg_td3 {
  const float* actor;               /* device, 16-byte aligned, actor_floats floats: the trunk's layers, then the head (A rows padded to 16) */
  float* actor_target;              /* likewise; written by mcg_td3_polyak alone */
  const float* critic;              /* device, 16-byte aligned, critic_floats floats: qf0, then qf1 where n_critics = 2 (mcg_sac's layout) */
  float* critic_target;             /* likewise; written by mcg_td3_polyak alone */
  int32_t n_envs, obs_dim, act_dim; /* n_envs: rows of mcg_td3_act (the other entries take their rows per call) */
  int32_t n_pi, pi_width[3];        /* the actor's trunk: 1..3 layers, widths multiples of 16, at most 256 */
  int32_t n_qf, qf_width[3];        /* each critic likewise */
  int32_t activation;               /* MCG_POLICY_TANH or MCG_POLICY_RELU */
  int32_t n_critics;                /* 2: TD3; 1: DDPG */
  int64_t actor_floats, critic_floats;      /* must equal what mcg_td3_blob_floats gives for this shape */
} mcg_td3;

typedef struct mcg_td3_act_out {    /* device pointers, float32; all but action may be NULL to skip */
  float* action;         /* [N, A]  required */
  float* mean;           /* [N, A]  the actor's output, tanh of the head */
  float* noise;          /* [N, A]  noise_std * eps */
} mcg_td3_act_out;

typedef struct mcg_td3_target_out { /* device pointers, float32; all but target may be NULL to skip */
  float* target;         /* [B]     required */
  float* next_action;    /* [B, A]  a' */
  float* next_q;         /* [n_critics, B]  the target critics at (next_obs, a'), before the min */
  float* noise;          /* [B, A]  n, after the clip */
} mcg_td3_target_out;

typedef struct mcg_td3_actor_grad_out {     /* device pointers, float32; any may be NULL to skip (the struct's pointer too) */
  float* action;         /* [B, A]  a = actor(obs) */
  float* q_pi;           /* [B]     qf0(obs, a) */
  float* dq_da;          /* [B, A]  qf0's dQ/da */
} mcg_td3_actor_grad_out;

/* actor_floats + critic_floats, and the two through the pointers (either may be NULL); 0, and zeros, for a refused shape. */
int64_t mcg_td3_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int n_critics,
                            int64_t* actor_floats, int64_t* critic_floats);

/* The collection action  action = fminf(fmaxf(mean + noise, -1), 1), the sum rounded to float32 once [RECALL: NormalActionNoise with
   mean 0, then the clip of OffPolicyAlgorithm._sample_action]; noise_std = 0 is what scripts/train.py does (it passes no action
   noise).  `obs` is what mcg_reset / mcg_step wrote (float64, read in place and rounded to float32).  One launch, one wave per tile
   of 16 environments.  Also refused: n_envs < 1 or >= 2^27; a null mcg_step_out or obs / achieved_goal / desired_goal in it; a
   noise_std that is negative or not finite; a null mcg_td3_act_out or a null action. */
int mcg_td3_act(const mcg_td3* td3, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset, float noise_std,
                const mcg_td3_act_out* out, void* stream);

/* The critics of the blob `which` names on B rows: q[0 .. B) is qf0, and with two critics q[B .. 2 B) is qf1.  One launch, one wave
   per (tile, critic).  Also refused: `which` other than the two above; B < 1 or >= 2^27; a null mcg_sac_rows or field of it; a null q. */
int mcg_td3_q(const mcg_td3* td3, int which, const mcg_sac_rows* rows, int64_t B, float* q /* [n_critics, B] */, void* stream);

/* The smoothed TD target as one launch, in float32:
     n = fminf(fmaxf(sigma * eps, -clip), clip);   a' = fminf(fmaxf(mean' + n, -1), 1), mean' = actor_target(next_obs);
     target = fmaf((1 - done) * gamma, min_k q_k, reward), q_k = critic_target_k(next_obs, a')      (the product rounded to float32
   before the fmaf, as mcg_sac_target's; with one critic the min is q_0).  A workgroup of n_critics waves per tile of 16 samples.
   Read of `batch` as mcg_sac_target reads it.  Also refused: B < 1 or >= 2^27; a null batch or one of the five fields; gamma outside
   [0, 1]; a sigma or clip that is negative or not finite; a null mcg_td3_target_out or a null target. */
int mcg_td3_target(const mcg_td3* td3, const mcg_her_batch* batch, int64_t B, uint64_t seed, uint64_t call, float gamma, float sigma,
                   float clip, const mcg_td3_target_out* out, void* stream);

/* critic_target <- (1 - tau) critic_target + tau critic and actor_target <- (1 - tau) actor_target + tau actor, each by
   mcg_sac_polyak's rule, rounding by rounding, the tau = 1 copy included.  Two launches.  Also refused: tau outside [0, 1];
   critic == critic_target; actor == actor_target. */
int mcg_td3_polyak(const mcg_td3* td3, double tau, void* stream);

int64_t mcg_td3_grad_work_floats(const mcg_td3* td3, int64_t B);          /* scratch of both gradient entries; 0 for a refused shape or B */

/* The critic loss sum_k mean((q_k - y)^2) and its gradient over the whole critic blob; dq_k = (2 (q_k - y)) * (float)(1 / B), the
   doubling exact.  `rows`: obs, achieved, desired, action [B, .]; y [B]: the TD target.
   grad   [critic_floats], 16-byte aligned, in the blob's own layout; every padding position is written +0.0f.
   stats  [8]: [0] critic_loss, [2] mean(q0), [3] mean(q1) (0 with one critic), [5], [6], [7] 0 are written; [1] and [4] are left.
   work   scratch, 16-byte aligned; its content before the call does not matter.
   Reads `critic` alone of the blobs.  Three launches: a wave per (tile, critic), the dW blocks per part, the sum in part order.
   Also refused: B < 1 or >= 2^27; a null mcg_sac_rows or field of it; a null y or stats; a null or misaligned grad or work;
   work_floats below what this entry needs. */
int mcg_td3_critic_grad(const mcg_td3* td3, const mcg_sac_rows* rows, const float* y, int64_t B, float* work, int64_t work_floats,
                        float* grad, float* stats, void* stream);

/* The actor loss -mean(qf0(obs, actor(obs))) and its gradient with respect to the actor blob alone: per component, with a = tanh(z),
     d/dz = (float)(-(double)dQ/da (1 - a^2) / B)      (in double from the float32 values, rounded once).
   `rows`: obs, achieved, desired (action is not read).  qf1 is not read.
   grad   [actor_floats], 16-byte aligned, the blob's layout; padding (feature columns from D + 6, head rows from A) is +0.0f.
   stats  [1] actor_loss, [4] mean(q_pi) are written; the others are left.
   Reads `actor` and `critic`; writes neither, nor a target.  Three launches: a wave per tile (the actor forward, the qf0 forward,
   the walk back to the action columns, the head, the walk back through the actor), the dW blocks per part, the sum in part order.
   Also refused: as mcg_td3_critic_grad, without y and rows->action. */
int mcg_td3_actor_grad(const mcg_td3* td3, const mcg_sac_rows* rows, int64_t B, float* work, int64_t work_floats, float* grad, float* stats,
                       const mcg_td3_actor_grad_out* out, void* stream);

/* ---- The CNN actor-critic forward for the -v1 picture ids (SB3's CnnPolicy = ActorCriticCnnPolicy for a Box(0, 255, (C, S, S), uint8):
   a NatureCNN features extractor shared by actor and critic, net_arch = [], a DiagGaussianDistribution; mcg_cnn.hip).  Stateless: the
   caller owns the weights (one float32 device blob, laid out as mcg_cnn.hip's head states and mycobotgym_amd/cnn_policy.py packs it),
   the scratch and the call number.  Two launches on `stream` (the convolutions, one workgroup per few pictures; the dense stage on
   tiles of 32 rows), no synchronisation, no atomics.  Additive: MCG_ABI_VERSION stays 8.
     input      x = (float)byte / 255.0f (IEEE division), or the float32 already divided (mcg_rollout_img_gather's pix_f32).
     cnn        Conv2d(C, 32, 8, stride 4), Conv2d(32, 64, 4, stride 2), Conv2d(64, 64, 3, stride 1), each followed by max(., 0), no
                padding: o1 = (S - 8) / 4 + 1, o2 = (o1 - 4) / 2 + 1, o3 = o2 - 2 (integer division); flattened as c o3^2 + y o3 + x.
     linear     features = max(W x + b, 0), [rows, F];  heads: mean = action_net(features) [rows, A], value = value_net(features) [rows].
                float32 throughout (v_mfma_f32_16x16x4_f32; the order of a sum over k is the kernel's).
     noise      as mcg_policy_forward's, with the domain byte 12: counter ((uint32)gid, (uint32)call, pair ^ ((uint32)(call >> 32) << 8),
                12 ^ ((uint32)(gid >> 32) << 8)); Box-Muller in double, rounded to float32 once.
     action, log_prob (forward), log_prob, entropy (evaluate): the formulas of mcg_policy_forward and mcg_policy_evaluate.
   A row of the outputs depends on its own picture and its global id alone.
   Accepted: channels in [1, 16], image_size in [36, 96], features_dim a multiple of 16 in [16, 512], act_dim in [1, 16]. */
#define MCG_CNN_UINT8 0
#define MCG_CNN_FLOAT32 1

typedef struct mcg_cnn_policy {
  const float* blob;                /* device, 16-byte aligned, blob_floats floats */
  float* scratch;                   /* device, 16-byte aligned: the flattened conv features, [rows, 64 o3^2]; written by every call */
  int32_t n_envs, channels, image_size, features_dim, act_dim;
  int64_t blob_floats;              /* must equal mcg_cnn_blob_floats of this shape */
  int64_t scratch_floats;           /* >= mcg_cnn_scratch_floats of this shape and the call's rows */
} mcg_cnn_policy;

typedef struct mcg_cnn_obs {        /* pictures [rows, C, S, S]; only the S x S plane must be contiguous */
  const void* pixels;               /* device */
  int32_t dtype;                    /* MCG_CNN_UINT8, or MCG_CNN_FLOAT32: already divided by 255 */
  int64_t env_stride, chan_stride;  /* in elements */
} mcg_cnn_obs;

typedef struct mcg_cnn_out {        /* device pointers, any may be NULL to skip (not all) */
  float* action;         /* [N, A] */
  float* value;          /* [N] */
  float* log_prob;       /* [N] */
  float* mean;           /* [N, A] */
  float* noise;          /* [N, A]  eps */
  float* features;       /* [N, F]  the extractor's output (tests) */
} mcg_cnn_out;

/* Sizes in floats; 0 for a refused shape (scratch: or rows outside [1, 2^27)). */
int64_t mcg_cnn_blob_floats(int channels, int image_size, int features_dim, int act_dim);
int64_t mcg_cnn_scratch_floats(int channels, int image_size, int features_dim, int act_dim, int64_t rows);

/* rows = pol->n_envs.  With only `value` (and `features`) set no policy-head work is done; the caller then uses up no call number.
   Refused (MCG_ERR_ARG, each by a message that names the field): a null struct, blob or scratch; a shape outside the accepted domain;
   blob_floats or scratch_floats that do not fit; a misaligned blob or scratch; null pixels; an unknown dtype; a negative stride or a
   channel stride below S * S while channels > 1; all outputs null. */
int mcg_cnn_forward(const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, uint64_t seed, uint64_t call, int64_t env_id_offset,
                    int deterministic, const mcg_cnn_out* out, void* stream);

/* SB3's evaluate_actions, forward only, on `rows` pictures and `actions` [rows, A] (pol->n_envs is not read). */
int mcg_cnn_evaluate(const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, const float* actions, int64_t rows,
                     const mcg_policy_eval_out* out, void* stream);

/* Device self-test of the step kernels' bad-value check (mj_checkPos / mj_checkVel / mj_checkAcc at the end of a sub-step): no engine
   handle, nothing a rollout calls.  `in` is [n][MCG_SELFTEST_BAD_VALUE_IN] doubles on the device, one case per row: a[12], r[12],
   qd_old[12], q_old[12], h.  A lane forms rhs = fma(-h, r, a), qdn = fma(h, rhs, qd_old), qn = fma(h, qdn, q_old) as the Euler step
   of a sub-step does, writes qdn[12], qn[12] to state [n][24], and evaluates the check twice on those registers: each[c] = the 36
   single compares !(|x| <= 1e10) ORed, any[c] = the one maximum and one sum the three-wave Reach kernel of the joint controller uses.
   The two must be equal for every input (tests/test_gpu_reach_bad_value_tail.py holds them to that on values no state of the engine
   reaches: +-inf, NaN, 1e10 and its neighbours).  MCG_ERR_ARG for a null pointer or n outside [1, 2^20]. */
#define MCG_SELFTEST_BAD_VALUE_IN 49
int mcg_selftest_bad_value(const double* in, int n, double* state /* [n][24] device */, uint8_t* each /* [n] device */,
                           uint8_t* any /* [n] device */, void* stream);

/* Device self-test of the factor of H = H_eq + M + D that the side waves of the joint controller's three-wave Reach kernel form after
   barrier S2: no engine handle, nothing a rollout calls.  `in` is [n][MCG_SELFTEST_FACTOR_H_IN] doubles on the device, one case per
   row: H_eq[78], M[78] (packed lower triangles, tri(i, j) = i (i + 1) / 2 + j; only the patterns' nonzeros are read), D[10] and
   act[10] of the limit rows (act != 0: D is added to the row's diagonal), b[12].  A lane puts H_eq and M into its LDS column, where
   the kernel keeps them, and factors and solves H x = b twice from there: by build_H + ldl_factor, the route of the main wave and of
   every other kernel, and by build_factor_H, the side waves' row-by-row route.  out is [n][MCG_SELFTEST_FACTOR_H_OUT]: L[78] (unit
   lower multipliers, D on the diagonal, zero off the pattern), dinv[12], x[12] of the first route, then the same of the second.  The
   two must agree bit for bit (tests/test_gpu_reach_factor_order.py).  MCG_ERR_ARG for a null pointer or n outside [1, 2^20]. */
#define MCG_SELFTEST_FACTOR_H_IN 188
#define MCG_SELFTEST_FACTOR_H_OUT 204
int mcg_selftest_factor_h(const double* in, int n, double* out, void* stream);

#ifdef __cplusplus
}
#endif
#endif
