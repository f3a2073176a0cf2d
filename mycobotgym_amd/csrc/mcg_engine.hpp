// mcg_engine.hpp -- what mcg_hip.hip, mcg_render.hip and, through mcg_buffer.hpp, mcg_replay.hip and mcg_rollout.hip share on the host side: error reporting, the layout of an engine's
// state, its two kernel-parameter views (Cfg, View) and the handle behind the C ABI (mcg_env).  Internal: include/mcg.h is the boundary.
#pragma once

#include <hip/hip_runtime.h>
#include <cmath>
#include <cstdint>
#include <vector>

#include "mcg.h"

namespace mcg {

// Writes the calling thread's message, the one mcg_last_error() hands out, and returns `code`.  Defined in mcg_hip.hip, next to the buffer.
__attribute__((format(printf, 2, 3))) int mcg_fail(int code, const char* fmt, ...);
#define HIP_OK(expr) do { hipError_t e_ = (expr); if (e_ != hipSuccess) return mcg::mcg_fail(MCG_ERR_HIP, #expr ": %s", hipGetErrorString(e_)); } while (0)

inline double norm3(const double* v) { return std::sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2]); }

// The float64 state of an engine is struct-of-arrays: rows of n doubles (n fastest), field after field.  The first row of each field:
// qpos[nq] qvel[nv] ctrl[7] warm[nv] qlag[nq] goal[3] ep_return[1] dr[2].  (mcg_state in include/mcg.h is the caller's view of the same fields.)
struct StateRows { int qpos, qvel, ctrl, warm, qlag, goal, ep_return, dr; };
__host__ __device__ constexpr StateRows state_rows(int nq, int nv) { return {0, nq, nq + nv, nq + nv + 7, nq + 2 * nv + 7, 2 * nq + 2 * nv + 7, 2 * nq + 2 * nv + 10, 2 * nq + 2 * nv + 11}; }
constexpr int state_doubles(int nq, int nv) { return state_rows(nq, nv).dr + 2; }

// mcg_render.hip: the ray caster's face table of a checked polytope block, into e->faces_host and e->foff (host only, no HIP call)
void render_face_table(mcg_env* e, const double* polytopes);

}  // namespace mcg

// Kernel parameter types: in an unnamed namespace, as they were inside mcg_hip.hip, so that the kernels' mangled names stay what they are.
namespace {

struct Cfg {
  int n, has_object, controller, fetch, reward_type, frame_skip, control_steps, max_episode_steps;
  int target_in_the_air, auto_reset, nq, nv, obs_dim, act_dim, dr_enable, block_gripper;
  int coop_pair;         // PickAndPlace: the cooperative phase solves two environments per wave (default; MCG_COOP_PAIR=0: one per wave, the first implementation)
  int hidden;            // Reach with reward_shaping: the cube stays in the physics as a hidden free body (mycobot.py:475-481)
  double dr_mass[2], dr_fric[2], qpos0_cube[7];
  double distance_threshold, height_offset, igx[3], dt, grip_center, grip_range;
  double init_qpos[19], init_qvel[18], init_ctrl[7];
  unsigned long long seed;
  long long env_id_offset;
  unsigned long long* cnt;   // device: mcg_counters (reset-cap hits, bad-state resets, contacts dropped by the cap, flagged env-sub-steps)
};

struct View {           // SoA state: row r of env i at d[r * n + i]
  double* d; int32_t* i32; int n, nq, nv;
  __host__ __device__ mcg::StateRows rows() const { return mcg::state_rows(nq, nv); }
  double* row(int r) const { return d + (size_t)r * n; }      // host: a field's rows as the [dim, N] array a kernel takes
  __device__ double& qpos(int k, int i) const { return d[(size_t)(rows().qpos + k) * n + i]; }
  __device__ double& qvel(int k, int i) const { return d[(size_t)(rows().qvel + k) * n + i]; }
  __device__ double& ctrl(int k, int i) const { return d[(size_t)(rows().ctrl + k) * n + i]; }
  __device__ double& warm(int k, int i) const { return d[(size_t)(rows().warm + k) * n + i]; }
  __device__ double& qlag(int k, int i) const { return d[(size_t)(rows().qlag + k) * n + i]; }
  __device__ double& goal(int k, int i) const { return d[(size_t)(rows().goal + k) * n + i]; }
  __device__ double& epret(int i) const { return d[(size_t)rows().ep_return * n + i]; }
  __device__ double& dr(int k, int i) const { return d[(size_t)(rows().dr + k) * n + i]; }
  __device__ int32_t& elapsed(int i) const { return i32[i]; }
  __device__ int32_t& episode(int i) const { return i32[n + i]; }
  __device__ int32_t& eplen(int i) const { return i32[2 * n + i]; }
};

}  // namespace

struct mcg_env {      // the handle behind the C ABI
  Cfg cfg;
  View view;
  mcg_model* d_model;
  double* d_poly;                 // the mesh geoms' collision tables (mcg_create: polytopes)
  unsigned long long* d_cnt;      // mcg_counters
  int device;
  int num_cu;
  float4* d_faces;     // the ray caster: the polytopes' face planes as float32 (n, d), mesh by mesh, each range padded to a multiple of four;
  std::vector<float> faces_host;      // made at mcg_create (render_face_table), uploaded by the first picture (an engine that never draws allocates nothing for it)
  int foff[MCG_NMESH + 1];
  bool render_ok;      // false: created from a caller's model that the polytope block at hand does not fit (render_why)
  char render_why[200];
  bool no_split;       // MCG_NO_SPLIT=1 in the environment at mcg_create: always the one-wave REACH kernels (tests, A/B timing)
};
