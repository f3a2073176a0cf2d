// mcg_rollout.hip -- the on-policy rollout buffer (include/mcg.h: mcg_rollout_*): insertion with the time-limit bootstrap, the advantage
// recursion (GAE) and the shuffled minibatch gather on the device.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives: the step, render and replay kernels' code
// objects stay laid out as they are without this file.  Kernels and C entries are both here.  The C side is stateless: every call gets
// the caller's device pointers in an mcg_rollout_buf; of mcg_engine.hpp it uses the error reporting alone.
//
// A record is float32 throughout and is read and written as 4-byte words (the gather: as 8-byte pairs); Layout names the words.
#include <hip/hip_runtime.h>

#include <cmath>

#include "mcg.h"
#include "mcg_buffer.hpp"        // what the replay buffer has too: launched, record_bytes, carry, copy_phase; philox4x32_10

using namespace mcg;

namespace {

constexpr int ROLLOUT_STREAM = 4;       // Philox stream of the permutation (0: goals, 1: mass and friction, 2: pictures, 3: HER)
constexpr int FEISTEL_ROUNDS = 4;
constexpr int ADD_LANES = 256;
constexpr int GAE_LANES = 64;           // lane = environment and nothing is shared: one wave per block spreads 8192 environments over 128 CUs

struct Layout {                          // word indices inside a record: obs at 0
  int D, A, w_ach, w_des, w_act, w_logp, words;
};
Layout layout(int D, int A) {
  Layout L;
  L.D = D; L.A = A;
  L.w_ach = D; L.w_des = D + 3; L.w_act = D + 6; L.w_logp = L.w_act + A;
  L.words = padded_words(L.w_logp + 1);
  return L;
}

struct Roll {                            // mcg_rollout_buf as the kernels see it
  uint32_t* rec; float *rew, *val, *adv, *ret, *last_obs, *last_goals; uint8_t *start, *last_start;
  int n, T;
  float g32, c32;                        // (float)gamma, (float)(gamma * gae_lambda)
  Layout L;
};

// ------------------------------------------------------------------------------------------------------------ start
__global__ __launch_bounds__(ADD_LANES) void rollout_start_kernel(Roll B, const double* __restrict__ obs, const double* __restrict__ ach,
                                                                  const double* __restrict__ des, const uint8_t* __restrict__ mask) {
  const int per = B.L.D + 7;             // obs[D], achieved[3], desired[3], last_start
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x;
  if (x >= (long long)B.n * per) return;
  const int e = (int)(x / per), j = (int)(x % per), D = B.L.D;
  if (mask && mask[e] == 0) return;
  if (j < D) B.last_obs[(size_t)e * D + j] = (float)obs[(size_t)e * D + j];
  else if (j < D + 3) B.last_goals[e * 6 + (j - D)] = (float)ach[e * 3 + (j - D)];
  else if (j < D + 6) B.last_goals[e * 6 + (j - D)] = (float)des[e * 3 + (j - D - 3)];
  else B.last_start[e] = 1;
}

// -------------------------------------------------------------------------------------------------------------- add
// Lane = one word of one environment's record, and one more lane per environment for the plane row; environments are neighbours in
// a step's row, so the grid writes one contiguous run.  Every element of last_obs / last_goals / last_start has one lane, which reads
// it and then overwrites it.
__global__ __launch_bounds__(ADD_LANES) void rollout_add_kernel(Roll B, int pos, const float* __restrict__ actions,
                                                                const float* __restrict__ values, const float* __restrict__ log_probs,
                                                                const float* __restrict__ final_values, mcg_step_out O) {
#pragma clang fp contract(off)
  const Layout& L = B.L;
  const int elems = L.words + 1;
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x;
  if (x >= (long long)B.n * elems) return;
  const int e = (int)(x / elems), w = (int)(x % elems);
  const size_t at = (size_t)pos * B.n + e;
  if (w == L.words) {                    // the plane row, and the one writer of last_start
    const bool term = O.terminated[e] != 0, trunc = O.truncated[e] != 0;
    float r = (float)O.reward[e];
    if (final_values && trunc && !term) {          // [RECALL] SB3 collect_rollouts: rewards[idx] += gamma * terminal_value
      const float boot = B.g32 * final_values[e];
      r = r + boot;
    }
    B.rew[at] = r;
    B.val[at] = values[e];
    B.start[at] = B.last_start[e];
    B.last_start[e] = (term || trunc) ? 1 : 0;
    return;
  }
  uint32_t bits = 0;
  if (w < L.w_ach) {
    const size_t a = (size_t)e * L.D + w;
    bits = carry(B.last_obs[a], O.obs[a]);
  } else if (w < L.w_act) {
    const int c = w - L.w_ach;           // 0..2 achieved, 3..5 desired
    bits = carry(B.last_goals[e * 6 + c], c < 3 ? O.achieved_goal[e * 3 + c] : O.desired_goal[e * 3 + (c - 3)]);
  } else if (w < L.w_logp) {
    bits = __float_as_uint(actions[(size_t)e * L.A + (w - L.w_act)]);
  } else if (w == L.w_logp) {
    bits = __float_as_uint(log_probs[e]);
  }
  B.rec[at * L.words + w] = bits;
}

// -------------------------------------------------------------------------------------------------------------- gae
// Lane = environment, a backward loop over the host value T, plane rows coalesced.  The three loads of step t - 1 are issued before the
// arithmetic of step t; the dependent chain per step is (c32 * nnt) * last, + delta: the other products do not wait for `last`.
__global__ __launch_bounds__(GAE_LANES) void rollout_gae_kernel(Roll B, const float* __restrict__ last_values) {
#pragma clang fp contract(off)
  const int e = blockIdx.x * GAE_LANES + threadIdx.x;
  if (e >= B.n) return;
  const size_t N = (size_t)B.n;
  float vn = last_values[e];
  float nnt = 1.0f - (float)B.last_start[e];
  size_t at = (size_t)(B.T - 1) * N + e;
  float r = B.rew[at], v = B.val[at];
  uint8_t s = B.start[at];
  float last = 0.0f;
  for (int t = B.T - 1; t >= 0; t--) {
    float r1 = 0.0f, v1 = 0.0f;
    uint8_t s1 = 0;
    if (t > 0) { r1 = B.rew[at - N]; v1 = B.val[at - N]; s1 = B.start[at - N]; }
    const float boot = (B.g32 * vn) * nnt;
    const float delta = (r + boot) - v;
    const float keep = B.c32 * nnt;
    last = delta + keep * last;
    B.adv[at] = last;
    B.ret[at] = last + v;
    vn = v; nnt = 1.0f - (float)s;       // episode_start[t] is start_next of step t - 1
    r = r1; v = v1; s = s1;
    at -= N;                             // (wraps below row 0 after the last pass; not used then)
  }
}

// ----------------------------------------------------------------------------------------------------------- gather
struct Batch { float *obs, *ach, *des, *act, *val, *logp, *adv, *ret; int32_t* index; };

// one 4-byte word of a record to its place in row j of the outputs
MCG_DEV void emit_word(const Layout& L, const Batch& O, int j, int w, uint32_t bits) {
  const float f = __uint_as_float(bits);
  if (w < L.w_ach) { if (O.obs) O.obs[(size_t)j * L.D + w] = f; }
  else if (w < L.w_des) { if (O.ach) O.ach[(size_t)j * 3 + (w - L.w_ach)] = f; }
  else if (w < L.w_act) { if (O.des) O.des[(size_t)j * 3 + (w - L.w_des)] = f; }
  else if (w < L.w_logp) { if (O.act) O.act[(size_t)j * L.A + (w - L.w_act)] = f; }
  else if (w == L.w_logp) { if (O.logp) O.logp[j] = f; }
}

__global__ __launch_bounds__(SAMPLE_LANES) void rollout_gather_kernel(Roll B, unsigned long long seed, unsigned long long epoch, int first,
                                                                      int count, int h, Batch O) {
  const Layout& L = B.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int j0 = (blockIdx.x * (SAMPLE_LANES / 64) + wave) * SPW;       // wave-uniform; first output row of this wave
  if (j0 >= count) return;
  // ---- index phase: lane i < SPW walks position first + j0 + i through the Feistel network until it lands below M
  const uint32_t M = (uint32_t)B.n * (uint32_t)B.T;                     // < 2^31 (host check)
  const uint32_t half = (1u << h) - 1u;
  const uint32_t c1 = (uint32_t)epoch, c3 = (uint32_t)ROLLOUT_STREAM ^ ((uint32_t)(epoch >> 32) << 8);
  const int j = j0 + lane;
  const bool mine = lane < SPW && j < count;
  uint32_t x = mine ? (uint32_t)first + (uint32_t)j : 0u;
  bool need = mine;
  do {                                   // wave-uniform, per-lane effects predicated on `need`; ends because a bijection's cycles close
    uint32_t Lh = x >> h, Rh = x & half;
#pragma unroll
    for (int r = 0; r < FEISTEL_ROUNDS; r++) {
      uint32_t w[4];
      philox4x32_10(Rh, c1, (uint32_t)r, c3, (uint32_t)seed, (uint32_t)(seed >> 32), w);
      const uint32_t nr = Lh ^ (w[0] & half);
      Lh = Rh; Rh = nr;
    }
    if (need) x = (Lh << h) | Rh;
    need = need && x >= M;
  } while (__any(need));
  const int src = (int)((size_t)(x % (uint32_t)B.T) * B.n + x / (uint32_t)B.T);      // row of i = e * T + t in the [T, N] planes; < M
  if (mine) {                            // the three plane words of a sample: scattered 4-byte loads
    const float v = B.val[src], a = B.adv[src], g = B.ret[src];
    if (O.val) O.val[j] = v;
    if (O.adv) O.adv[j] = a;
    if (O.ret) O.ret[j] = g;
    if (O.index) O.index[j] = (int32_t)x;
  }
  // ---- copy phase
  copy_phase(lane, j0, count, L.words / 2,
    [&](int, int i, int p) { return B.rec + (size_t)__builtin_amdgcn_readlane(src, i) * L.words + 2 * p; },
    [&](int, int row, int p, uint2 v) {
      emit_word(L, O, row, 2 * p, v.x);
      emit_word(L, O, row, 2 * p + 1, v.y);
    });
}

// ------------------------------------------------------------------------------------------------------- host side
int check_buf(const mcg_rollout_buf* b, const char* who) {
  if (!b) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_rollout_buf", who);
  if (!b->records || !b->reward || !b->value || !b->episode_start || !b->advantage || !b->returns || !b->last_obs || !b->last_goals ||
      !b->last_start)
    return mcg_fail(MCG_ERR_ARG, "%s: null pointer in mcg_rollout_buf", who);
  if (b->n_envs < 1 || b->obs_dim < 1 || b->act_dim < 1 || b->n_steps < 1)
    return mcg_fail(MCG_ERR_ARG, "%s: n_envs, obs_dim, act_dim and n_steps must be >= 1", who);
  if ((long long)b->n_steps * b->n_envs >= (1ll << 31)) return mcg_fail(MCG_ERR_ARG, "%s: n_steps * n_envs must be below 2^31", who);
  if (((uintptr_t)b->records & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: records is not 16-byte aligned", who);
  if (!std::isfinite(b->gamma) || !std::isfinite(b->gae_lambda) || b->gamma < 0.0 || b->gamma > 1.0 || b->gae_lambda < 0.0 ||
      b->gae_lambda > 1.0)
    return mcg_fail(MCG_ERR_ARG, "%s: gamma and gae_lambda must be finite and in [0, 1]", who);
  return MCG_OK;
}

Roll view(const mcg_rollout_buf* b) {
  Roll B;
  B.rec = static_cast<uint32_t*>(b->records); B.rew = b->reward; B.val = b->value; B.adv = b->advantage; B.ret = b->returns;
  B.last_obs = b->last_obs; B.last_goals = b->last_goals; B.start = b->episode_start; B.last_start = b->last_start;
  B.n = b->n_envs; B.T = b->n_steps;
  B.g32 = (float)b->gamma; B.c32 = (float)(b->gamma * b->gae_lambda);
  B.L = layout(b->obs_dim, b->act_dim);
  return B;
}

}  // namespace

extern "C" {

int64_t mcg_rollout_record_bytes(int obs_dim, int act_dim) {
  return record_bytes(obs_dim, act_dim, layout(obs_dim, act_dim).words);
}

int mcg_rollout_start(const mcg_rollout_buf* buf, const mcg_step_out* first, const uint8_t* mask, void* stream) {
  if (const int rc = check_buf(buf, "mcg_rollout_start")) return rc;
  if (!first) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_start: null mcg_step_out");
  if (!first->obs || !first->achieved_goal || !first->desired_goal)
    return mcg_fail(MCG_ERR_ARG, "mcg_rollout_start: obs, achieved_goal and desired_goal of the reset's output are required");
  const Roll B = view(buf);
  const long long total = (long long)B.n * (B.L.D + 7);
  hipLaunchKernelGGL(rollout_start_kernel, dim3(blocks(total, ADD_LANES)), dim3(ADD_LANES), 0, (hipStream_t)stream,
                     B, first->obs, first->achieved_goal, first->desired_goal, mask);
  return launched("mcg_rollout");
}

int mcg_rollout_add(const mcg_rollout_buf* buf, int pos, const float* actions, const float* values, const float* log_probs,
                    const float* final_values, const mcg_step_out* out, void* stream) {
  if (const int rc = check_buf(buf, "mcg_rollout_add")) return rc;
  if (pos < 0 || pos >= buf->n_steps) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: pos outside [0, n_steps)");
  if (!actions) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: null actions");
  if (!values) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: null values");
  if (!log_probs) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: null log_probs");
  if (!out) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: null mcg_step_out");
  if (!out->obs || !out->achieved_goal || !out->desired_goal || !out->reward || !out->terminated || !out->truncated)
    return mcg_fail(MCG_ERR_ARG, "mcg_rollout_add: obs, achieved_goal, desired_goal, reward, terminated and truncated of the step's output are required");
  const Roll B = view(buf);
  const long long total = (long long)B.n * (B.L.words + 1);
  hipLaunchKernelGGL(rollout_add_kernel, dim3(blocks(total, ADD_LANES)), dim3(ADD_LANES), 0, (hipStream_t)stream,
                     B, pos, actions, values, log_probs, final_values, *out);
  return launched("mcg_rollout");
}

int mcg_rollout_gae(const mcg_rollout_buf* buf, const float* last_values, void* stream) {
  if (const int rc = check_buf(buf, "mcg_rollout_gae")) return rc;
  if (!last_values) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gae: null last_values");
  const Roll B = view(buf);
  hipLaunchKernelGGL(rollout_gae_kernel, dim3(blocks(B.n, GAE_LANES)), dim3(GAE_LANES), 0, (hipStream_t)stream,
                     B, last_values);
  return launched("mcg_rollout");
}

int mcg_rollout_gather(const mcg_rollout_buf* buf, uint64_t seed, uint64_t epoch, int64_t first, int64_t count,
                       const mcg_rollout_batch* out, void* stream) {
  if (const int rc = check_buf(buf, "mcg_rollout_gather")) return rc;
  const int64_t M = (int64_t)buf->n_steps * buf->n_envs;
  if (first < 0) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gather: first < 0");
  if (count < 1) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gather: count must be >= 1");
  if (first > M || count > M - first) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gather: first + count > n_steps * n_envs");
  if (!out) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gather: null mcg_rollout_batch");
  if (!out->obs && !out->achieved && !out->desired && !out->action && !out->old_value && !out->old_log_prob && !out->advantage &&
      !out->returns && !out->index)
    return mcg_fail(MCG_ERR_ARG, "mcg_rollout_gather: all outputs are null");
  int b = 2;
  while ((1ll << b) < M) b += 2;         // the smallest even b >= 2 with 2^b >= M; M < 2^31, so b <= 32
  const Roll B = view(buf);
  const Batch O = {out->obs, out->achieved, out->desired, out->action, out->old_value, out->old_log_prob, out->advantage, out->returns, out->index};
  hipLaunchKernelGGL(rollout_gather_kernel, dim3(blocks(count, SAMPLES_PER_BLOCK)), dim3(SAMPLE_LANES), 0,
                     (hipStream_t)stream, B, (unsigned long long)seed, (unsigned long long)epoch, (int)first, (int)count, b / 2, O);
  return launched("mcg_rollout");
}

}  // extern "C"
