// mcg_replay.hip -- the hindsight replay buffer (include/mcg.h: mcg_her_*): insertion and `future`-strategy sampling on the device.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives: the step kernels' code object stays laid
// out as it is without this file.  Kernels and C entries are both here.  The C side is stateless: every call gets the caller's device
// pointers in an mcg_her_buf; of mcg_engine.hpp it uses the error reporting alone.
//
// A record is read and written as 4-byte words (the nine float64 goals, words 0-17, as 8-byte pairs); W_* below name the words.
#include <hip/hip_runtime.h>

#include "mcg.h"
#include "mcg_buffer.hpp"        // what the rollout buffer has too: launched, record_bytes, carry, copy_phase; philox_pair

using namespace mcg;

namespace {

constexpr int GOAL_WORDS = 18;          // achieved[3], next_achieved[3], desired[3] as doubles
constexpr int HER_MAX_DRAWS = 256;      // rejection draws per sample; draw HER_MAX_DRAWS picks the future step
constexpr int ADD_LANES = 256;

struct Layout {                          // word indices inside a record
  int D, A, w_nobs, w_act, w_rew, w_t, w_len, w_term, words;
};
Layout layout(int D, int A) {
  Layout L;
  L.D = D; L.A = A;
  L.w_nobs = GOAL_WORDS + D; L.w_act = L.w_nobs + D; L.w_rew = L.w_act + A;
  L.w_t = L.w_rew + 1; L.w_len = L.w_rew + 2; L.w_term = L.w_rew + 3;
  L.words = padded_words(L.w_term + 1);
  return L;
}

struct Her {                             // mcg_her_buf as the kernels see it
  uint32_t* rec; int32_t* t_run; float* last_obs; double* last_ach; unsigned long long* cnt;
  int n, cap, max_steps, reward_type;
  double thr;
  Layout L;
};

MCG_DEV int clampi(int x, int lo, int hi) { return x < lo ? lo : (x > hi ? hi : x); }
MCG_DEV uint32_t* record(const Her& B, int slot, int e) { return B.rec + ((size_t)slot * B.n + e) * B.L.words; }

// ------------------------------------------------------------------------------------------------------------ start
__global__ __launch_bounds__(ADD_LANES) void her_start_kernel(Her B, const double* __restrict__ obs, const double* __restrict__ ach,
                                                              const uint8_t* __restrict__ mask) {
  const int per = B.L.D + 4;             // obs[D], achieved[3], t_run
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x;
  if (x >= (long long)B.n * per) return;
  const int e = (int)(x / per), j = (int)(x % per);
  if (mask && mask[e] == 0) return;
  if (j < B.L.D) B.last_obs[(size_t)e * B.L.D + j] = (float)obs[(size_t)e * B.L.D + j];
  else if (j < B.L.D + 3) B.last_ach[e * 3 + (j - B.L.D)] = ach[e * 3 + (j - B.L.D)];
  else B.t_run[e] = 0;
}

// -------------------------------------------------------------------------------------------------------------- add
// A block takes `epb` whole environments, lane = record element (a float64 goal or a 4-byte word): the environments of a slot are
// neighbours in memory, so a block writes one contiguous run.  Every reader of an environment's t_run sits in its block and reads
// it (into LDS) before the barrier; the one writer writes after it.
constexpr int ADD_MAX_EPB = 16;
__global__ __launch_bounds__(ADD_LANES) void her_add_kernel(Her B, int pos, int epb, const float* __restrict__ actions, mcg_step_out O) {
  __shared__ int s_t[ADD_MAX_EPB], s_done[ADD_MAX_EPB];
  const Layout& L = B.L;
  const int e0 = blockIdx.x * epb, tid = threadIdx.x;
  if (tid < epb && e0 + tid < B.n) {
    s_t[tid] = clampi(B.t_run[e0 + tid], 0, B.max_steps);
    s_done[tid] = (O.truncated[e0 + tid] | O.terminated[e0 + tid]) != 0;
  }
  __syncthreads();
  const int elems = 9 + (L.words - GOAL_WORDS);
  for (int x = tid; x < epb * elems; x += ADD_LANES) {
    const int le = x / elems, j = x % elems, e = e0 + le;
    if (e >= B.n) break;
    const int t = s_t[le];
    const bool done = s_done[le], whole = done && t < B.max_steps;      // an over-long episode stays abandoned when it ends
    uint32_t* rec = record(B, pos, e);
    if (j < 9) {
      const int k = j % 3;
      double v;
      if (j < 3) { v = B.last_ach[e * 3 + k]; B.last_ach[e * 3 + k] = O.achieved_goal[e * 3 + k]; }
      else if (j < 6) v = done ? O.final_achieved[e * 3 + k] : O.achieved_goal[e * 3 + k];
      else v = done ? O.final_desired[e * 3 + k] : O.desired_goal[e * 3 + k];
      reinterpret_cast<double*>(rec)[j] = v;
      continue;
    }
    const int w = GOAL_WORDS + (j - 9);
    uint32_t bits = 0;
    if (w < L.w_nobs) {
      const size_t a = (size_t)e * L.D + (w - GOAL_WORDS);
      bits = carry(B.last_obs[a], O.obs[a]);
    } else if (w < L.w_act) {
      const size_t a = (size_t)e * L.D + (w - L.w_nobs);
      bits = __float_as_uint((float)(done ? O.final_obs[a] : O.obs[a]));
    } else if (w < L.w_rew) {
      bits = __float_as_uint(actions[(size_t)e * L.A + (w - L.w_act)]);
    } else if (w == L.w_rew) {
      bits = __float_as_uint((float)O.reward[e]);
    } else if (w == L.w_t) {
      bits = (uint32_t)t;
    } else if (w == L.w_len) {
      bits = whole ? (uint32_t)(t + 1) : 0u;
      // this lane is the environment's one writer of t_run
      int t1 = 0;
      if (!done) {
        t1 = t < B.max_steps ? t + 1 : B.max_steps;                     // saturates
        if (t < B.max_steps && t1 == B.max_steps) atomicAdd(B.cnt + 1, 1ull);      // max_episode_steps transitions and no done flag
      }
      B.t_run[e] = t1;
    } else if (w == L.w_term) {
      bits = O.terminated[e] != 0 ? 1u : 0u;
    }
    rec[w] = bits;
  }
  // back-fill: the finished episode's length into its earlier slots (pos - j, j = 1..t); bounded by max_episode_steps
  for (int x = tid; x < epb * B.max_steps; x += ADD_LANES) {
    const int le = x / B.max_steps, j = x % B.max_steps + 1, e = e0 + le;
    if (e >= B.n) break;
    const int t = s_t[le];
    if (!(s_done[le] && t < B.max_steps && j <= t)) continue;
    int slot = pos - j; if (slot < 0) slot += B.cap;
    record(B, slot, e)[L.w_len] = (uint32_t)(t + 1);
  }
}

// ----------------------------------------------------------------------------------------------------------- sample
MCG_DEV void her_pair(unsigned long long seed, unsigned long long call, uint32_t k, uint32_t draw, double& u0, double& u1) {
  philox_pair(k, (uint32_t)call, draw, DOMAIN_HER ^ ((uint32_t)(call >> 32) << 8), seed, u0, u1);
}

struct Batch { float *obs, *ach, *des, *nobs, *nach, *act, *rew, *done; int32_t* index; };

// one 4-byte word of sample k's record to its place in the outputs
MCG_DEV void emit_word(const Her& B, const Batch& O, int k, int w, uint32_t bits, bool relabel, const uint32_t* rec, const uint32_t* frec) {
  const Layout& L = B.L;
  if (w < L.w_nobs) { if (O.obs) O.obs[(size_t)k * L.D + (w - GOAL_WORDS)] = __uint_as_float(bits); }
  else if (w < L.w_act) { if (O.nobs) O.nobs[(size_t)k * L.D + (w - L.w_nobs)] = __uint_as_float(bits); }
  else if (w < L.w_rew) { if (O.act) O.act[(size_t)k * L.A + (w - L.w_act)] = __uint_as_float(bits); }
  else if (w == L.w_rew) {
    float r = __uint_as_float(bits);
    if (relabel) {                       // reward_kernel's expression (mcg_hip.hip) on (next_achieved, new goal), in float64
      const double* ag = reinterpret_cast<const double*>(rec) + 3;
      const double* dg = reinterpret_cast<const double*>(frec) + 3;
      const double dx = ag[0] - dg[0], dy = ag[1] - dg[1], dz = ag[2] - dg[2];
      const double d = sqrt(dx * dx + dy * dy + dz * dz);
      r = (float)(B.reward_type == MCG_REWARD_SPARSE ? -(double)(float)(d > B.thr) : -d);
    }
    if (O.rew) O.rew[k] = r;
  }
  else if (w == L.w_term) { if (O.done) O.done[k] = (float)(bits & 0xffu); }
}

__global__ __launch_bounds__(SAMPLE_LANES) void her_sample_kernel(Her B, long long n_written, unsigned long long seed, unsigned long long call,
                                                                  int batch, int n_virtual, Batch O) {
  const Layout& L = B.L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int k0 = (blockIdx.x * (SAMPLE_LANES / 64) + wave) * SPW;       // wave-uniform
  if (k0 >= batch) return;
  // ---- index phase: lane i < SPW draws sample k0 + i
  const int k = k0 + lane;
  const int Wn = (int)(n_written < B.cap ? n_written : B.cap);
  const int pos = (int)(n_written % B.cap);
  const long long oldest = n_written > B.cap ? n_written - B.cap : 0;
  bool need = lane < SPW && k < batch && Wn > 0;
  bool gave_up = lane < SPW && k < batch && Wn == 0;
  int s = -1, e = -1, t = 0, len = 0;
  for (int d = 0; d < HER_MAX_DRAWS && __any(need); d++) {               // wave-uniform, per-lane effects predicated on `need`
    double u0, u1;
    her_pair(seed, call, (uint32_t)k, (uint32_t)d, u0, u1);
    int cs = (int)floor(u0 * (double)Wn); cs = cs > Wn - 1 ? Wn - 1 : cs;
    int ce = (int)floor(u1 * (double)B.n); ce = ce > B.n - 1 ? B.n - 1 : ce;
    int ct = 0, cl = 0;
    if (need) {
      const uint32_t* rec = record(B, cs, ce);
      ct = clampi((int)rec[L.w_t], 0, B.max_steps);
      cl = clampi((int)rec[L.w_len], 0, B.max_steps);
    }
    int back = pos - 1 - cs; if (back < 0) back += B.cap;
    const long long a = n_written - 1 - back;
    const bool ok = need && cl > 0 && a - ct >= oldest;
    if (ok) { s = cs; e = ce; t = ct; len = cl; }
    need = need && !ok;
  }
  gave_up = gave_up || need;
  if (__any(gave_up)) { if (gave_up) atomicAdd(B.cnt, 1ull); }
  int fs = -1;
  const bool is_virtual = lane < SPW && k < batch && k >= batch - n_virtual && s >= 0;
  if (__any(is_virtual)) {
    double u0, u1;
    her_pair(seed, call, (uint32_t)k, (uint32_t)HER_MAX_DRAWS, u0, u1);
    int f = t + (int)floor(u0 * (double)(len - t));
    f = f > len - 1 ? len - 1 : f;
    int slot = (s + f - t) % B.cap; if (slot < 0) slot += B.cap;          // |f - t| <= max_episode_steps <= capacity / 2
    if (is_virtual) fs = slot;
  }
  if (lane < SPW && k < batch && O.index) { O.index[(size_t)k * 3] = s; O.index[(size_t)k * 3 + 1] = e; O.index[(size_t)k * 3 + 2] = fs; }
  // ---- copy phase
  const uint32_t* rec[4]; const uint32_t* frec[4];                      // of the four samples in flight
  copy_phase(lane, k0, batch, L.words / 2,
    [&](int u, int i, int p) {
      const int si = __builtin_amdgcn_readlane(s, i), ei = __builtin_amdgcn_readlane(e, i), fi = __builtin_amdgcn_readlane(fs, i);
      rec[u] = si >= 0 ? record(B, si, ei) : nullptr;
      frec[u] = fi >= 0 ? record(B, fi, ei) : nullptr;
      if (!rec[u]) return rec[u];
      // a virtual sample's desired goal (pairs 6-8) is the future record's next_achieved (pairs 3-5)
      return (frec[u] && p >= 6 && p < 9) ? frec[u] + 2 * (p - 3) : rec[u] + 2 * p;
    },
    [&](int u, int row, int p, uint2 v) {
      if (p < 9) {                       // a float64 goal
        const double g = __longlong_as_double((long long)(((unsigned long long)v.y << 32) | v.x));
        float* dst = p < 3 ? O.ach : (p < 6 ? O.nach : O.des);
        if (dst) dst[(size_t)row * 3 + p % 3] = (float)g;
      } else {
        emit_word(B, O, row, 2 * p, v.x, frec[u] != nullptr, rec[u], frec[u]);
        emit_word(B, O, row, 2 * p + 1, v.y, frec[u] != nullptr, rec[u], frec[u]);
      }
    });
}

int check_buf(const mcg_her_buf* b, const char* who) {
  if (!b) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_her_buf", who);
  if (!b->records || !b->t_run || !b->last_obs || !b->last_achieved || !b->counters) return mcg_fail(MCG_ERR_ARG, "%s: null pointer in mcg_her_buf", who);
  if (b->n_envs < 1 || b->obs_dim < 1 || b->act_dim < 1) return mcg_fail(MCG_ERR_ARG, "%s: n_envs, obs_dim and act_dim must be >= 1", who);
  if (b->max_episode_steps < 1) return mcg_fail(MCG_ERR_ARG, "%s: max_episode_steps must be >= 1", who);
  if ((long long)b->capacity < 2ll * b->max_episode_steps)
    return mcg_fail(MCG_ERR_ARG, "%s: capacity < 2 * max_episode_steps (an episode must not overlap itself in the ring)", who);
  if (((uintptr_t)b->records & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: records is not 16-byte aligned", who);
  return MCG_OK;
}

Her view(const mcg_her_buf* b) {
  Her B;
  B.rec = static_cast<uint32_t*>(b->records); B.t_run = b->t_run; B.last_obs = b->last_obs; B.last_ach = b->last_achieved;
  B.cnt = reinterpret_cast<unsigned long long*>(b->counters);
  B.n = b->n_envs; B.cap = b->capacity; B.max_steps = b->max_episode_steps; B.reward_type = b->reward_type; B.thr = b->distance_threshold;
  B.L = layout(b->obs_dim, b->act_dim);
  return B;
}

}  // namespace

extern "C" {

int64_t mcg_her_record_bytes(int obs_dim, int act_dim) {
  return record_bytes(obs_dim, act_dim, layout(obs_dim, act_dim).words);
}

int mcg_her_start(const mcg_her_buf* buf, const mcg_step_out* first, const uint8_t* mask, void* stream) {
  if (const int rc = check_buf(buf, "mcg_her_start")) return rc;
  if (!first) return mcg_fail(MCG_ERR_ARG, "mcg_her_start: null mcg_step_out");
  if (!first->obs || !first->achieved_goal) return mcg_fail(MCG_ERR_ARG, "mcg_her_start: obs and achieved_goal of the reset's output are required");
  const Her B = view(buf);
  const long long total = (long long)B.n * (B.L.D + 4);
  hipLaunchKernelGGL(her_start_kernel, dim3(blocks(total, ADD_LANES)), dim3(ADD_LANES), 0, (hipStream_t)stream,
                     B, first->obs, first->achieved_goal, mask);
  return launched("mcg_her");
}

int mcg_her_add(const mcg_her_buf* buf, int64_t n_written, const float* actions, const mcg_step_out* out, void* stream) {
  if (const int rc = check_buf(buf, "mcg_her_add")) return rc;
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "mcg_her_add: n_written < 0");
  if (!actions) return mcg_fail(MCG_ERR_ARG, "mcg_her_add: null actions");
  if (!out) return mcg_fail(MCG_ERR_ARG, "mcg_her_add: null mcg_step_out");
  if (!out->obs || !out->achieved_goal || !out->desired_goal || !out->reward || !out->terminated || !out->truncated || !out->final_obs ||
      !out->final_achieved || !out->final_desired)
    return mcg_fail(MCG_ERR_ARG, "mcg_her_add: obs, achieved_goal, desired_goal, reward, terminated, truncated and the three final_* of the step's output are required");
  const Her B = view(buf);
  const int elems = 9 + (B.L.words - GOAL_WORDS);
  int epb = ADD_LANES / elems;
  epb = epb < 1 ? 1 : (epb > ADD_MAX_EPB ? ADD_MAX_EPB : epb);
  hipLaunchKernelGGL(her_add_kernel, dim3(blocks(B.n, epb)), dim3(ADD_LANES), 0, (hipStream_t)stream,
                     B, (int)(n_written % B.cap), epb, actions, *out);
  return launched("mcg_her");
}

int mcg_her_sample(const mcg_her_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch, int n_virtual,
                   const mcg_her_batch* out, void* stream) {
  if (const int rc = check_buf(buf, "mcg_her_sample")) return rc;
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "mcg_her_sample: n_written < 0");
  if (batch < 1) return mcg_fail(MCG_ERR_ARG, "mcg_her_sample: batch must be >= 1");
  if (n_virtual < 0 || n_virtual > batch) return mcg_fail(MCG_ERR_ARG, "mcg_her_sample: n_virtual outside [0, batch]");
  if (!out) return mcg_fail(MCG_ERR_ARG, "mcg_her_sample: null mcg_her_batch");
  if (n_virtual > 0 && buf->reward_type != MCG_REWARD_SPARSE && buf->reward_type != MCG_REWARD_DENSE)
    return mcg_fail(MCG_ERR_UNSUPPORTED, "mcg_her_sample: relabelling needs a reward that depends on the goals alone (sparse or dense); reward_shaping depends on simulator state");
  const Her B = view(buf);
  const Batch O = {out->obs, out->achieved, out->desired, out->next_obs, out->next_achieved, out->action, out->reward, out->done, out->index};
  hipLaunchKernelGGL(her_sample_kernel, dim3(blocks(batch, SAMPLES_PER_BLOCK)), dim3(SAMPLE_LANES), 0,
                     (hipStream_t)stream, B, (long long)n_written, (unsigned long long)seed, (unsigned long long)call, batch, n_virtual, O);
  return launched("mcg_her");
}

}  // extern "C"
