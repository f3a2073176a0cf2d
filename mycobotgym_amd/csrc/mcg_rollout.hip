// mcg_rollout.hip -- the on-policy rollout buffers (include/mcg.h: mcg_rollout_* for state observations, mcg_rollout_img_* for pictures):
// insertion with the time-limit bootstrap, the advantage recursion (GAE) and the shuffled minibatch gather on the device.  The plane
// row, the recursion and the permutation exist once and serve both.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives: the step, render and replay kernels' code
// objects stay laid out as they are without this file.  Kernels and C entries are both here.  The C side is stateless: every call gets
// the caller's device pointers in an mcg_rollout_buf; of mcg_engine.hpp it uses the error reporting alone.
//
// A record is float32 throughout and is read and written as 4-byte words (the gather: as 8-byte pairs); Layout names the words.
#include <hip/hip_runtime.h>

#include <cmath>
#include <utility>

#include "mcg.h"
#include "mcg_buffer.hpp"        // what the replay buffer has too: launched, record_bytes, carry, copy_phase; philox4x32_10
#include "mcg_pixels.hpp"        // what the picture replay buffer has too: Pix, Src, load_chunk, each_unit, the output rows' stores

using namespace mcg;

namespace {

constexpr int FEISTEL_ROUNDS = 4;
constexpr int ADD_LANES = 256;
constexpr int GAE_LANES = 64;           // lane = environment and nothing is shared: one wave per block spreads 8192 environments over 128 CUs
constexpr int MAX_FRAME_STACK = 8;      // frames of a stack that the picture buffer's stacked entries rebuild (mcg_frame_stack_push's limit)

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
// The plane row of environment e at `at` = pos * N + e, and the one writer of last_start: one lane per environment (both buffers).
MCG_DEV void plane_row(const Roll& B, size_t at, int e, const float* __restrict__ values, const float* __restrict__ final_values,
                       const double* __restrict__ reward, const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated) {
#pragma clang fp contract(off)
  const bool term = terminated[e] != 0, trunc = truncated[e] != 0;
  float r = (float)reward[e];
  if (final_values && trunc && !term) {            // [RECALL] SB3 collect_rollouts: rewards[idx] += gamma * terminal_value
    const float boot = B.g32 * final_values[e];
    r = r + boot;
  }
  B.rew[at] = r;
  B.val[at] = values[e];
  B.start[at] = B.last_start[e];
  B.last_start[e] = (term || trunc) ? 1 : 0;
}

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
  if (w == L.words) {
    plane_row(B, at, e, values, final_values, O.reward, O.terminated, O.truncated);
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
// The index phase of both gathers, one lane per sample: position `k` of the epoch (on the lanes with `mine`; the others ride along)
// walks through the Feistel network until it lands below M -> the transition's flat index i = env * T + step.
MCG_DEV uint32_t walk(bool mine, uint32_t k, uint32_t M, int h, unsigned long long seed, unsigned long long epoch) {
  const uint32_t half = (1u << h) - 1u;
  const uint32_t c1 = (uint32_t)epoch, c3 = DOMAIN_ROLLOUT ^ ((uint32_t)(epoch >> 32) << 8);
  uint32_t x = mine ? k : 0u;
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
  return x;
}

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
  const int j = j0 + lane;
  const bool mine = lane < SPW && j < count;
  const uint32_t x = walk(mine, (uint32_t)first + (uint32_t)j, M, h, seed, epoch);
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


// ================================================================================================ the picture buffer
// mcg_rollout_img_*: the planes, the recursion and the permutation are the ones above (plane_row, rollout_gae_kernel, walk); what is
// new is data movement, and every kernel here is judged by bytes per second.  A picture is X.P bytes (a multiple of 16) in `pixels`,
// so every access to `pixels` is one aligned 16-byte word per lane, 1 KiB contiguous per wave instruction (mcg_pixels.hpp).
// Lane = 16 bytes of row `row` of pixels, environments neighbours: the grid writes one contiguous run.  One more lane per
// environment, after the pixels, sets last_start.
template <int W>
__global__ __launch_bounds__(ADD_LANES) void img_start_kernel(Roll B, Pix X, int row, Src S, const uint8_t* __restrict__ mask) {
  const int c16 = X.P >> 4;
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, npix = (long long)B.n * c16;
  if (x >= npix + B.n) return;
  const int e = x < npix ? (int)(x / c16) : (int)(x - npix);
  if (mask && mask[e] == 0) return;
  if (x < npix) {
    const int q = (int)(x % c16);
    reinterpret_cast<uint4*>(X.px + ((size_t)row * B.n + e) * X.P)[q] = load_chunk<W>(X, S, e, q * 16);
  } else {
    B.last_start[e] = 1;
  }
}

// The same run into row pos + 1; after the pixels, per environment, one lane per 16 bytes of its record and one for its plane row.
template <int W>
__global__ __launch_bounds__(ADD_LANES) void img_add_kernel(Roll B, Pix X, int pos, Src S, const float* __restrict__ actions,
                                                            const float* __restrict__ values, const float* __restrict__ log_probs,
                                                            const float* __restrict__ final_values, const double* __restrict__ reward,
                                                            const uint8_t* __restrict__ terminated, const uint8_t* __restrict__ truncated) {
  const int c16 = X.P >> 4, r16 = X.rw >> 2;
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, npix = (long long)B.n * c16;
  if (x < npix) {
    const int e = (int)(x / c16), q = (int)(x % c16);
    reinterpret_cast<uint4*>(X.px + ((size_t)(pos + 1) * B.n + e) * X.P)[q] = load_chunk<W>(X, S, e, q * 16);
    return;
  }
  const long long y = x - npix;
  if (y >= (long long)B.n * (r16 + 1)) return;
  const int e = (int)(y / (r16 + 1)), q = (int)(y % (r16 + 1));
  const size_t at = (size_t)pos * B.n + e;
  if (q == r16) {
    plane_row(B, at, e, values, final_values, reward, terminated, truncated);
    return;
  }
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {          // action[A], log_prob, zeros
    const int i = 4 * q + k;
    w[k] = i < X.A ? __float_as_uint(actions[(size_t)e * X.A + i]) : i == X.A ? __float_as_uint(log_probs[e]) : 0u;
  }
  reinterpret_cast<uint4*>(B.rec)[at * r16 + q] = make_uint4(w[0], w[1], w[2], w[3]);
}

// Row `row` (> 0) of pixels to row 0: lane = 16 bytes.
__global__ __launch_bounds__(ADD_LANES) void img_carry_kernel(Roll B, Pix X, int row) {
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, n16 = (long long)B.n * (X.P >> 4);
  if (x >= n16) return;
  uint4* to = reinterpret_cast<uint4*>(X.px);
  to[x] = to[(size_t)row * n16 + x];
}

// The carry of a buffer that hands out stacks of k frames: pixel rows pos - (k - 1) .. pos go to rows -(k - 1) .. 0 and episode_start
// rows pos - (k - 1) .. pos - 1 to rows -(k - 1) .. -1 (rows before row 0: the caller's history rows).  Source and destination overlap
// where pos < k, so this is frame_stack_push_kernel's in-place shift: a lane owns one 16-byte position of one environment in all k
// rows, loads them all and only then stores; no other lane touches that position in any row.  After the pixels one lane per
// environment does the same with its k - 1 flag bytes.  Row offsets are signed and 64-bit.  The rows a lane holds are a pack expansion
// over I = 0 .. K - 1 of the compiler's own 16-byte vector type: held as HIP's uint4 (a class), more than five rows went to scratch.
template <class V, int... I>
MCG_DEV void shift_rows(V* at, int pos, long long stride, std::integer_sequence<int, I...>) {
  const V v[] = {at[(long long)(pos - I) * stride]...};          // row pos - I, every load before the first store
  ((at[-(long long)I * stride] = v[I]), ...);                    // to row -I
}

template <int K>
__global__ __launch_bounds__(ADD_LANES) void img_carry_stacked_kernel(Roll B, Pix X, int pos) {
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, n16 = (long long)B.n * (X.P >> 4);
  if (x < n16) {
    typedef unsigned int word16 __attribute__((ext_vector_type(4)));
    shift_rows(reinterpret_cast<word16*>(X.px) + x, pos, n16, std::make_integer_sequence<int, K>{});
    return;
  }
  const long long e = x - n16;
  if (e >= B.n) return;
  if constexpr (K > 1)                   // flag rows pos - 1 .. pos - (K - 1) to rows -1 .. -(K - 1): the same shift, one row further back
    shift_rows(B.start + e - B.n, pos, (long long)B.n, std::make_integer_sequence<int, K - 1>{});
}

struct ImgBatch { uint8_t* pix; float *pix_f32, *act, *val, *logp, *adv, *ret; int32_t* index; };

// One sample per wave, four per block: a minibatch of 4096 is 4096 waves, four on every SIMD of the chip, each with its sample's
// 4 KB or more in flight (measured against 2 and 4 samples per wave, which share a walk but leave the chip a half or a quarter as many
// waves to hide the loads behind: DESIGN.md section 13).  The index phase is rollout_gather_kernel's with every lane of the wave on
// the wave's one sample, so the picture's row needs no broadcast.
// ALIGN: what divides Pu and the output pointers (the host's choice): 16 -- the u8 rows are stored as 16-byte words, 4 -- as 4-byte
// words, 1 -- as bytes; the normalised picture is one float4 per lane from 4 source bytes (ALIGN >= 4: a wave's store instruction
// covers 1 KiB contiguous) or one float per lane.
template <int ALIGN>
__global__ __launch_bounds__(SAMPLE_LANES) void img_gather_kernel(Roll B, Pix X, unsigned long long seed, unsigned long long epoch,
                                                                  int first, int count, int h, ImgBatch O) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (SAMPLE_LANES / 64) + (threadIdx.x >> 6);   // wave-uniform; the output row of this wave
  if (j >= count) return;
  // ---- index phase
  const uint32_t M = (uint32_t)B.n * (uint32_t)B.T;                     // < 2^31 (host check)
  const uint32_t x = walk(true, (uint32_t)first + (uint32_t)j, M, h, seed, epoch);
  const size_t src = (size_t)(x % (uint32_t)B.T) * B.n + x / (uint32_t)B.T;          // row in the [T, N] planes; < M
  if (lane == 0) {                       // the sample's plane words
    const float v = B.val[src], a = B.adv[src], g = B.ret[src];
    if (O.val) O.val[j] = v;
    if (O.adv) O.adv[j] = a;
    if (O.ret) O.ret[j] = g;
    if (O.index) O.index[j] = (int32_t)x;
  }
  const uint32_t* rec = B.rec + src * X.rw;          // and its record: action[A], log_prob
  if (O.act)
    for (int w = lane; w < X.A; w += 64) O.act[(size_t)j * X.A + w] = __uint_as_float(rec[w]);
  if (O.logp && lane == 0) O.logp[j] = __uint_as_float(rec[X.A]);
  // ---- copy phase
  const uint8_t* from = X.px + src * X.P;
  if (O.pix) {
    uint8_t* row = O.pix + (size_t)j * X.Pu;
    each_unit<uint4>(lane, X.P >> 4,
      [&](int q) { return reinterpret_cast<const uint4*>(from)[q]; },
      [&](int q, uint4 v) { store_u8<ALIGN>(row, X.Pu, q, v); });
  }
  if (O.pix_f32) {                       // byte / 255: the correctly rounded float32 quotient (IEEE division, nothing reciprocal)
    float* row = O.pix_f32 + (size_t)j * X.Pu;
    if constexpr (ALIGN >= 4) {
      each_unit<uint32_t>(lane, X.Pu >> 2,
        [&](int q) { return reinterpret_cast<const uint32_t*>(from)[q]; },
        [&](int q, uint32_t v) { reinterpret_cast<float4*>(row)[q] = quotient_255(v); });
    } else {
      each_unit<uint8_t>(lane, X.Pu, [&](int q) { return from[q]; }, [&](int q, uint8_t v) { row[q] = (float)v / 255.0f; });
    }
  }
}

// img_gather_kernel on stacks of k frames rebuilt from the single stored frames: one sample per wave, four per block, the walk, the
// plane words and the record exactly as there.  Index phase: the flags of rows t, t - 1, .. t - (k - 2) of the sample's environment
// are loaded together -- their addresses depend on the draw alone (a row before row 0 is one of the caller's history rows), so the
// phase waits for memory once more, not k - 1 times -- and then tested up to the first episode start: `depth` frames of the stack
// belong to the sample's episode.  Copy phase: the source picture is the outer loop, slot s = 0 .. k - 1 takes row t - (k - 1 - s) in
// one full-width pass of each_unit (no unit has to find its picture); a slot before the episode's start is stored as zeros and its
// source is not loaded.  Every byte of the output row (k * Pu long) is written.  Slot s starts at byte s * Pu of the row, so ALIGN,
// which divides Pu and the output pointers (store_align), divides every slot's address too.
template <int ALIGN>
__global__ __launch_bounds__(SAMPLE_LANES) void img_gather_stacked_kernel(Roll B, Pix X, unsigned long long seed, unsigned long long epoch,
                                                                          int first, int count, int h, int k, ImgBatch O) {
  const int lane = threadIdx.x & 63;
  const int j = blockIdx.x * (SAMPLE_LANES / 64) + (threadIdx.x >> 6);   // wave-uniform; the output row of this wave
  if (j >= count) return;
  // ---- index phase
  const uint32_t M = (uint32_t)B.n * (uint32_t)B.T;                     // < 2^31 (host check)
  const uint32_t x = walk(true, (uint32_t)first + (uint32_t)j, M, h, seed, epoch);
  const long long t = x % (uint32_t)B.T, e = x / (uint32_t)B.T, n = B.n;
  const size_t src = (size_t)(t * n + e);            // row in the [T, N] planes; < M
  uint8_t flag[MAX_FRAME_STACK - 1];
#pragma unroll
  for (int i = 0; i < MAX_FRAME_STACK - 1; i++)
    flag[i] = i < k - 1 ? B.start[(t - i) * n + e] : (uint8_t)1;
  if (lane == 0) {                       // the sample's plane words
    const float v = B.val[src], a = B.adv[src], g = B.ret[src];
    if (O.val) O.val[j] = v;
    if (O.adv) O.adv[j] = a;
    if (O.ret) O.ret[j] = g;
    if (O.index) O.index[j] = (int32_t)x;
  }
  const uint32_t* rec = B.rec + src * X.rw;          // and its record: action[A], log_prob
  if (O.act)
    for (int w = lane; w < X.A; w += 64) O.act[(size_t)j * X.A + w] = __uint_as_float(rec[w]);
  if (O.logp && lane == 0) O.logp[j] = __uint_as_float(rec[X.A]);
  int depth = 1;
#pragma unroll
  for (int i = 0; i < MAX_FRAME_STACK - 1; i++)     // row t - i is no episode start: row t - i - 1 belongs to the same episode
    if (depth == i + 1 && flag[i] == 0) depth = i + 2;
  depth = __builtin_amdgcn_readfirstlane(depth);    // (every lane holds the same value: the copy loop's branch is a scalar one)
  // ---- copy phase
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
  for (int s = 0; s < k; s++) {
    const int back = k - 1 - s;
    const bool live = back < depth;
    const uint8_t* from = X.px + ((t - back) * n + e) * X.P;
    const size_t slot = ((size_t)j * k + s) * X.Pu;
    if (O.pix) {
      uint8_t* row = O.pix + slot;
      if (live)
        each_unit<uint4>(lane, X.P >> 4,
          [&](int q) { return reinterpret_cast<const uint4*>(from)[q]; },
          [&](int q, uint4 v) { store_u8<ALIGN>(row, X.Pu, q, v); });
      else
        for (int q = lane; q < (X.P >> 4); q += 64) store_u8<ALIGN>(row, X.Pu, q, zero);
    }
    if (O.pix_f32) {                     // byte / 255: the correctly rounded float32 quotient (IEEE division, nothing reciprocal)
      float* row = O.pix_f32 + slot;
      if constexpr (ALIGN >= 4) {
        if (live)
          each_unit<uint32_t>(lane, X.Pu >> 2,
            [&](int q) { return reinterpret_cast<const uint32_t*>(from)[q]; },
            [&](int q, uint32_t v) { reinterpret_cast<float4*>(row)[q] = quotient_255(v); });
        else
          for (int q = lane; q < (X.Pu >> 2); q += 64) reinterpret_cast<float4*>(row)[q] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
      } else {
        if (live)
          each_unit<uint8_t>(lane, X.Pu, [&](int q) { return from[q]; }, [&](int q, uint8_t v) { row[q] = (float)v / 255.0f; });
        else
          for (int q = lane; q < X.Pu; q += 64) row[q] = 0.0f;
      }
    }
  }
}

// ------------------------------------------------------------------------------------------- host side, pictures
int check_img(const mcg_rollout_img_buf* b, const char* who) {
  if (!b) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_rollout_img_buf", who);
  if (!b->pixels || !b->records || !b->reward || !b->value || !b->episode_start || !b->advantage || !b->returns || !b->last_start)
    return mcg_fail(MCG_ERR_ARG, "%s: null pointer in mcg_rollout_img_buf", who);
  if (b->n_envs < 1 || b->channels < 1 || b->size < 1 || b->act_dim < 1 || b->n_steps < 1)
    return mcg_fail(MCG_ERR_ARG, "%s: n_envs, channels, size, act_dim and n_steps must be >= 1", who);
  if (b->channels > 8) return mcg_fail(MCG_ERR_ARG, "%s: channels must be <= 8", who);
  if (b->size > 512) return mcg_fail(MCG_ERR_ARG, "%s: size must be <= 512", who);
  if ((long long)b->n_steps * b->n_envs >= (1ll << 31)) return mcg_fail(MCG_ERR_ARG, "%s: n_steps * n_envs must be below 2^31", who);
  if (((uintptr_t)b->pixels & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: pixels is not 16-byte aligned", who);
  if (((uintptr_t)b->records & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: records is not 16-byte aligned", who);
  if (!std::isfinite(b->gamma) || !std::isfinite(b->gae_lambda) || b->gamma < 0.0 || b->gamma > 1.0 || b->gae_lambda < 0.0 ||
      b->gae_lambda > 1.0)
    return mcg_fail(MCG_ERR_ARG, "%s: gamma and gae_lambda must be finite and in [0, 1]", who);
  return MCG_OK;
}

Roll planes(const mcg_rollout_img_buf* b) {
  Roll B = {};
  B.rec = static_cast<uint32_t*>(b->records); B.rew = b->reward; B.val = b->value; B.adv = b->advantage; B.ret = b->returns;
  B.start = b->episode_start; B.last_start = b->last_start;
  B.n = b->n_envs; B.T = b->n_steps;
  B.g32 = (float)b->gamma; B.c32 = (float)(b->gamma * b->gae_lambda);
  return B;
}

Pix pixels(const mcg_rollout_img_buf* b) {
  Pix X;
  X.px = b->pixels; X.SS = b->size * b->size; X.Pu = b->channels * X.SS; X.P = (X.Pu + 15) / 16 * 16;      // Pu <= 8 * 512 * 512
  X.A = b->act_dim; X.rw = padded_words(b->act_dim + 1);
  return X;
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

int64_t mcg_rollout_img_record_bytes(int act_dim) { return act_dim < 1 ? 0 : (int64_t)padded_words(act_dim + 1) * 4; }

int mcg_rollout_img_start(const mcg_rollout_img_buf* buf, int pos, const uint8_t* img, int64_t env_stride, int64_t chan_stride,
                          const uint8_t* mask, void* stream) {
  if (const int rc = check_img(buf, "mcg_rollout_img_start")) return rc;
  if (pos < 0 || pos > buf->n_steps) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_start: pos outside [0, n_steps]");
  if (const int rc = check_src(buf->channels, buf->size, img, env_stride, chan_stride, "mcg_rollout_img_start", "img")) return rc;
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  const Src S = {img, (long long)env_stride, (long long)chan_stride};
  const dim3 grid(blocks((long long)B.n * (X.P / 16) + B.n, ADD_LANES)), block(ADD_LANES);
  switch (load_width(buf->channels, buf->size, img, env_stride, chan_stride)) {
    case 16: hipLaunchKernelGGL(img_start_kernel<16>, grid, block, 0, (hipStream_t)stream, B, X, pos, S, mask); break;
    case 4: hipLaunchKernelGGL(img_start_kernel<4>, grid, block, 0, (hipStream_t)stream, B, X, pos, S, mask); break;
    default: hipLaunchKernelGGL(img_start_kernel<1>, grid, block, 0, (hipStream_t)stream, B, X, pos, S, mask);
  }
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_add(const mcg_rollout_img_buf* buf, int pos, const float* actions, const float* values, const float* log_probs,
                        const float* final_values, const uint8_t* img, int64_t env_stride, int64_t chan_stride, const double* reward,
                        const uint8_t* terminated, const uint8_t* truncated, void* stream) {
  if (const int rc = check_img(buf, "mcg_rollout_img_add")) return rc;
  if (pos < 0 || pos >= buf->n_steps) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_add: pos outside [0, n_steps)");
  if (!actions) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_add: null actions");
  if (!values) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_add: null values");
  if (!log_probs) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_add: null log_probs");
  if (!reward || !terminated || !truncated)
    return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_add: reward, terminated and truncated of the step's output are required");
  if (const int rc = check_src(buf->channels, buf->size, img, env_stride, chan_stride, "mcg_rollout_img_add", "img")) return rc;
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  const Src S = {img, (long long)env_stride, (long long)chan_stride};
  const dim3 grid(blocks((long long)B.n * (X.P / 16) + (long long)B.n * (X.rw / 4 + 1), ADD_LANES)), block(ADD_LANES);
#define MCG_IMG_ADD(W) hipLaunchKernelGGL(img_add_kernel<W>, grid, block, 0, (hipStream_t)stream, B, X, pos, S, actions, values, \
                                          log_probs, final_values, reward, terminated, truncated)
  switch (load_width(buf->channels, buf->size, img, env_stride, chan_stride)) {
    case 16: MCG_IMG_ADD(16); break;
    case 4: MCG_IMG_ADD(4); break;
    default: MCG_IMG_ADD(1);
  }
#undef MCG_IMG_ADD
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_gae(const mcg_rollout_img_buf* buf, const float* last_values, void* stream) {
  if (const int rc = check_img(buf, "mcg_rollout_img_gae")) return rc;
  if (!last_values) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gae: null last_values");
  const Roll B = planes(buf);
  hipLaunchKernelGGL(rollout_gae_kernel, dim3(blocks(B.n, GAE_LANES)), dim3(GAE_LANES), 0, (hipStream_t)stream, B, last_values);
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_carry(const mcg_rollout_img_buf* buf, int pos, void* stream) {
  if (const int rc = check_img(buf, "mcg_rollout_img_carry")) return rc;
  if (pos < 0 || pos > buf->n_steps) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_carry: pos outside [0, n_steps]");
  if (pos == 0) return MCG_OK;           // the picture to continue from is in row 0 already
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  hipLaunchKernelGGL(img_carry_kernel, dim3(blocks((long long)B.n * (X.P / 16), ADD_LANES)), dim3(ADD_LANES), 0, (hipStream_t)stream, B, X,
                     pos);
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_gather(const mcg_rollout_img_buf* buf, uint64_t seed, uint64_t epoch, int64_t first, int64_t count,
                           const mcg_rollout_img_batch* out, void* stream) {
  if (const int rc = check_img(buf, "mcg_rollout_img_gather")) return rc;
  const int64_t M = (int64_t)buf->n_steps * buf->n_envs;
  if (first < 0) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gather: first < 0");
  if (count < 1) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gather: count must be >= 1");
  if (first > M || count > M - first) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gather: first + count > n_steps * n_envs");
  if (!out) return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gather: null mcg_rollout_img_batch");
  if (!out->pix && !out->pix_f32 && !out->action && !out->old_value && !out->old_log_prob && !out->advantage && !out->returns &&
      !out->index)
    return mcg_fail(MCG_ERR_ARG, "mcg_rollout_img_gather: all outputs are null");
  int b = 2;
  while ((1ll << b) < M) b += 2;         // as mcg_rollout_gather
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  const ImgBatch O = {out->pix, out->pix_f32, out->action, out->old_value, out->old_log_prob, out->advantage, out->returns, out->index};
  const int align = store_align(X.Pu, (uint64_t)(uintptr_t)out->pix, (uint64_t)(uintptr_t)out->pix_f32);
  const dim3 grid(blocks(count, SAMPLE_LANES / 64)), block(SAMPLE_LANES);
#define MCG_IMG_GATHER(AL) hipLaunchKernelGGL(img_gather_kernel<AL>, grid, block, 0, (hipStream_t)stream, B, X, (unsigned long long)seed, \
                                              (unsigned long long)epoch, (int)first, (int)count, b / 2, O)
  switch (align) {
    case 16: MCG_IMG_GATHER(16); break;
    case 4: MCG_IMG_GATHER(4); break;
    default: MCG_IMG_GATHER(1);
  }
#undef MCG_IMG_GATHER
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_carry_stacked(const mcg_rollout_img_buf* buf, int pos, int frame_stack, void* stream) {
  const char* who = "mcg_rollout_img_carry_stacked";
  if (const int rc = check_img(buf, who)) return rc;
  if (frame_stack < 1 || frame_stack > MAX_FRAME_STACK) return mcg_fail(MCG_ERR_ARG, "%s: frame_stack must be in [1, 8]", who);
  if (pos < 0 || pos > buf->n_steps) return mcg_fail(MCG_ERR_ARG, "%s: pos outside [0, n_steps]", who);
  if (pos == 0) return MCG_OK;           // every row is where it belongs already
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  const dim3 grid(blocks((long long)B.n * (X.P / 16) + B.n, ADD_LANES)), block(ADD_LANES);
#define MCG_IMG_CARRY(K) case K: hipLaunchKernelGGL(img_carry_stacked_kernel<K>, grid, block, 0, (hipStream_t)stream, B, X, pos); break
  switch (frame_stack) {
    MCG_IMG_CARRY(1); MCG_IMG_CARRY(2); MCG_IMG_CARRY(3); MCG_IMG_CARRY(4); MCG_IMG_CARRY(5); MCG_IMG_CARRY(6); MCG_IMG_CARRY(7);
    MCG_IMG_CARRY(8);
  }
#undef MCG_IMG_CARRY
  return launched("mcg_rollout_img");
}

int mcg_rollout_img_gather_stacked(const mcg_rollout_img_buf* buf, int frame_stack, uint64_t seed, uint64_t epoch, int64_t first,
                                   int64_t count, const mcg_rollout_img_batch* out, void* stream) {
  const char* who = "mcg_rollout_img_gather_stacked";
  if (const int rc = check_img(buf, who)) return rc;
  if (frame_stack < 1 || frame_stack > MAX_FRAME_STACK) return mcg_fail(MCG_ERR_ARG, "%s: frame_stack must be in [1, 8]", who);
  const int64_t M = (int64_t)buf->n_steps * buf->n_envs;
  if (first < 0) return mcg_fail(MCG_ERR_ARG, "%s: first < 0", who);
  if (count < 1) return mcg_fail(MCG_ERR_ARG, "%s: count must be >= 1", who);
  if (first > M || count > M - first) return mcg_fail(MCG_ERR_ARG, "%s: first + count > n_steps * n_envs", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_rollout_img_batch", who);
  if (!out->pix && !out->pix_f32 && !out->action && !out->old_value && !out->old_log_prob && !out->advantage && !out->returns &&
      !out->index)
    return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  int b = 2;
  while ((1ll << b) < M) b += 2;         // as mcg_rollout_gather
  const Roll B = planes(buf);
  const Pix X = pixels(buf);
  const ImgBatch O = {out->pix, out->pix_f32, out->action, out->old_value, out->old_log_prob, out->advantage, out->returns, out->index};
  const int align = store_align(X.Pu, (uint64_t)(uintptr_t)out->pix, (uint64_t)(uintptr_t)out->pix_f32);
  const dim3 grid(blocks(count, SAMPLE_LANES / 64)), block(SAMPLE_LANES);
#define MCG_IMG_GATHER(AL) hipLaunchKernelGGL(img_gather_stacked_kernel<AL>, grid, block, 0, (hipStream_t)stream, B, X, \
                                              (unsigned long long)seed, (unsigned long long)epoch, (int)first, (int)count, b / 2, frame_stack, O)
  switch (align) {
    case 16: MCG_IMG_GATHER(16); break;
    case 4: MCG_IMG_GATHER(4); break;
    default: MCG_IMG_GATHER(1);
  }
#undef MCG_IMG_GATHER
  return launched("mcg_rollout_img");
}

}  // extern "C"
