// mcg_policy.hpp -- what mcg_policy.hip (the forward of collection) and mcg_policy_grad.hip (evaluate_actions, the loss gradient, Adam)
// share: the blob's plan, the kernel's view of a policy, the matrix instruction and the layer helpers of the forward pass.  The blob's
// layout and the operand map of v_mfma_f32_16x16x4_f32 are stated in mcg_policy.hip's head; each file's own rule stays in that file.
// And what every policy's code object shares, mcg_cnn.hip's and (through mcg_sac.hpp) the off-policy learners' too: the matrix
// instruction, the Gaussian draw gauss4, and the diagonal Gaussian head -- sampling, the log-prob of stored actions with its
// derivative, the entropy -- for ActorCritic and CnnActorCritic.
#pragma once

#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>

#include "mcg.h"
#include "mcg_buffer.hpp"        // blocks, launched; mcg_fail; philox_pair

namespace {

constexpr int MAX_LAYERS = 3, MAX_WIDTH = 256, MAX_ACT = 16, MAX_OBS = 4096;
constexpr int WAVE = 64, TILE = 16;

typedef float f4 __attribute__((ext_vector_type(4)));

struct Net {                             // one trunk and its head: layer n is the head
  int n, nt[MAX_LAYERS];                 // hidden layers and their widths in tiles of 16 units
  int w[MAX_LAYERS + 1], b[MAX_LAYERS + 1];      // offsets of a layer's tiles and of its bias in the blob, in floats
};
struct Pol {                             // mcg_policy as the kernel sees it; net[0]: the value net, net[1]: the policy net
  const float* blob; Net net[2]; int log_std, N, D, A, kb0, act;
};

MCG_DEV f4 mfma(float a, float b, f4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

MCG_DEV float activate(int act, float x) { return act == MCG_POLICY_TANH ? tanhf(x) : fmaxf(x, 0.0f); }

// x[L], L = 0..3, by selects (the layer loop is a loop: its index is no constant)
MCG_DEV int sel4(const int (&x)[MAX_LAYERS + 1], int L) { return L == 0 ? x[0] : L == 1 ? x[1] : L == 2 ? x[2] : x[3]; }

// The first layer: the k-blocks are a loop (any D), the sample's columns are read where they lie and rounded to float32 (In: double,
// the engine's observation; float, a minibatch of the rollout buffer).
template <int MT, class In>
MCG_DEV void first_layer(const Pol& P, const Net& net, const In* __restrict__ obs, const In* __restrict__ ach,
                         const In* __restrict__ des, int env, int g, int lane, f4 (&out)[MT]) {
  const float* __restrict__ W = P.blob + net.w[0];
  const float* __restrict__ bias = P.blob + net.b[0];
  const int nt = net.nt[0], D = P.D;
#pragma unroll
  for (int t = 0; t < MT; t++) {
    out[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (t < nt) out[t] = *reinterpret_cast<const f4*>(bias + 16 * t + 4 * g);
  }
  for (int kb = 0; kb < P.kb0; kb++) {
    const int f = 4 * kb + g;
    float x = 0.0f;
    if (f < 3) x = (float)ach[(size_t)env * 3 + f];
    else if (f < 6) x = (float)des[(size_t)env * 3 + (f - 3)];
    else if (f < D + 6) x = (float)obs[(size_t)env * D + (f - 6)];
#pragma unroll
    for (int t = 0; t < MT; t++)
      if (t < nt) out[t] = mfma(W[(t * P.kb0 + kb) * WAVE + lane], x, out[t]);
  }
}

// A later layer or a head: `in`'s registers are the B operands (mcg_policy.hip's head); layer `L` of `net`, nti input and nto output tiles.
template <int MTI, int MTO>
MCG_DEV void dense(const Pol& P, const Net& net, int L, int nti, int nto, const f4 (&in)[MTI], f4 (&out)[MTO], int g, int lane) {
  const float* __restrict__ W = P.blob + sel4(net.w, L);
  const float* __restrict__ bias = P.blob + sel4(net.b, L);
  const int nkb = 4 * nti;
#pragma unroll
  for (int T = 0; T < MTO; T++) {
    out[T] = f4{0.0f, 0.0f, 0.0f, 0.0f};
    if (T < nto) {
      f4 c = *reinterpret_cast<const f4*>(bias + 16 * T + 4 * g);
#pragma unroll
      for (int t = 0; t < MTI; t++) {
        if (t < nti) {
#pragma unroll
          for (int r = 0; r < 4; r++) c = mfma(W[(T * nkb + 4 * t + r) * WAVE + lane], in[t][r], c);
        }
      }
      out[T] = c;
    }
  }
}

// net[k] by selects: an index that is no constant would send the kernel's arguments through scratch
MCG_DEV Net pick(const Net& x, const Net& y, int k) {
  Net z;
  z.n = k ? y.n : x.n;
#pragma unroll
  for (int L = 0; L < MAX_LAYERS; L++) z.nt[L] = k ? y.nt[L] : x.nt[L];
#pragma unroll
  for (int L = 0; L <= MAX_LAYERS; L++) { z.w[L] = k ? y.w[L] : x.w[L]; z.b[L] = k ? y.b[L] : x.b[L]; }
  return z;
}

// ---------------------------------------------------------------------------------------------- the diagonal Gaussian
// Lane 16 g + i holds rows 4 g + r of a head, r = 0..3: components 4 g .. 4 g + 3 of sample i, pairs 2 g and 2 g + 1; the four lanes of
// a sample are summed by __shfl_xor 16, then 32: an order that does not depend on the tile.
constexpr double LOG_SQRT_2PI_D = 0.918938533204672742;                 // ln(2 pi) / 2
constexpr float ENTROPY_0 = 1.418938533204672742f;                      // 1/2 + ln(2 pi) / 2

struct EvalOut { float *value, *log_prob, *entropy; };                  // mcg_policy_eval_out

// n, zeros -> components 4 g .. 4 g + 3 of a row's standard Gaussian draw, those from A on left as they are: one Philox block per pair of
// components, Box-Muller in double, the second value of a last odd pair dropped.  The counter (mcg_policy.hip's head): `id` the global
// environment id or the row, `call` the caller's count, `stream` the domain byte (enum Domain, mcg_philox.hpp).
MCG_DEV void gauss4(f4& n, int A, int g, unsigned long long seed, unsigned long long id, unsigned long long call, uint32_t stream) {
#pragma unroll
  for (int q = 0; q < 2; q++) {
    if (4 * g + 2 * q < A) {
      double u0, u1, s, c;
      const uint32_t pair = (uint32_t)(2 * g + q);
      mcg::philox_pair((uint32_t)id, (uint32_t)call, pair ^ ((uint32_t)(call >> 32) << 8), stream ^ ((uint32_t)(id >> 32) << 8), seed, u0, u1);
      const double rad = sqrt(-2.0 * log(1.0 - u0));
      sincos(6.283185307179586476925 * u1, &s, &c);
      n[2 * q] = (float)(rad * c);
      if (4 * g + 2 * q + 1 < A) n[2 * q + 1] = (float)(rad * s);
    }
  }
}

// What sampling gives a lane: its components (zeros from A on; the mean is the head's rows) and the sample's log-prob (on all four lanes).
struct Sampled { f4 action, mean, noise; float log_prob; };

// The head's rows h and log_std's ls of a lane -> the sample.  The action is mean + exp(log_std) eps in double, rounded once (not clipped:
// the step kernels clip what they read); the log-prob is float32 throughout.  deterministic: the mean, no block, the log-prob of eps = 0.
MCG_DEV Sampled gauss_sample(int A, const f4& h, const f4& ls, int g, unsigned long long seed, unsigned long long id, unsigned long long call,
                             uint32_t stream, bool deterministic) {
  Sampled d;
  d.noise = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (!deterministic) gauss4(d.noise, A, g, seed, id, call, stream);
  float lp = 0.0f;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    d.action[r] = d.mean[r] = 0.0f;
    if (4 * g + r < A) {
      const float eps = d.noise[r];
      d.action[r] = deterministic ? h[r] : (float)((double)h[r] + exp((double)ls[r]) * (double)eps);
      d.mean[r] = h[r];
      lp += (-0.5f * eps) * eps - ls[r] - 0.918938533204672742f;               // - eps^2 / 2 - log_std - ln(2 pi) / 2
    }
  }
  lp += __shfl_xor(lp, 16);
  lp += __shfl_xor(lp, 32);
  d.log_prob = lp;
  return d;
}

// SB3's evaluate_actions: the log-prob of the stored `actions` of `row` -> on all four lanes, in double from the float32 mean (log_prob -
// old_log_prob and (ratio - 1) - ln ratio cancel most of its digits, and a sum of A terms of magnitude 1 in float32 would leave them its
// rounding: a few 1e-7 on a ratio near 1); the caller rounds it once.  dmu, dls: d log_prob / d mean_c = (a - mean) / sigma^2 and
// d log_prob / d log_std_c of the lane's components, zeros from A on (the gradient's; an evaluation drops them).
MCG_DEV double gauss_log_prob(int A, const f4& h, const f4& ls, const float* __restrict__ actions, size_t row, int g, f4& dmu, f4& dls) {
  double lpd = 0.0;
  dmu = dls = f4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < A) {
      const double inv = exp(-(double)ls[r]), zd = ((double)actions[row * A + c] - (double)h[r]) * inv;
      lpd += -0.5 * zd * zd - (double)ls[r] - LOG_SQRT_2PI_D;
      const float z = (float)zd;
      dmu[r] = z * (float)inv;
      dls[r] = z * z - 1.0f;
    }
  }
  lpd += __shfl_xor(lpd, 16);
  lpd += __shfl_xor(lpd, 32);
  return lpd;
}

// The entropy of the Gaussian: it depends on log_std alone.  Float32, in the components' order.
MCG_DEV float gauss_entropy(int A, const float* log_std) {
  float ent = 0.0f;
  for (int c = 0; c < A; c++) ent += ENTROPY_0 + log_std[c];
  return ent;
}

// ------------------------------------------------------------------------------------------------------- host side
// The dimensions and widths every plan accepts (this one, and mcg_sac.hpp's for the off-policy learners) -> true; false and `why`, a
// message that names the field.  `x`: the second net's prefix ("vf", "qf"); x_first: its widths are looked at before pi's.
inline bool checked_shape(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_x, const int32_t* x_width, const char* x,
                          bool x_first, const char** why) {
  static thread_local char msg[80];
  *why = msg;
  if (obs_dim < 1 || act_dim < 1) { *why = "obs_dim and act_dim must be >= 1"; return false; }
  if (obs_dim > MAX_OBS) { *why = "obs_dim must be <= 4096"; return false; }
  if (act_dim > MAX_ACT) { *why = "act_dim must be <= 16"; return false; }
  if (n_pi < 1 || n_pi > MAX_LAYERS) { *why = "n_pi must be in [1, 3]"; return false; }
  if (n_x < 1 || n_x > MAX_LAYERS) { snprintf(msg, sizeof msg, "n_%s must be in [1, 3]", x); return false; }
  if (!pi_width || !x_width) { snprintf(msg, sizeof msg, "null pi_width or %s_width", x); return false; }
  for (int k = 0; k < 2; k++) {
    const bool second = (k == 0) == x_first;
    const int n = second ? n_x : n_pi;
    const int32_t* w = second ? x_width : pi_width;
    for (int L = 0; L < n; L++)
      if (w[L] < 16 || w[L] > MAX_WIDTH || w[L] % 16 != 0) {
        snprintf(msg, sizeof msg, "%s_width[%d] must be a multiple of 16 in [16, 256]", second ? x : "pi", L);
        return false;
      }
  }
  return true;
}

// The blob's plan for a shape -> its size in floats; 0 and `why` (a message that names the field) for a refused shape.
inline int64_t plan(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_vf, const int32_t* vf_width, Pol* P, const char** why) {
  if (!checked_shape(obs_dim, act_dim, n_pi, pi_width, n_vf, vf_width, "vf", true, why)) return 0;
  const int kb0 = (obs_dim + 6 + 3) / 4;
  int64_t at = 0;
  for (int k = 1; k >= 0; k--) {         // the policy net first
    const int n = k ? n_pi : n_vf;
    const int32_t* w = k ? pi_width : vf_width;
    Net net = {};
    net.n = n;
    for (int L = 0; L <= n; L++) {
      const int out_tiles = L < n ? w[L] / 16 : 1, nkb = L == 0 ? kb0 : w[L - 1] / 4;
      if (L < n) net.nt[L] = out_tiles;
      net.w[L] = (int)at; at += (int64_t)out_tiles * nkb * WAVE;
      net.b[L] = (int)at; at += (int64_t)out_tiles * 16;
    }
    if (P) P->net[k] = net;
  }
  if (P) { P->log_std = (int)at; P->kb0 = kb0; P->D = obs_dim; P->A = act_dim; }
  return at + 16;                        // < 2^21 floats at the largest shape
}

// What every entry checks of an mcg_policy before it launches -> the blob's size, and P filled but for N; 0 after mcg_fail.
inline int64_t checked_plan(const char* who, const mcg_policy* pol, Pol* P) {
  if (!pol) { mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy", who); return 0; }
  if (!pol->blob) { mcg_fail(MCG_ERR_ARG, "%s: blob is null", who); return 0; }
  const char* why = nullptr;
  const int64_t floats = plan(pol->obs_dim, pol->act_dim, pol->n_pi, pol->pi_width, pol->n_vf, pol->vf_width, P, &why);
  if (floats == 0) { mcg_fail(MCG_ERR_ARG, "%s: %s", who, why); return 0; }
  if (pol->activation != MCG_POLICY_TANH && pol->activation != MCG_POLICY_RELU) {
    mcg_fail(MCG_ERR_ARG, "%s: activation must be MCG_POLICY_TANH or MCG_POLICY_RELU", who); return 0; }
  if (pol->blob_floats != floats) {
    mcg_fail(MCG_ERR_ARG, "%s: blob_floats is %lld, mcg_policy_blob_floats gives %lld for this shape", who, (long long)pol->blob_floats,
             (long long)floats);
    return 0;
  }
  if (((uintptr_t)pol->blob & 15) != 0) { mcg_fail(MCG_ERR_ARG, "%s: blob is not 16-byte aligned", who); return 0; }
  P->blob = pol->blob; P->act = pol->activation;
  return floats;
}

inline int widest_layer(const mcg_policy* pol) {
  int widest = 0;
  for (int L = 0; L < pol->n_pi; L++) widest = pol->pi_width[L] > widest ? pol->pi_width[L] : widest;
  for (int L = 0; L < pol->n_vf; L++) widest = pol->vf_width[L] > widest ? pol->vf_width[L] : widest;
  return widest;
}

// The B every entry over rows accepts (B * MAX_ACT indexes in int); silent, for the *_work_floats entries.
inline bool rows_in_range(int64_t B) { return B >= 1 && B * MAX_ACT < (1ll << 31); }

// The same, refused in the entry's name.
inline bool checked_rows(const char* who, int64_t B) {
  if (rows_in_range(B)) return true;
  if (B < 1) mcg_fail(MCG_ERR_ARG, "%s: B must be >= 1", who);
  else mcg_fail(MCG_ERR_ARG, "%s: B must be below 2^27", who);
  return false;
}

}  // namespace
