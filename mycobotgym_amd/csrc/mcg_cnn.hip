// mcg_cnn.hip -- the CNN actor-critic forward for the -v1 picture ids (include/mcg.h: mcg_cnn_*): SB3's CnnPolicy -- a NatureCNN
// features extractor shared by actor and critic, the two heads directly on its features, a diagonal Gaussian -- reading the uint8
// pictures where the environment, FrameStack or a buffer left them and writing action, value and log-prob in the forms
// mcg_rollout_img_add takes.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  Kernels and C entries are both here.  The
// C side is stateless; of mcg_engine.hpp it uses the error reporting alone.
//
// ---- Two launches.  cnn_conv_kernel: the three convolutions as implicit GEMMs (no im2col buffer anywhere), a workgroup of four waves
// per E pictures, each layer's activations in LDS, the third layer's output -- the flattened features of the extractor's cnn, 64 o3^2
// floats per picture -- to a scratch in global memory.  cnn_dense_kernel: Linear(64 o3^2, F) + ReLU, the two heads and the Gaussian on
// tiles of 32 rows, a workgroup of four waves per tile.  Every product is the transposed one of mcg_policy.hip's head on
// v_mfma_f32_16x16x4_f32, float32 in and out:
//     D[unit][column] += W[unit][k] * X[k][column]      A operand: 16 units x 4 k of the weights, B operand: 4 k x 16 columns
// Lane l = 16 g + i holds A[i][g] and B[g][i], and afterwards D[4 g + r][i] in register r.  A column is an output position of a
// picture (convolutions) or a row of the batch (dense stage).
//
// ---- The k order.  Every layer's K is a multiple of 16 (C 64, 512, 576, 64 o3^2, F), and every layer is packed as _nets.py packs a
// later layer: k-block 4 t + r, lane group g <-> natural k = 16 t + 4 g + r, natural meaning PyTorch's weight.reshape(out, -1), that is
// (c, ky, kx) for a convolution.  So a lane's B operands of the four instructions of chunk t are four CONSECUTIVE natural k: for conv1
// four neighbouring pixels of one row (c = t / 4, ky = 2 (t % 4) + g / 2, kx = 4 (g % 2) + r), for conv2 one row of the window
// (c = t, ky = g, kx = r), for the linear layer and the heads one aligned 16-byte load.  conv3's window of 9 has no such structure:
// its lanes divide k by 9 and 3.
//
// ---- The convolution kernel's work split.  The columns of a layer are the positions of all E pictures of the workgroup, picture
// after picture, in tiles of 16; a wave keeps up to NP = 4 column tiles' accumulators per tile of 16 output channels, so that a
// weight operand (one coalesced 256-byte load from global memory / L2) serves four instructions.  conv1 has two channel tiles: every
// wave takes both, on every fourth group of four column tiles, so that a gathered pixel serves two instructions; conv2 and conv3 have
// four: wave w takes tile w.  A ragged last column tile computes on the last valid position and stores nothing.  conv1 gathers its B
// operand from the picture in global memory (environment and channel strides in elements: the [N, C, S, S] view of [C, N, S, S] planes
// and a contiguous tensor are both read in place); a byte becomes byte / 255 through a table of the 256 quotients in LDS, each formed
// once per workgroup by the IEEE division, so the bits are the division's (against dividing every pixel in every window it falls
// into, and one channel tile per wave: 0.79 -> 0.74 ms at C = 1 and 1.25 -> 1.01 ms at C = 4, 8192 pictures of 64 x 64).  conv2 and
// conv3 gather from LDS with computed addresses.  LDS: E (32 o1^2 + 64 o2^2) floats and the table's 1 KB; E is the largest of 4, 3, 2,
// 1 that keeps it within 64 KB (S = 64: one picture, 39 KB; S <= 43: four), and a single picture above that (S >= 84) asks for up to
// 94 KB of the 160 KB.
//
// ---- The dense kernel's work split.  The F / 16 unit tiles of the linear layer are dealt to the four waves (tile T to wave T % 4, at
// most 8 each), both row tiles' accumulators per unit tile, so that a weight operand serves two instructions and the 2 MB of weights at
// F = 512 are read once per 32 rows.  The features go to LDS (float4 (k / 4, row): what a head's lane reads is one 16-byte slot, the
// lanes of a row tile side by side), then wave w takes row tile w % 2 and head w / 2 (0: value_net, 1: action_net and the Gaussian).
//
// ---- The blob (float32; mycobotgym_amd/cnn_policy.py: pack / unpack restate it).  In this order, each layer as its tiles
// (tile (T, kb), float 16 g + i = W[16 T + i][k(kb, g)], k as above) then its bias: conv1 [32, 64 C], conv2 [64, 512], conv3 [64, 576],
// linear [F, 64 o3^2], action_net (A rows padded with zeros to 16) [16, F], value_net (1 row padded to 16) [16, F]; then log_std padded
// to 16.  Every piece is a multiple of 16 floats.
//
// ---- The noise and the Gaussian head: mcg_policy.hpp's (gauss4's counter layout, stated at mcg_policy.hip's head), with a domain byte
// of its own, DOMAIN_CNN (enum Domain, mcg_philox.hpp).
//
// ---- Order.  No atomics; every sum's order is fixed by the shape alone, and a row's depends on neither its place in the batch nor
// on the batch's size: equal pictures and equal global ids give equal bits.
#include <type_traits>

#include "mcg_policy.hpp"        // f4, mfma, WAVE, MAX_ACT, rows_in_range, EvalOut, the Gaussian head; mcg_buffer.hpp: blocks, launched, mcg_fail

using namespace mcg;

namespace {

constexpr int WAVES = 4, LANES = WAVE * WAVES, NP = 4, ROWS = 32, MAXM = 8;
constexpr int MIN_S = 36, MAX_S = 96, MAX_C = 16, MAX_F = 512, MAX_E = 4;
constexpr int LDS_SOFT = 64 * 1024, QUOTIENT_BYTES = 256 * (int)sizeof(float);

struct Cnn {                             // mcg_cnn_policy as the kernels see it; offsets into the blob in floats
  const float* blob;
  int C, S, F, A, o1, o2, o3, n1, n2, n3, K3;
  int w1, b1, w2, b2, w3, b3, wl, bl, wa, ba, wv, bv, log_std;
};
struct Out { float *action, *value, *log_prob, *mean, *noise, *features; };

// byte / 255 for all 256 bytes, by the first 256 lanes of a workgroup: the correctly rounded quotient (IEEE division, nothing
// reciprocal), formed once per byte value instead of once per pixel and window
MCG_DEV void quotient_of(float* table, int lane) {
  if (lane < 256) table[lane] = (float)lane / 255.0f;
}

// Channel tiles T .. T + MT - 1 of a layer of `chunks` chunks of 16 k, on the column tiles pt0 .. of the Q columns (at most NP of them):
//   prep(q)              what gather needs of column q (an offset), computed once
//   gather(t, g, at, x)  the four B operands of chunk t: natural k = 16 t + 4 g + r, r = 0..3; they serve all MT channel tiles
//   store(q, ch, v)      max(., 0) of channels ch .. ch + 3 of column q
template <int MT, class Prep, class Gather, class Store>
MCG_DEV void conv_tiles(const float* __restrict__ W, const float* __restrict__ bias, int chunks, int T, int pt0, int tiles, int Q, int lane,
                        Prep prep, Gather gather, Store store) {
  const int g = lane >> 4, i = lane & 15;
  const int np = tiles - pt0 < NP ? tiles - pt0 : NP;
  decltype(prep(0)) at[NP];
  f4 acc[MT][NP];
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const int q = (pt0 + j) * 16 + i;
    at[j] = prep(q < Q ? q : Q - 1);     // a ragged tile's extra columns compute on a valid position and store nothing
#pragma unroll
    for (int m = 0; m < MT; m++) acc[m][j] = *reinterpret_cast<const f4*>(bias + 16 * (T + m) + 4 * g);
  }
  const float* __restrict__ Wt = W + (size_t)T * chunks * 4 * WAVE + lane;
  for (int t = 0; t < chunks; t++) {
    float a[MT][4];
#pragma unroll
    for (int m = 0; m < MT; m++)
#pragma unroll
      for (int r = 0; r < 4; r++) a[m][r] = Wt[((size_t)m * chunks * 4 + 4 * t + r) * WAVE];
#pragma unroll
    for (int j = 0; j < NP; j++) {
      if (j < np) {
        float x[4];
        gather(t, g, at[j], x);
#pragma unroll
        for (int r = 0; r < 4; r++)
#pragma unroll
          for (int m = 0; m < MT; m++) acc[m][j] = mfma(a[m][r], x[r], acc[m][j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NP; j++) {
    const int q = (pt0 + j) * 16 + i;
    if (j < np && q < Q) {
#pragma unroll
      for (int m = 0; m < MT; m++) {
        f4 v = acc[m][j];
#pragma unroll
        for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.0f);
        store(q, 16 * (T + m) + 4 * g, v);
      }
    }
  }
}

// In: uint8_t, or float (already divided by 255).  es, cs: the picture's environment and channel strides in elements.
template <class In>
__global__ __launch_bounds__(LANES) void cnn_conv_kernel(Cnn P, const In* __restrict__ pix, long long es, long long cs, long long rows, int E,
                                                         float* __restrict__ feat) {
  extern __shared__ __attribute__((aligned(16))) float lds[];
  float* const l1 = lds;                                     // [E][32][o1^2]
  float* const l2 = lds + (size_t)E * 32 * P.n1;             // [E][64][o2^2]
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long row0 = (long long)blockIdx.x * E;
  const int S = P.S, o1 = P.o1, o2 = P.o2, o3 = P.o3, n1 = P.n1, n2 = P.n2, n3 = P.n3;
  float* const quotient = l2 + (size_t)E * 64 * n2;          // [256]: byte / 255 (a uint8 picture)
  if constexpr (std::is_same_v<In, uint8_t>) {
    quotient_of(quotient, threadIdx.x);
    __syncthreads();
  }
  {  // ---- conv1: the picture -> l1; both channel tiles on every wave, so that a gathered pixel serves two instructions
    const int Q = E * n1, tiles = (Q + 15) / 16;
    for (int pt0 = w * NP; pt0 < tiles; pt0 += WAVES * NP)
      conv_tiles<2>(P.blob + P.w1, P.blob + P.b1, 4 * P.C, 0, pt0, tiles, Q, lane,
                 [&](int q) {
                   const int e = q / n1, p = q - e * n1, oy = p / o1, ox = p - oy * o1;
                   const long long row = row0 + e < rows ? row0 + e : rows - 1;      // a ragged group's extra pictures read the last one
                   return row * es + (long long)(4 * oy) * S + 4 * ox;
                 },
                 [&](int t, int g, long long at, float (&x)[4]) {
                   const In* __restrict__ from = pix + at + (long long)(t >> 2) * cs + (2 * (t & 3) + (g >> 1)) * S + 4 * (g & 1);
#pragma unroll
                   for (int r = 0; r < 4; r++) {
                     if constexpr (std::is_same_v<In, uint8_t>) x[r] = quotient[from[r]];
                     else x[r] = from[r];
                   }
                 },
                 [&](int q, int ch, f4 v) {
                   const int e = q / n1, p = q - e * n1;
#pragma unroll
                   for (int r = 0; r < 4; r++) l1[(e * 32 + ch + r) * n1 + p] = v[r];
                 });
  }
  __syncthreads();
  {  // ---- conv2: l1 -> l2
    const int Q = E * n2, tiles = (Q + 15) / 16;
    for (int pt0 = 0; pt0 < tiles; pt0 += NP)
      conv_tiles<1>(P.blob + P.w2, P.blob + P.b2, 32, w, pt0, tiles, Q, lane,
                 [&](int q) {
                   const int e = q / n2, p = q - e * n2, oy = p / o2, ox = p - oy * o2;
                   return e * 32 * n1 + 2 * oy * o1 + 2 * ox;
                 },
                 [&](int t, int g, int at, float (&x)[4]) {
                   const float* from = l1 + at + t * n1 + g * o1;
#pragma unroll
                   for (int r = 0; r < 4; r++) x[r] = from[r];
                 },
                 [&](int q, int ch, f4 v) {
                   const int e = q / n2, p = q - e * n2;
#pragma unroll
                   for (int r = 0; r < 4; r++) l2[(e * 64 + ch + r) * n2 + p] = v[r];
                 });
  }
  __syncthreads();
  {  // ---- conv3: l2 -> the scratch, flattened in PyTorch's order c o3^2 + y o3 + x
    const int Q = E * n3, tiles = (Q + 15) / 16;
    for (int pt0 = 0; pt0 < tiles; pt0 += NP)
      conv_tiles<1>(P.blob + P.w3, P.blob + P.b3, 36, w, pt0, tiles, Q, lane,
                 [&](int q) {
                   const int e = q / n3, p = q - e * n3, oy = p / o3, ox = p - oy * o3;
                   return e * 64 * n2 + oy * o2 + ox;
                 },
                 [&](int t, int g, int at, float (&x)[4]) {
#pragma unroll
                   for (int r = 0; r < 4; r++) {
                     const int k = 16 * t + 4 * g + r, c = k / 9, rem = k - 9 * c, ky = rem / 3, kx = rem - 3 * ky;
                     x[r] = l2[at + c * n2 + ky * o2 + kx];
                   }
                 },
                 [&](int q, int ch, f4 v) {
                   const int e = q / n3, p = q - e * n3;
                   if (row0 + e < rows) {
#pragma unroll
                     for (int r = 0; r < 4; r++) feat[(size_t)(row0 + e) * P.K3 + (size_t)(ch + r) * n3 + p] = v[r];
                   }
                 });
  }
}

// EVAL = false: mcg_cnn_forward (O);  true: mcg_cnn_evaluate (actions, V).  `policy`: the action head and the Gaussian are wanted.
template <bool EVAL>
__global__ __launch_bounds__(LANES) void cnn_dense_kernel(Cnn P, const float* __restrict__ feat, long long rows, unsigned long long seed,
                                                          unsigned long long call, long long env_id_offset, int deterministic, int policy,
                                                          Out O, const float* __restrict__ actions, EvalOut V) {
  extern __shared__ __attribute__((aligned(16))) float hid[];      // [F / 4][ROWS] float4: units 4 u .. 4 u + 3 of a row
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, g = lane >> 4, i = lane & 15;
  const long long first = (long long)blockIdx.x * ROWS;
  const int nt = P.F / 16, chunks = P.K3 / 16;
  {  // ---- Linear(64 o3^2, F) + ReLU: this wave's unit tiles w, w + 4, .., both row tiles
    f4 acc[MAXM][2];
#pragma unroll
    for (int m = 0; m < MAXM; m++) {
      f4 b = {0.0f, 0.0f, 0.0f, 0.0f};
      if (w + WAVES * m < nt) b = *reinterpret_cast<const f4*>(P.blob + P.bl + 16 * (w + WAVES * m) + 4 * g);
      acc[m][0] = b; acc[m][1] = b;
    }
    const float* x0 = feat + (size_t)(first + i < rows ? first + i : rows - 1) * P.K3 + 4 * g;       // a ragged tile's extra rows read
    const float* x1 = feat + (size_t)(first + 16 + i < rows ? first + 16 + i : rows - 1) * P.K3 + 4 * g;      // the last one
    const float* __restrict__ W = P.blob + P.wl + lane;
    for (int t = 0; t < chunks; t++) {
      const f4 u0 = *reinterpret_cast<const f4*>(x0 + 16 * t), u1 = *reinterpret_cast<const f4*>(x1 + 16 * t);
#pragma unroll
      for (int m = 0; m < MAXM; m++) {
        if (w + WAVES * m < nt) {
          const float* __restrict__ Wt = W + ((size_t)(w + WAVES * m) * chunks * 4 + 4 * t) * WAVE;
#pragma unroll
          for (int r = 0; r < 4; r++) {
            const float a = Wt[r * WAVE];
            acc[m][0] = mfma(a, u0[r], acc[m][0]);
            acc[m][1] = mfma(a, u1[r], acc[m][1]);
          }
        }
      }
    }
#pragma unroll
    for (int m = 0; m < MAXM; m++) {
      const int T = w + WAVES * m;
      if (T < nt) {
#pragma unroll
        for (int rt = 0; rt < 2; rt++) {
          f4 v = acc[m][rt];
#pragma unroll
          for (int r = 0; r < 4; r++) v[r] = fmaxf(v[r], 0.0f);
          *reinterpret_cast<f4*>(hid + ((4 * T + g) * ROWS + 16 * rt + i) * 4) = v;
          const long long row = first + 16 * rt + i;
          if (!EVAL && O.features && row < rows) {
#pragma unroll
            for (int r = 0; r < 4; r++) O.features[(size_t)row * P.F + 16 * T + 4 * g + r] = v[r];
          }
        }
      }
    }
  }
  __syncthreads();
  // ---- the heads: row tile w % 2; w / 2 = 0: value_net, 1: action_net and the Gaussian
  const int rt = w & 1, k = w >> 1;
  const long long s = first + 16 * rt + i;
  const bool live = s < rows;
  const long long row = live ? s : rows - 1;
  if (first + 16 * rt >= rows) return;                        // (no row of this tile exists)
  if (k == 0 ? !(EVAL ? V.value : O.value) : !policy) return;
  f4 h = *reinterpret_cast<const f4*>(P.blob + (k ? P.ba : P.bv) + 4 * g);
  {
    const float* __restrict__ W = P.blob + (k ? P.wa : P.wv) + lane;
    for (int t = 0; t < nt; t++) {
      const f4 u = *reinterpret_cast<const f4*>(hid + ((4 * t + g) * ROWS + 16 * rt + i) * 4);
#pragma unroll
      for (int r = 0; r < 4; r++) h = mfma(W[(4 * t + r) * WAVE], u[r], h);
    }
  }                                      // lane 16 g + i: rows 4 g + r of the head, row i of the tile
  if (k == 0) {
    if (live && g == 0) (EVAL ? V.value : O.value)[s] = h[0];
    return;
  }
  const f4 ls = *reinterpret_cast<const f4*>(P.blob + P.log_std + 4 * g);
  if (EVAL) {                            // mcg_policy_evaluate's rule (mcg_policy.hpp); the derivative is not wanted
    f4 dmu, dls;
    const double lpd = gauss_log_prob(P.A, h, ls, actions, (size_t)row, g, dmu, dls);
    if (live && g == 0) {
      if (V.log_prob) V.log_prob[s] = (float)lpd;
      if (V.entropy) V.entropy[s] = gauss_entropy(P.A, P.blob + P.log_std);
    }
    return;
  }
  // ---- the diagonal Gaussian (mcg_policy.hpp): this lane has components 4 g .. 4 g + 3
  const Sampled d = gauss_sample(P.A, h, ls, g, seed, (unsigned long long)(env_id_offset + row), call, DOMAIN_CNN, deterministic);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < P.A && live) {
      const size_t at = (size_t)s * P.A + c;
      if (O.action) O.action[at] = d.action[r];
      if (O.mean) O.mean[at] = d.mean[r];
      if (O.noise) O.noise[at] = d.noise[r];
    }
  }
  if (O.log_prob && live && g == 0) O.log_prob[s] = d.log_prob;
}

// ------------------------------------------------------------------------------------------------------- host side
// The blob's plan for a shape -> its size in floats; 0 and `why` (a message that names the field) for a refused shape.
inline int64_t plan(int C, int S, int F, int A, Cnn* P, const char** why) {
  if (C < 1 || C > MAX_C) { *why = "channels must be in [1, 16]"; return 0; }
  if (S < MIN_S || S > MAX_S) { *why = "image_size must be in [36, 96]"; return 0; }
  if (F < 16 || F > MAX_F || F % 16 != 0) { *why = "features_dim must be a multiple of 16 in [16, 512]"; return 0; }
  if (A < 1 || A > MAX_ACT) { *why = "act_dim must be in [1, 16]"; return 0; }
  Cnn p = {};
  p.C = C; p.S = S; p.F = F; p.A = A;
  p.o1 = (S - 8) / 4 + 1; p.o2 = (p.o1 - 4) / 2 + 1; p.o3 = p.o2 - 2;
  p.n1 = p.o1 * p.o1; p.n2 = p.o2 * p.o2; p.n3 = p.o3 * p.o3; p.K3 = 64 * p.n3;
  int at = 0;                            // < 2^22 floats at the largest shape
  p.w1 = at; at += 32 * 64 * C; p.b1 = at; at += 32;
  p.w2 = at; at += 64 * 512;    p.b2 = at; at += 64;
  p.w3 = at; at += 64 * 576;    p.b3 = at; at += 64;
  p.wl = at; at += F * p.K3;    p.bl = at; at += F;
  p.wa = at; at += 16 * F;      p.ba = at; at += 16;
  p.wv = at; at += 16 * F;      p.bv = at; at += 16;
  p.log_std = at; at += 16;
  if (P) *P = p;
  return at;
}

// What both entries check before they launch -> MCG_OK with P filled; the code after mcg_fail.
inline int checked(const char* who, const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, int64_t rows, Cnn* P) {
  if (!pol) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_cnn_policy", who);
  if (!pol->blob) return mcg_fail(MCG_ERR_ARG, "%s: blob is null", who);
  const char* why = nullptr;
  const int64_t floats = plan(pol->channels, pol->image_size, pol->features_dim, pol->act_dim, P, &why);
  if (floats == 0) return mcg_fail(MCG_ERR_ARG, "%s: %s", who, why);
  if (pol->blob_floats != floats)
    return mcg_fail(MCG_ERR_ARG, "%s: blob_floats is %lld, mcg_cnn_blob_floats gives %lld for this shape", who, (long long)pol->blob_floats,
                    (long long)floats);
  if (((uintptr_t)pol->blob & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: blob is not 16-byte aligned", who);
  if (rows < 1) return mcg_fail(MCG_ERR_ARG, "%s: the number of rows (n_envs, rows) must be >= 1", who);
  if (!rows_in_range(rows)) return mcg_fail(MCG_ERR_ARG, "%s: the number of rows (n_envs, rows) must be below 2^27", who);
  if (!pol->scratch) return mcg_fail(MCG_ERR_ARG, "%s: scratch is null", who);
  if (((uintptr_t)pol->scratch & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: scratch is not 16-byte aligned", who);
  if (pol->scratch_floats < rows * P->K3)
    return mcg_fail(MCG_ERR_ARG, "%s: scratch_floats is %lld, mcg_cnn_scratch_floats gives %lld for this shape and %lld rows", who,
                    (long long)pol->scratch_floats, (long long)(rows * P->K3), (long long)rows);
  if (!obs) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_cnn_obs", who);
  if (!obs->pixels) return mcg_fail(MCG_ERR_ARG, "%s: pixels is null", who);
  if (obs->dtype != MCG_CNN_UINT8 && obs->dtype != MCG_CNN_FLOAT32)
    return mcg_fail(MCG_ERR_ARG, "%s: dtype must be MCG_CNN_UINT8 or MCG_CNN_FLOAT32", who);
  if (obs->env_stride < 0 || obs->chan_stride < 0) return mcg_fail(MCG_ERR_ARG, "%s: env_stride and chan_stride must be >= 0", who);
  if (pol->channels > 1 && obs->chan_stride < (int64_t)pol->image_size * pol->image_size)
    return mcg_fail(MCG_ERR_ARG, "%s: chan_stride must be >= image_size^2 (the S x S plane is contiguous)", who);
  P->blob = pol->blob;
  return MCG_OK;
}

// The two launches.  The LDS of the convolution kernel decides how many pictures a workgroup takes.
template <bool EVAL>
inline int launch(const char* what, const Cnn& P, const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, int64_t rows, unsigned long long seed,
                  unsigned long long call, long long env_id_offset, int deterministic, int policy, const Out& O, const float* actions,
                  const EvalOut& V, hipStream_t stream) {
  const size_t per = sizeof(float) * (32 * (size_t)P.n1 + 64 * (size_t)P.n2);
  int E = (int)((LDS_SOFT - QUOTIENT_BYTES) / per);
  E = E < 1 ? 1 : E > MAX_E ? MAX_E : E;
  const size_t conv_lds = per * E + QUOTIENT_BYTES;
  const dim3 cgrid(blocks(rows, E)), dgrid(blocks(rows, ROWS)), block(LANES);
  if (obs->dtype == MCG_CNN_UINT8) {
    if (conv_lds > (size_t)LDS_SOFT) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cnn_conv_kernel<uint8_t>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_lds);
      if (e != hipSuccess) return mcg_fail(MCG_ERR_HIP, "%s: %zu bytes of LDS: %s", what, conv_lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(cnn_conv_kernel<uint8_t>, cgrid, block, conv_lds, stream, P, static_cast<const uint8_t*>(obs->pixels),
                       (long long)obs->env_stride, (long long)obs->chan_stride, (long long)rows, E, pol->scratch);
  } else {
    if (conv_lds > (size_t)LDS_SOFT) {
      const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(&cnn_conv_kernel<float>), hipFuncAttributeMaxDynamicSharedMemorySize, (int)conv_lds);
      if (e != hipSuccess) return mcg_fail(MCG_ERR_HIP, "%s: %zu bytes of LDS: %s", what, conv_lds, hipGetErrorString(e));
    }
    hipLaunchKernelGGL(cnn_conv_kernel<float>, cgrid, block, conv_lds, stream, P, static_cast<const float*>(obs->pixels),
                       (long long)obs->env_stride, (long long)obs->chan_stride, (long long)rows, E, pol->scratch);
  }
  if (const int e = launched(what)) return e;
  hipLaunchKernelGGL(cnn_dense_kernel<EVAL>, dgrid, block, sizeof(float) * ROWS * (size_t)P.F, stream, P, pol->scratch, (long long)rows, seed,
                     call, env_id_offset, deterministic, policy, O, actions, V);
  return launched(what);
}

}  // namespace

extern "C" {

int64_t mcg_cnn_blob_floats(int channels, int image_size, int features_dim, int act_dim) {
  const char* why;
  return plan(channels, image_size, features_dim, act_dim, nullptr, &why);
}

int64_t mcg_cnn_scratch_floats(int channels, int image_size, int features_dim, int act_dim, int64_t rows) {
  const char* why;
  Cnn P = {};
  if (plan(channels, image_size, features_dim, act_dim, &P, &why) == 0 || !rows_in_range(rows)) return 0;
  return rows * P.K3;
}

int mcg_cnn_forward(const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, uint64_t seed, uint64_t call, int64_t env_id_offset,
                    int deterministic, const mcg_cnn_out* out, void* stream) {
  const char* who = "mcg_cnn_forward";
  Cnn P = {};
  if (const int e = checked(who, pol, obs, pol ? pol->n_envs : 0, &P)) return e;
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_cnn_out", who);
  if (!out->action && !out->value && !out->log_prob && !out->mean && !out->noise && !out->features)
    return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  const Out O = {out->action, out->value, out->log_prob, out->mean, out->noise, out->features};
  const int policy = (out->action || out->log_prob || out->mean || out->noise) ? 1 : 0;      // value alone: no policy-head work
  return launch<false>("mcg_cnn_forward", P, pol, obs, pol->n_envs, (unsigned long long)seed, (unsigned long long)call, (long long)env_id_offset,
                       deterministic != 0, policy, O, nullptr, EvalOut{}, (hipStream_t)stream);
}

int mcg_cnn_evaluate(const mcg_cnn_policy* pol, const mcg_cnn_obs* obs, const float* actions, int64_t rows,
                     const mcg_policy_eval_out* out, void* stream) {
  const char* who = "mcg_cnn_evaluate";
  Cnn P = {};
  if (const int e = checked(who, pol, obs, rows, &P)) return e;
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy_eval_out", who);
  if (!out->value && !out->log_prob && !out->entropy) return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  const int policy = (out->log_prob || out->entropy) ? 1 : 0;
  if (policy && !actions) return mcg_fail(MCG_ERR_ARG, "%s: actions is null", who);
  const EvalOut V = {out->value, out->log_prob, out->entropy};
  return launch<true>("mcg_cnn_evaluate", P, pol, obs, rows, 0ull, 0ull, 0ll, 1, policy, Out{}, actions, V, (hipStream_t)stream);
}

}  // extern "C"
