// mcg_grad.hpp -- what the three gradient code objects share, mcg_policy_grad.hip (PPO / A2C), mcg_sac_grad.hip (SAC) and
// mcg_td3_grad.hip (TD3 / DDPG): a net's row map of a tile in `work` and the block list of its dW products; in a tile kernel the
// tile sum, the features, activations and dZ kept as rows, the hidden layers' forward with their rows kept and the walk back through
// W^T; the dW kernel (one 16 x 16 block of dW = dZ X^T over a part's tiles); in a reduce kernel the sum of the partial blobs in part
// order and the 64-lane sum of a tile-sum slot; the workgroup sum in double; Adam's kernel.  On the host: the numbering of a net's
// rows, a layer's entry of the block list, the buffer checks and Adam's bias-correction scalars.  The three products and the work
// split are stated at the head of mcg_policy_grad.hip; each family's loss, head, tile kernels and statistics stay in its own file,
// and what takes a `Sac` is mcg_sac_grad.hpp's.
#pragma once

#include "mcg_policy.hpp"

namespace {

constexpr int PARTS_NARROW = 16, PARTS_WIDE = 4;
constexpr int ALL_COLUMNS = 1 << 30;
constexpr int MAX_BLOCK_LAYERS = 2 * (MAX_LAYERS + 2);
static_assert(MAX_BLOCK_LAYERS >= 2 * (MAX_LAYERS + 1) + 1, "PPO's blob: per net its layers and the head, and log_std");
static_assert(MAX_BLOCK_LAYERS >= 2 * (MAX_LAYERS + 2), "a critic blob: per critic its layers, the head, the action tiles");

struct GRows {                           // a net's rows of a tile in `work`, in rows of 16 floats
  int x[MAX_LAYERS + 1];                 // x[L]: the input of layer L (x[0]: the features, fr rows; x[n]: the heads' input)
  int d[MAX_LAYERS + 1];                 // d[L]: dZ of layer L (d[n]: the head's -- SAC's actor: mu's -- 16 rows)
  int xa, d2, rows, fr;                  // the action's 16 rows (a critic); a second head's dZ rows (SAC's actor: log_std's head; PPO's
                                         // policy net: the log_std terms); rows in all; feature rows (D + 6 padded to 16)
  long long base, stride;                // the net's first float in `work`; from critic 0's chunks to critic 1's
};
struct Block {                           // one layer's blocks of the dW product: nT rows of (ncb blocks of 16 columns, then nb bias blocks)
  int blk0, nT, ncb, xrow, drow, w, b, nkb, first, rows;
  int cols, nb;                          // columns from `cols` on are padding, written +0; nb: 1 with the bias, 0 without
  long long base;
};
struct Blocks { Block l[MAX_BLOCK_LAYERS]; int n, total; };

// the sum over the 16 samples of a tile, in an order that does not depend on the data (every lane gets it)
MCG_DEV float sum16(float x) {
  x += __shfl_xor(x, 8); x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
  return x;
}

// the sum over the wave's 64 lanes, as a reduce kernel sums a tile-sum slot (every lane gets it)
template <class T>
MCG_DEV T sum64(T x) {
  for (int m = 32; m >= 1; m >>= 1) x += __shfl_xor(x, m);
  return x;
}

// rows `at + 16 t + 4 g + r` of the tile's chunk <- register r of tile t (the accumulator layout), sample i
template <int MT>
MCG_DEV void store_rows(float* chunk, int at, int nt, const f4 (&v)[MT], int g, int i) {
#pragma unroll
  for (int t = 0; t < MT; t++)
    if (t < nt) {
#pragma unroll
      for (int r = 0; r < 4; r++) chunk[(size_t)(at + 16 * t + 4 * g + r) * TILE + i] = v[t][r];
    }
}

// the features as rows: a first layer's X (columns from D + 6 on are zeros)
MCG_DEV void store_features(float* chunk, int at, int fr, int D, const float* obs, const float* ach, const float* des, int row, int g, int i) {
  for (int f = g; f < fr; f += 4) {
    float x = 0.0f;
    if (f < 3) x = ach[(size_t)row * 3 + f];
    else if (f < 6) x = des[(size_t)row * 3 + (f - 3)];
    else if (f < D + 6) x = obs[(size_t)row * D + (f - 6)];
    chunk[(size_t)(at + f) * TILE + i] = x;
  }
}

// a: a first layer's sums -> the last hidden layer's activations, as mcg_sac.hpp's hidden(); where `keep` (this wave keeps the rows),
// every layer's activations are stored as the rows x[1..n] of the chunk: the inputs of the layers 1..n.
template <int MT>
MCG_DEV void hidden_rows(const Pol& P, const Net& net, const GRows& R, float* chunk, bool keep, f4 (&a)[MT], int g, int i, int lane) {
  f4 b[MT];
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, a[t][r]);
  if (keep) store_rows<MT>(chunk, R.x[1], net.nt[0], a, g, i);
  for (int L = 1; L < net.n; L++) {
    dense<MT, MT>(P, net, L, L == 1 ? net.nt[0] : net.nt[1], L == 1 ? net.nt[1] : net.nt[2], a, b, g, lane);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, b[t][r]);
    if (keep) store_rows<MT>(chunk, L == 1 ? R.x[2] : R.x[3], L == 1 ? net.nt[1] : net.nt[2], a, g, i);
  }
}

// c + tile T of W^T dZ: W a layer's tiles over nkb k-blocks, dZ its nto tiles in the accumulator layout (mcg_policy_grad.hip's head)
template <int MT>
MCG_DEV f4 wt_acc(const float* __restrict__ W, int nkb, int T, int nto, const f4 (&d)[MT], f4 c, int g, int i) {
#pragma unroll
  for (int t = 0; t < MT; t++) {
    if (t < nto) {
      const f4 w = *reinterpret_cast<const f4*>(W + (size_t)(t * nkb + 4 * T + (i & 3)) * WAVE + 16 * (i >> 2) + 4 * g);
#pragma unroll
      for (int r = 0; r < 4; r++) c = mfma(w[r], d[t][r], c);
    }
  }
  return c;
}

// act'(y) by the activation's output y: tanh' = 1 - y^2, relu' = [y > 0]
MCG_DEV float act_prime(int act, float y) { return act == MCG_POLICY_TANH ? 1.0f - y * y : (y > 0.0f ? 1.0f : 0.0f); }

// d: dZ of layer `from` of `net` (the head: from = n) -> dZ of layer `to` (act'(y) (W^T dZ), layer by layer), each stored as rows where
// STORE.  The activations are re-read from the chunk, as this lane stored them.
template <int MT, bool STORE>
MCG_DEV void walk_back(const Pol& P, const Net& net, const GRows& R, float* chunk, int from, int to, f4 (&d)[MT], int g, int i) {
  f4 e[MT];
  for (int L = from; L > to; L--) {
    const int nto = L == net.n ? 1 : (L == 1 ? net.nt[1] : net.nt[2]);          // tiles of dZ_L: the product's k
    const int nti = L == 1 ? net.nt[0] : L == 2 ? net.nt[1] : net.nt[2];        // tiles of layer L's input: the product's rows
    const float* __restrict__ W = P.blob + sel4(net.w, L);
    const float* y = chunk + (size_t)sel4(R.x, L) * TILE;
#pragma unroll
    for (int T = 0; T < MT; T++) {
      e[T] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (T < nti) {
        f4 c = wt_acc<MT>(W, 4 * nti, T, nto, d, f4{0.0f, 0.0f, 0.0f, 0.0f}, g, i);
#pragma unroll
        for (int r = 0; r < 4; r++) c[r] *= act_prime(P.act, y[(size_t)(16 * T + 4 * g + r) * TILE + i]);
        e[T] = c;
      }
    }
    if (STORE) store_rows<MT>(chunk, sel4(R.d, L - 1), nti, e, g, i);
#pragma unroll
    for (int t = 0; t < MT; t++) d[t] = e[t];
  }
}

// One 16 x 16 block `blk` of dW (or 16 biases) over the tiles of one part -> its place in the part's partial blob.
MCG_DEV void dw_block(const Block& me, int blk, int part, const float* __restrict__ work, float* __restrict__ partials, long long blob_floats,
                      int ntiles, int tpp) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int local = blk - me.blk0, T = local / (me.ncb + me.nb), cb = local % (me.ncb + me.nb);
  const bool bias = cb == me.ncb;
  const int t0 = part * tpp, t1 = min(t0 + tpp, ntiles);
  const size_t stride = (size_t)me.rows * TILE;
  const float* __restrict__ A = work + me.base + (size_t)(me.drow + 16 * T + i) * TILE + 4 * g;
  const float* __restrict__ Bm = work + me.base + (size_t)(me.xrow + (bias ? 0 : 16 * cb) + i) * TILE + 4 * g;
  f4 acc = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = t0; t < t1; t++) {
    const f4 a4 = *reinterpret_cast<const f4*>(A + t * stride);
    f4 b4 = {1.0f, 1.0f, 1.0f, 1.0f};
    if (!bias) b4 = *reinterpret_cast<const f4*>(Bm + t * stride);
#pragma unroll
    for (int q = 0; q < 4; q++) acc = mfma(a4[q], b4[q], acc);
  }
  float* out = partials + (size_t)part * blob_floats;          // register r: dW[16 T + 4 g + r][16 cb + i]
  if (bias) {
    if (i == 0) *reinterpret_cast<f4*>(out + me.b + 16 * T + 4 * g) = acc;
    return;
  }
  if (16 * cb + i >= me.cols) acc = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (me.first) {                        // column 16 cb + i = 4 kb + g': tile (T, kb), float 16 g' + 4 g + r
    const int kb = 4 * cb + (i >> 2);
    if (kb < me.nkb) *reinterpret_cast<f4*>(out + me.w + (size_t)(T * me.nkb + kb) * WAVE + 16 * (i & 3) + 4 * g) = acc;
  } else {                               // column 16 cb + i = 16 t + 4 g' + r': tile (T, 4 t + r'), float 16 g' + 4 g + r
    *reinterpret_cast<f4*>(out + me.w + (size_t)(T * me.nkb + 4 * cb + (i & 3)) * WAVE + 16 * (i >> 2) + 4 * g) = acc;
  }
}

// The dW kernel: one wave per block of the list and part.
__global__ __launch_bounds__(WAVE) void dw_kernel(Blocks Q, const float* __restrict__ work, float* __restrict__ partials, long long blob_floats,
                                                  int ntiles, int tpp) {
  const int blk = blockIdx.x, part = blockIdx.y;
  Block me = Q.l[0];
#pragma unroll
  for (int q = 1; q < MAX_BLOCK_LAYERS; q++)
    if (q < Q.n && blk >= Q.l[q].blk0) me = Q.l[q];              // (constant indices: selects, no scratch)
  dw_block(me, blk, part, work, partials, blob_floats, ntiles, tpp);
}

// position p of the partial blobs' sum, in part order
MCG_DEV float sum_parts(const float* __restrict__ partials, int parts, long long blob_floats, long long p) {
  float sum = partials[p];
  for (int q = 1; q < parts; q++) sum += partials[(size_t)q * blob_floats + p];
  return sum;
}

// A reduce kernel's blocks but the last: grad[p] = sum_parts, less `less` on the n positions from `at` on (PPO's entropy term on
// log_std) -> true; false in the last block, which sums the tiles' slots into the family's stats.
MCG_DEV bool reduced_parts(const float* __restrict__ partials, int parts, long long blob_floats, float* __restrict__ grad, int at = 0, int n = 0,
                           float less = 0.0f) {
  if (!(blockIdx.x < gridDim.x - 1)) return false;
  const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
  if (p < blob_floats) {
    float sum = sum_parts(partials, parts, blob_floats, p);
    if (p >= at && p < at + n) sum -= less;
    grad[p] = sum;
  }
  return true;
}

// the sum over a workgroup of 1024 in a fixed tree (every thread gets it)
MCG_DEV double block_sum(double x, double* lds) {
  const int t = threadIdx.x;
  __syncthreads();
  lds[t] = x;
  __syncthreads();
  for (int m = 512; m >= 1; m >>= 1) {
    if (t < m) lds[t] += lds[t + m];
    __syncthreads();
  }
  return lds[0];
}

// torch.optim.Adam's rule on one element, without amsgrad or weight decay; step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step);
// omb1, omb2: 1 - beta1 and 1 - beta2 as the caller rounds them
MCG_DEV void adam_one(float* __restrict__ p, float gj, float* __restrict__ m, float* __restrict__ v, long long j, float beta1, float beta2,
                      float omb1, float omb2, float step_size, float bc2_sqrt, float eps) {
  const float mj = beta1 * m[j] + omb1 * gj;
  const float vj = beta2 * v[j] + omb2 * (gj * gj);
  m[j] = mj;
  v[j] = vj;
  p[j] = p[j] - step_size * (mj / (sqrtf(vj) / bc2_sqrt + eps));
}

// Adam on a blob in place; norm: the gradient's norm for clip-by-norm to max_norm, or null for no clipping.  THREADS: the block's size
// (a template: only the code objects that launch it hold it).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void adam_kernel(float* __restrict__ p, const float* __restrict__ grad, float* __restrict__ m,
                                                   float* __restrict__ v, long long n, const float* __restrict__ norm, float max_norm,
                                                   float beta1, float beta2, float omb1, float omb2, float step_size, float bc2_sqrt, float eps) {
  const long long j = (long long)blockIdx.x * THREADS + threadIdx.x;
  if (j >= n) return;
  const float coef = norm ? fminf(1.0f, max_norm / (norm[0] + 1e-6f)) : 1.0f;
  adam_one(p, grad[j] * coef, m, v, j, beta1, beta2, omb1, omb2, step_size, bc2_sqrt, eps);
}

// ------------------------------------------------------------------------------------------------------- host side
// the split of ntiles tiles into parts: tiles per part, parts
inline void split_parts(int ntiles, int widest, int* tpp, int* parts) {
  const int max_parts = widest <= 64 ? PARTS_NARROW : PARTS_WIDE;
  *tpp = (ntiles + max_parts - 1) / max_parts;
  *parts = (ntiles + *tpp - 1) / *tpp;
}

// x[1..n] of `net` from `row` on -> the row after them
inline int number_inputs(GRows& R, const Net& net, int row) {
  for (int L = 0; L < net.n; L++) { R.x[L + 1] = row; row += 16 * net.nt[L]; }
  return row;
}

// A net's rows: fr feature rows, the action's 16 rows where `action`, x[1..n], d[0..n] -> the row after them
inline int number_rows(GRows& R, const Net& net, int fr, bool action) {
  int row = fr;
  R.fr = fr; R.x[0] = 0;
  if (action) { R.xa = row; row += 16; }
  row = number_inputs(R, net, row);
  for (int L = 0; L <= net.n; L++) { R.d[L] = row; row += L < net.n ? 16 * net.nt[L] : 16; }
  return row;
}

// The Block of layer L of `net` (the head: L = n) from its row map; P: the first layer's columns (D, kb0).  blk0 is add_block's.
inline Block layer_block(const Pol& P, const Net& net, const GRows& R, int L) {
  Block b = {};
  b.nT = L < net.n ? net.nt[L] : 1; b.ncb = L == 0 ? R.fr / 16 : net.nt[L - 1]; b.nb = 1;
  b.xrow = R.x[L]; b.drow = R.d[L]; b.w = net.w[L]; b.b = net.b[L];
  b.nkb = L == 0 ? P.kb0 : 4 * net.nt[L - 1]; b.first = L == 0; b.cols = L == 0 ? P.D + 6 : ALL_COLUMNS;
  b.rows = R.rows; b.base = R.base;
  return b;
}

inline void add_block(Blocks& Q, int& blk, const Block& b) {
  Block& o = Q.l[Q.n++];
  o = b;
  o.blk0 = blk;
  blk += o.nT * (o.ncb + o.nb);
}

inline bool checked_buffer(const char* who, const void* p, const char* name) {
  if (!p) { mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is null", who, name); return false; }
  if (((uintptr_t)p & 15) != 0) { mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is not 16-byte aligned", who, name); return false; }
  return true;
}

// covers: the entry whose figure is enough for both layouts (mcg_sac_grad_work_floats, mcg_td3_grad_work_floats)
inline bool checked_work(const char* who, const float* work, int64_t work_floats, long long need, const char* covers) {
  if (!checked_buffer(who, work, "work")) return false;
  if (work_floats < need) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: work_floats is %lld, this entry needs %lld for this shape and B (%s covers both)", who,
                  (long long)work_floats, need, covers);
    return false;
  }
  return true;
}

// Adam's bias-correction scalars at `step`: step_size = lr / (1 - beta1^step), bc2_sqrt = sqrt(1 - beta2^step)
struct AdamStep { float step_size, bc2_sqrt; };
inline AdamStep adam_step(int64_t step, double lr, double beta1, double beta2) {
  const double bc1 = 1.0 - std::pow(beta1, (double)step), bc2 = 1.0 - std::pow(beta2, (double)step);
  return {(float)(lr / bc1), (float)std::sqrt(bc2)};
}

}  // namespace
