// mcg_grad.hpp -- what the two gradient code objects share, mcg_policy_grad.hip (PPO / A2C) and mcg_sac_grad.hip (SAC): the tile sum,
// the activation and dZ rows in `work`, the walk of one 16 x 16 block of dW = dZ X^T over a part's
// tiles, the sum of the partial blobs in part order, the workgroup sum in double, and Adam's elementwise rule.  The three products and
// the work split are stated at the head of mcg_policy_grad.hip; each file's own loss, row map and block list stay in that file.
#pragma once

#include "mcg_policy.hpp"

namespace {

constexpr int PARTS_NARROW = 16, PARTS_WIDE = 4;
constexpr int ALL_COLUMNS = 1 << 30;

struct Block {                           // one layer's blocks of the dW product: nT rows of (ncb blocks of 16 columns, then nb bias blocks)
  int blk0, nT, ncb, xrow, drow, w, b, nkb, first, rows;
  int cols, nb;                          // columns from `cols` on are padding, written +0; nb: 1 with the bias, 0 without
  long long base;
};

// the split of ntiles tiles into parts: tiles per part, parts
inline void split_parts(int ntiles, int widest, int* tpp, int* parts) {
  const int max_parts = widest <= 64 ? PARTS_NARROW : PARTS_WIDE;
  *tpp = (ntiles + max_parts - 1) / max_parts;
  *parts = (ntiles + *tpp - 1) / *tpp;
}

// the sum over the 16 samples of a tile, in an order that does not depend on the data (every lane gets it)
MCG_DEV float sum16(float x) {
  x += __shfl_xor(x, 8); x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
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

// position p of the partial blobs' sum, in part order
MCG_DEV float sum_parts(const float* __restrict__ partials, int parts, long long blob_floats, long long p) {
  float sum = partials[p];
  for (int q = 1; q < parts; q++) sum += partials[(size_t)q * blob_floats + p];
  return sum;
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

}  // namespace
