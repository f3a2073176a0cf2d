// mcg_sac_grad.hpp -- what the two off-policy gradient code objects share, mcg_sac_grad.hip (SAC) and mcg_td3_grad.hip (TD3 / DDPG):
// a net's row map of a tile in `work`, the block list of the dW kernel, the critic's forward with the action as an operand and its
// rows kept, and the walk back through a net.  mcg_sac_grad.hip's head states the work split and the layout of `work`; each file's own
// loss, tile kernels and layouts stay in that file.
#pragma once

#include "mcg_grad.hpp"         // sum16, store_rows, Block, dw_block, sum_parts, block_sum, adam_one
#include "mcg_sac.hpp"          // Sac, Draw, squash, sac_plan, checked_sac

namespace {

constexpr int SAC_BLOCK_LAYERS = 2 * (MAX_LAYERS + 2);       // the critic blob: per critic its layers, the head, the action tiles

struct GRows {                           // a net's rows of a tile in `work`, in rows of 16 floats
  int x[MAX_LAYERS + 1];                 // x[L]: the input of layer L (x[0]: the features, fr rows; x[n]: the heads' input)
  int d[MAX_LAYERS + 1];                 // d[L]: dZ of layer L (d[n]: the head's -- the actor: mu's -- 16 rows)
  int xa, d2, rows, fr;                  // the action's 16 rows (a critic); the log_std head's dZ (the actor); rows in all; feature rows
  long long base, stride;                // the net's first float in `work`; from critic 0's chunks to critic 1's
};
struct SBlocks { Block l[SAC_BLOCK_LAYERS]; int n, total; };
struct SRows { const float *obs, *ach, *des, *action; };

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

// the features as rows: a first layer's X (columns from D + 6 on are zeros)
MCG_DEV void store_features(float* chunk, int at, int fr, int D, const SRows& X, int row, int g, int i) {
  for (int f = g; f < fr; f += 4) {
    float x = 0.0f;
    if (f < 3) x = X.ach[(size_t)row * 3 + f];
    else if (f < 6) x = X.des[(size_t)row * 3 + (f - 3)];
    else if (f < D + 6) x = X.obs[(size_t)row * D + (f - 6)];
    chunk[(size_t)(at + f) * TILE + i] = x;
  }
}

// Critic `P` forward on one row with the action `act` in the accumulator layout, the inputs of the layers 1..n stored as rows (and the
// features and the action, where ROWS0) -> the head's tile (the value: row 0, on the lanes g == 0).
template <int MT, bool ROWS0>
MCG_DEV f4 critic_forward(const Pol& P, int qa, const GRows& R, float* chunk, const SRows& X, int row, const f4& act, int g, int i, int lane) {
  const Net& net = P.net[0];
  f4 a[MT], b[MT], head[1];
  first_layer<MT, float>(P, net, X.obs, X.ach, X.des, row, g, lane, a);
  const float* __restrict__ Wa = P.blob + qa;
#pragma unroll
  for (int t = 0; t < MT; t++) {
    if (t < net.nt[0]) {
#pragma unroll
      for (int r = 0; r < 4; r++) a[t] = mfma(Wa[(t * 4 + r) * WAVE + lane], act[r], a[t]);
    }
  }
  if (ROWS0) {
    store_features(chunk, R.x[0], R.fr, P.D, X, row, g, i);
#pragma unroll
    for (int r = 0; r < 4; r++) chunk[(size_t)(R.xa + 4 * g + r) * TILE + i] = act[r];
  }
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, a[t][r]);
  store_rows<MT>(chunk, R.x[1], net.nt[0], a, g, i);
  for (int L = 1; L < net.n; L++) {
    dense<MT, MT>(P, net, L, L == 1 ? net.nt[0] : net.nt[1], L == 1 ? net.nt[1] : net.nt[2], a, b, g, lane);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, b[t][r]);
    store_rows<MT>(chunk, L == 1 ? R.x[2] : R.x[3], L == 1 ? net.nt[1] : net.nt[2], a, g, i);
  }
  dense<MT, 1>(P, net, net.n, last_tiles(net), 1, a, head, g, lane);
  return head[0];
}

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

// ------------------------------------------------------------------------------------------------------- host side
inline void add_block(SBlocks& Q, int& blk, const Block& b) {
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

}  // namespace
