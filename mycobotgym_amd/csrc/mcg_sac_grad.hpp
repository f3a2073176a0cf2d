// mcg_sac_grad.hpp -- what of the gradient code takes a `Sac`, shared by the two off-policy gradient code objects, mcg_sac_grad.hip
// (SAC) and mcg_td3_grad.hip (TD3 / DDPG): the critic's forward with the action as an operand and its rows kept, the critic tile kernel
// (the head's scale is each family's), and on the host the two entries' layouts of `work`.  The row map, the block list, the forward
// with rows kept, the walk back, the dW kernel and the host's numbering and checks are mcg_grad.hpp's, shared with PPO.
// mcg_sac_grad.hip's head states the work split and the layout of `work`; each family's loss, actor tile kernel and reduce stay in
// its own file.
#pragma once

#include "mcg_grad.hpp"         // GRows, Blocks, sum16, store_rows, store_features, hidden_rows, walk_back, number_rows, number_inputs,
                                // layer_block, add_block, split_parts
#include "mcg_sac.hpp"          // Sac, load_action, last_tiles

namespace {

struct SRows { const float *obs, *ach, *des, *action; };

// Critic `P` forward on one row with the action `act` in the accumulator layout, the inputs of the layers 1..n stored as rows (and the
// features and the action, where ROWS0) -> the head's tile (the value: row 0, on the lanes g == 0).
template <int MT, bool ROWS0>
MCG_DEV f4 critic_forward(const Pol& P, int qa, const GRows& R, float* chunk, const SRows& X, int row, const f4& act, int g, int i, int lane) {
  const Net& net = P.net[0];
  f4 a[MT], head[1];
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
    store_features(chunk, R.x[0], R.fr, P.D, X.obs, X.ach, X.des, row, g, i);
#pragma unroll
    for (int r = 0; r < 4; r++) chunk[(size_t)(R.xa + 4 * g + r) * TILE + i] = act[r];
  }
  hidden_rows<MT>(P, net, R, chunk, true, a, g, i, lane);
  dense<MT, 1>(P, net, net.n, last_tiles(net), 1, a, head, g, lane);
  return head[0];
}

// The critic tile kernel of both families, one wave per (tile of 16 samples, critic): the forward with every layer's input kept as rows,
// the tile's sums, dq at the head -- (q - y) / B, or with TWICE (TD3's loss has no 0.5) 2 (q - y) / B, the doubling exact -- and the
// backward pass to every layer's dZ rows.  (A kernel and no device function under two kernels: handed on by reference, the kernel's
// arguments go through scratch.)
template <int MT, bool TWICE>
__global__ __launch_bounds__(WAVE) void critic_tile_kernel(Sac S, GRows R, SRows X, const float* __restrict__ y, int B, float inv_b, float* work) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int tile = blockIdx.x, s = tile * TILE + i;
  const bool live = s < B;
  const int row = live ? s : B - 1;
  const int k = blockIdx.y;
  const Pol& P = k ? S.qf[1] : S.qf[0];
  float* chunk = work + R.base + (size_t)k * R.stride + (size_t)tile * R.rows * TILE;
  const f4 act = load_action(P.A, X.action, row, g);
  const f4 h = critic_forward<MT, true>(P, S.qa, R, chunk, X, row, act, g, i, lane);
  const bool mine = live && g == 0;      // (lanes g == 0 hold the value: row 0 of the head)
  const float diff = h[0] - y[row];
  const float sq = sum16(mine ? diff * diff : 0.0f), qs = sum16(mine ? h[0] : 0.0f);
  if (lane == 0) { work[4 + 8 * (size_t)tile + k] = sq; work[4 + 8 * (size_t)tile + 2 + k] = qs; }
  f4 d[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (mine) d[0][0] = (TWICE ? __fmul_rn(2.0f, diff) : diff) * inv_b;
  const Net& net = P.net[0];
  store_rows<MT>(chunk, sel4(R.d, net.n), 1, d, g, i);
  walk_back<MT, true>(P, net, R, chunk, net.n, 0, d, g, i);
}

struct Layout { GRows a, q; Blocks blocks; int ntiles, tpp, parts; long long partials, need; };

// The critic entry's row map, block list and split of `work`, over n_critics critics.
inline Layout critic_layout(const Sac& S, int64_t B, int widest_qf, int64_t critic_floats, int n_critics) {
  Layout Y = {};
  Y.ntiles = (int)((B + TILE - 1) / TILE);
  split_parts(Y.ntiles, widest_qf, &Y.tpp, &Y.parts);
  const Net& net = S.qf[0].net[0];
  const int fr = (S.pi.D + 6 + 15) / 16 * 16;
  GRows& R = Y.q;
  R.rows = number_rows(R, net, fr, true);
  R.base = 4 + 8ll * Y.ntiles; R.stride = (long long)Y.ntiles * R.rows * TILE;
  Y.partials = R.base + n_critics * R.stride;
  Y.need = Y.partials + (long long)Y.parts * critic_floats;
  int blk = 0;
  const int one = (int)(critic_floats / n_critics);
  for (int k = 0; k < n_critics; k++)
    for (int L = 0; L <= net.n; L++) {
      Block b = layer_block(S.pi, net, R, L);
      b.w += k * one; b.b += k * one; b.base += k * R.stride;
      add_block(Y.blocks, blk, b);
      if (L == 0) {                      // the action tiles: 16 columns in the later-layer order, no bias of their own
        Block a = b;
        a.ncb = 1; a.nb = 0; a.xrow = R.xa; a.w = S.qa + k * one; a.nkb = 4; a.first = 0; a.cols = S.pi.A;
        add_block(Y.blocks, blk, a);
      }
    }
  Y.blocks.total = blk;
  return Y;
}

// The actor entry's: the actor's rows and blocks (log_std_head: SAC's second head, its dZ rows d2 and its block); of each of the
// n_q_rows critics the entry runs (SAC: both; TD3: qf0) only the activation rows (no dZ is kept: no critic dW is formed).
inline Layout actor_layout(const Sac& S, int64_t B, int widest_pi, int64_t actor_floats, bool log_std_head, int n_q_rows) {
  Layout Y = {};
  Y.ntiles = (int)((B + TILE - 1) / TILE);
  split_parts(Y.ntiles, widest_pi, &Y.tpp, &Y.parts);
  const Net& net = S.pi.net[1];
  const Net& ls = S.pi.net[0];
  const int fr = (S.pi.D + 6 + 15) / 16 * 16, n = net.n;
  GRows& R = Y.a;
  R.rows = number_rows(R, net, fr, false);
  if (log_std_head) { R.d2 = R.rows; R.rows += 16; }
  R.base = 4 + 8ll * Y.ntiles; R.stride = 0;
  const Net& qnet = S.qf[0].net[0];
  GRows& Q = Y.q;
  Q.rows = number_inputs(Q, qnet, 0);
  Q.base = R.base + (long long)Y.ntiles * R.rows * TILE; Q.stride = (long long)Y.ntiles * Q.rows * TILE;
  Y.partials = Q.base + n_q_rows * Q.stride;
  Y.need = Y.partials + (long long)Y.parts * actor_floats;
  int blk = 0;
  for (int L = 0; L <= n; L++) add_block(Y.blocks, blk, layer_block(S.pi, net, R, L));       // the trunk and the head mu
  if (log_std_head) {                    // the head log_std: the head's input again, its own dZ rows, weights and bias
    Block b = layer_block(S.pi, net, R, n);
    b.drow = R.d2; b.w = ls.w[n]; b.b = ls.b[n];
    add_block(Y.blocks, blk, b);
  }
  Y.blocks.total = blk;
  return Y;
}

}  // namespace
