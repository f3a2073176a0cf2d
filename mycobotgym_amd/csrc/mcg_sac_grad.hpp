// mcg_sac_grad.hpp -- what the two off-policy gradient code objects share, mcg_sac_grad.hip (SAC) and mcg_td3_grad.hip (TD3 / DDPG):
// a net's row map of a tile in `work`, the hidden layers' forward with their rows kept, the critic's forward with the action as an
// operand, the walk back through a net, the critic tile kernel (the head's scale is each family's), the dW kernel and its block
// list, and on the host the two entries' layouts of `work` and its check.  mcg_sac_grad.hip's head states the work split and the
// layout of `work`; each family's loss, actor tile kernel and reduce stay in its own file.
#pragma once

#include "mcg_grad.hpp"         // sum16, store_rows, Block, dw_block, sum_parts, block_sum, adam_one
#include "mcg_sac.hpp"          // Sac, Draw, squash, load_action, blob_plan, checked_sac

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
    store_features(chunk, R.x[0], R.fr, P.D, X, row, g, i);
#pragma unroll
    for (int r = 0; r < 4; r++) chunk[(size_t)(R.xa + 4 * g + r) * TILE + i] = act[r];
  }
  hidden_rows<MT>(P, net, R, chunk, true, a, g, i, lane);
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

// One 16 x 16 block of dW (or 16 biases) over the tiles of one part -> its place in the part's partial blob.
__global__ __launch_bounds__(WAVE) void dw_kernel(SBlocks Q, const float* __restrict__ work, float* __restrict__ partials, long long blob_floats,
                                                  int ntiles, int tpp) {
  const int blk = blockIdx.x, part = blockIdx.y;
  Block me = Q.l[0];
#pragma unroll
  for (int q = 1; q < SAC_BLOCK_LAYERS; q++)
    if (q < Q.n && blk >= Q.l[q].blk0) me = Q.l[q];              // (constant indices: selects, no scratch)
  dw_block(me, blk, part, work, partials, blob_floats, ntiles, tpp);
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

struct Layout { GRows a, q; SBlocks blocks; int ntiles, tpp, parts; long long partials, need; };

// The critic entry's row map, block list and split of `work`, over n_critics critics.
inline Layout critic_layout(const Sac& S, int64_t B, int widest_qf, int64_t critic_floats, int n_critics) {
  Layout Y = {};
  Y.ntiles = (int)((B + TILE - 1) / TILE);
  split_parts(Y.ntiles, widest_qf, &Y.tpp, &Y.parts);
  const Net& net = S.qf[0].net[0];
  const int fr = (S.pi.D + 6 + 15) / 16 * 16;
  GRows& R = Y.q;
  int row = 0;
  R.fr = fr; R.x[0] = 0; row += fr;
  R.xa = row; row += 16;
  for (int L = 0; L < net.n; L++) { R.x[L + 1] = row; row += 16 * net.nt[L]; }
  for (int L = 0; L <= net.n; L++) { R.d[L] = row; row += L < net.n ? 16 * net.nt[L] : 16; }
  R.rows = row; R.base = 4 + 8ll * Y.ntiles; R.stride = (long long)Y.ntiles * row * TILE;
  Y.partials = R.base + n_critics * R.stride;
  Y.need = Y.partials + (long long)Y.parts * critic_floats;
  int blk = 0;
  const int one = (int)(critic_floats / n_critics);
  for (int k = 0; k < n_critics; k++)
    for (int L = 0; L <= net.n; L++) {
      Block b = {};
      b.nT = L < net.n ? net.nt[L] : 1; b.ncb = L == 0 ? fr / 16 : net.nt[L - 1]; b.nb = 1;
      b.xrow = R.x[L]; b.drow = R.d[L]; b.w = net.w[L] + k * one; b.b = net.b[L] + k * one;
      b.nkb = L == 0 ? S.pi.kb0 : 4 * net.nt[L - 1]; b.first = L == 0; b.cols = L == 0 ? S.pi.D + 6 : ALL_COLUMNS;
      b.rows = R.rows; b.base = R.base + k * R.stride;
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
  int row = 0;
  R.fr = fr; R.x[0] = 0; row += fr;
  for (int L = 0; L < n; L++) { R.x[L + 1] = row; row += 16 * net.nt[L]; }
  for (int L = 0; L <= n; L++) { R.d[L] = row; row += L < n ? 16 * net.nt[L] : 16; }
  if (log_std_head) { R.d2 = row; row += 16; }
  R.rows = row; R.base = 4 + 8ll * Y.ntiles; R.stride = 0;
  const Net& qnet = S.qf[0].net[0];
  GRows& Q = Y.q;
  row = 0;
  for (int L = 0; L < qnet.n; L++) { Q.x[L + 1] = row; row += 16 * qnet.nt[L]; }
  Q.rows = row; Q.base = R.base + (long long)Y.ntiles * R.rows * TILE; Q.stride = (long long)Y.ntiles * row * TILE;
  Y.partials = Q.base + n_q_rows * Q.stride;
  Y.need = Y.partials + (long long)Y.parts * actor_floats;
  int blk = 0;
  for (int L = 0; L <= n + (log_std_head ? 1 : 0); L++) {        // the trunk, the head mu, the head log_std
    const Net& from = L <= n ? net : ls;
    const int M = L <= n ? L : n;
    Block b = {};
    b.nT = M < n ? net.nt[M] : 1; b.ncb = M == 0 ? fr / 16 : net.nt[M - 1]; b.nb = 1;
    b.xrow = R.x[M]; b.drow = L <= n ? R.d[M] : R.d2; b.w = from.w[M]; b.b = from.b[M];
    b.nkb = M == 0 ? S.pi.kb0 : 4 * net.nt[M - 1]; b.first = M == 0; b.cols = M == 0 ? S.pi.D + 6 : ALL_COLUMNS;
    b.rows = R.rows; b.base = R.base;
    add_block(Y.blocks, blk, b);
  }
  Y.blocks.total = blk;
  return Y;
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

}  // namespace
