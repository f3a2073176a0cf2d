// mcg_td3_grad.hip -- TD3's and DDPG's update (include/mcg.h: mcg_td3_critic_grad, mcg_td3_actor_grad; Adam is mcg_sac_adam): the
// critic loss's gradient over the critic blob and the deterministic actor loss's gradient over the actor blob through qf0 as a
// constant.  A code object of its own, as mcg_td3.hip, whose plan and host checks it shares (mcg_td3.hpp); the critic's forward with
// its rows, the walk back, the row map and the block list are mcg_sac_grad.hpp's, the dW block and the sum in part order
// mcg_grad.hpp's (mcg_sac_grad.hip's and mcg_policy_grad.hip's heads state the work split).  Float32 throughout on
// v_mfma_f32_16x16x4_f32; deterministic: no atomics, every sum in an order that the shape and B alone fix.
//
// ---- The critic tile kernel: one wave per (tile of 16 samples, critic), as sac_critic_tile_kernel, with the loss
// sum_k mean((q_k - y)^2): dq = 2 (q - y) / B at the head, the doubling exact.
//
// ---- The actor tile kernel: one wave per tile.  The actor forward with its rows kept; tanh of the head; qf0 on the action in its
// registers with its activation rows kept; the walk back from dq = 1 down to the 16 action columns (dX only: no critic dW is
// formed); the head's dZ = -dQ/da (1 - a^2) / B, in double from the float32 values, rounded once; the walk back through the actor.
//
// ---- `work` (floats): [0..3] unused; [4 + 8 tile + s] the tile's sums (critic entry: s = k the squared errors of critic k, s = 2 + k
// its q sum; actor entry: s = 0 the q sum); then the row chunks per net and tile; then `parts` partial blobs.  Every float that is read
// was written by the same call.  A ragged last tile's extra lanes read the last valid sample and get dZ = +-0 at the head.
#include "mcg_sac_grad.hpp"     // GRows, SBlocks, SRows, critic_forward, walk_back, wt_acc, add_block, checked_buffer; mcg_grad.hpp
#include "mcg_td3.hpp"          // td3_plan, checked_td3, tanh_head

using namespace mcg;

namespace {

struct ActorOut { float *action, *q_pi, *dq_da; };

template <int MT>
__global__ __launch_bounds__(WAVE) void td3_critic_tile_kernel(Sac S, GRows R, SRows X, const float* __restrict__ y, int B, float inv_b,
                                                               float* work) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int tile = blockIdx.x, s = tile * TILE + i;
  const bool live = s < B;
  const int row = live ? s : B - 1;
  const int k = blockIdx.y;
  const Pol& P = k ? S.qf[1] : S.qf[0];
  float* chunk = work + R.base + (size_t)k * R.stride + (size_t)tile * R.rows * TILE;
  f4 act;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    act[r] = 0.0f;
    if (c < P.A) act[r] = X.action[(size_t)row * P.A + c];
  }
  const f4 h = critic_forward<MT, true>(P, S.qa, R, chunk, X, row, act, g, i, lane);
  const bool mine = live && g == 0;      // (lanes g == 0 hold the value: row 0 of the head)
  const float diff = h[0] - y[row];
  const float sq = sum16(mine ? diff * diff : 0.0f), qs = sum16(mine ? h[0] : 0.0f);
  if (lane == 0) { work[4 + 8 * (size_t)tile + k] = sq; work[4 + 8 * (size_t)tile + 2 + k] = qs; }
  f4 d[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (mine) d[0][0] = __fmul_rn(2.0f, diff) * inv_b;
  const Net& net = P.net[0];
  store_rows<MT>(chunk, sel4(R.d, net.n), 1, d, g, i);
  walk_back<MT, true>(P, net, R, chunk, net.n, 0, d, g, i);
}

template <int MT>
__global__ __launch_bounds__(WAVE) void td3_actor_tile_kernel(Sac S, GRows RA, GRows RQ, SRows X, int B, double inv_b, float* work, ActorOut O) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int tile = blockIdx.x, s = tile * TILE + i;
  const bool live = s < B;
  const int row = live ? s : B - 1;
  const Pol& PA = S.pi;
  const Net& net = PA.net[1];
  const int n = net.n;
  float* chunk = work + RA.base + (size_t)tile * RA.rows * TILE;
  // ---- the actor, as mcg_td3.hip's td3_actor(), with its rows kept
  f4 z[1];
  {
    f4 a[MT], b[MT];
    first_layer<MT, float>(PA, net, X.obs, X.ach, X.des, row, g, lane, a);
    store_features(chunk, RA.x[0], RA.fr, PA.D, X, row, g, i);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) a[t][r] = activate(PA.act, a[t][r]);
    store_rows<MT>(chunk, RA.x[1], net.nt[0], a, g, i);
    for (int L = 1; L < n; L++) {
      dense<MT, MT>(PA, net, L, L == 1 ? net.nt[0] : net.nt[1], L == 1 ? net.nt[1] : net.nt[2], a, b, g, lane);
#pragma unroll
      for (int t = 0; t < MT; t++)
#pragma unroll
        for (int r = 0; r < 4; r++) a[t][r] = activate(PA.act, b[t][r]);
      store_rows<MT>(chunk, L == 1 ? RA.x[2] : RA.x[3], L == 1 ? net.nt[1] : net.nt[2], a, g, i);
    }
    dense<MT, 1>(PA, net, n, last_tiles(net), 1, a, z, g, lane);
  }
  const f4 act = tanh_head(PA.A, z[0], g);
  // ---- qf0 on the action where it lies, and its dQ/da
  const Pol& PQ = S.qf[0];
  const Net& qnet = PQ.net[0];
  float* qchunk = work + RQ.base + (size_t)tile * RQ.rows * TILE;
  const f4 h = critic_forward<MT, false>(PQ, S.qa, RQ, qchunk, X, row, act, g, i, lane);
  const bool mine = live && g == 0;
  f4 d[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (mine) d[0][0] = 1.0f;
  walk_back<MT, false>(PQ, qnet, RQ, qchunk, qnet.n, 0, d, g, i);
  const f4 dqda = wt_acc<MT>(PQ.blob + S.qa, 4, 0, qnet.nt[0], d, f4{0.0f, 0.0f, 0.0f, 0.0f}, g, i);
  // ---- the head's derivative (include/mcg.h), and the outputs
  f4 dz = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int comp = 4 * g + r;
    if (live && comp < PA.A) {
      const double a = (double)act[r];
      dz[r] = (float)(-(double)dqda[r] * (1.0 - a * a) * inv_b);
      const size_t at = (size_t)s * PA.A + comp;
      if (O.action) O.action[at] = act[r];
      if (O.dq_da) O.dq_da[at] = dqda[r];
    }
  }
  if (mine && O.q_pi) O.q_pi[s] = h[0];
  const float qsum = sum16(mine ? h[0] : 0.0f);
  if (lane == 0) work[4 + 8 * (size_t)tile] = qsum;
  // ---- the actor's backward pass
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  d[0] = dz;
  store_rows<MT>(chunk, sel4(RA.d, n), 1, d, g, i);
  walk_back<MT, true>(PA, net, RA, chunk, n, 0, d, g, i);
}

// One 16 x 16 block of dW (or 16 biases) over the tiles of one part -> its place in the part's partial blob.
__global__ __launch_bounds__(WAVE) void td3_dw_kernel(SBlocks Q, const float* __restrict__ work, float* __restrict__ partials, long long blob_floats,
                                                      int ntiles, int tpp) {
  const int blk = blockIdx.x, part = blockIdx.y;
  Block me = Q.l[0];
#pragma unroll
  for (int q = 1; q < SAC_BLOCK_LAYERS; q++)
    if (q < Q.n && blk >= Q.l[q].blk0) me = Q.l[q];              // (constant indices: selects, no scratch)
  dw_block(me, blk, part, work, partials, blob_floats, ntiles, tpp);
}

// grad[p] = the partial blobs' sum in part order; the last block: the tiles' sums -> stats (include/mcg.h names the slots).
__global__ __launch_bounds__(256) void td3_reduce_kernel(const float* __restrict__ work, const float* __restrict__ partials, int parts,
                                                         long long blob_floats, int ntiles, int actor, int n_critics, float inv_b,
                                                         float* __restrict__ grad, float* __restrict__ stats) {
  if (blockIdx.x < gridDim.x - 1) {
    const long long p = (long long)blockIdx.x * 256 + threadIdx.x;
    if (p < blob_floats) grad[p] = sum_parts(partials, parts, blob_floats, p);
    return;
  }
  if (threadIdx.x >= WAVE) return;
  const bool two = !actor && n_critics == 2;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = threadIdx.x; t < ntiles; t += WAVE) {
    const float* w = work + 4 + 8 * (size_t)t;
    acc[0] += w[0];
    if (!actor) acc[2] += w[2];
    if (two) { acc[1] += w[1]; acc[3] += w[3]; }
  }
#pragma unroll
  for (int j = 0; j < 4; j++)
    for (int m = 32; m >= 1; m >>= 1) acc[j] += __shfl_xor(acc[j], m);
  if (threadIdx.x != 0) return;
  if (actor) {
    const float mean = acc[0] * inv_b;
    stats[1] = -mean; stats[4] = mean;
  } else {
    stats[0] = two ? acc[0] * inv_b + acc[1] * inv_b : acc[0] * inv_b;
    stats[2] = acc[2] * inv_b; stats[3] = two ? acc[3] * inv_b : 0.0f;
    stats[5] = stats[6] = stats[7] = 0.0f;
  }
}

// ------------------------------------------------------------------------------------------------------- host side
struct Layout { GRows a, q; SBlocks blocks; int ntiles, tpp, parts; long long partials, need; };

// The critic entry's row map, block list and split of `work`: sac_grad's, over n_critics critics.
Layout critic_layout(const Sac& S, int64_t B, int widest_qf, int64_t critic_floats, int n_critics) {
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

// The actor entry's: the actor's rows and blocks; of qf0 only the activation rows (no dZ is kept: no critic dW is formed).
Layout actor_layout(const Sac& S, int64_t B, int widest_pi, int64_t actor_floats) {
  Layout Y = {};
  Y.ntiles = (int)((B + TILE - 1) / TILE);
  split_parts(Y.ntiles, widest_pi, &Y.tpp, &Y.parts);
  const Net& net = S.pi.net[1];
  const int fr = (S.pi.D + 6 + 15) / 16 * 16, n = net.n;
  GRows& R = Y.a;
  int row = 0;
  R.fr = fr; R.x[0] = 0; row += fr;
  for (int L = 0; L < n; L++) { R.x[L + 1] = row; row += 16 * net.nt[L]; }
  for (int L = 0; L <= n; L++) { R.d[L] = row; row += L < n ? 16 * net.nt[L] : 16; }
  R.rows = row; R.base = 4 + 8ll * Y.ntiles; R.stride = 0;
  const Net& qnet = S.qf[0].net[0];
  GRows& Q = Y.q;
  row = 0;
  for (int L = 0; L < qnet.n; L++) { Q.x[L + 1] = row; row += 16 * qnet.nt[L]; }
  Q.rows = row; Q.base = R.base + (long long)Y.ntiles * R.rows * TILE; Q.stride = 0;
  Y.partials = Q.base + (long long)Y.ntiles * Q.rows * TILE;
  Y.need = Y.partials + (long long)Y.parts * actor_floats;
  int blk = 0;
  for (int L = 0; L <= n; L++) {         // the trunk, the head
    Block b = {};
    b.nT = L < n ? net.nt[L] : 1; b.ncb = L == 0 ? fr / 16 : net.nt[L - 1]; b.nb = 1;
    b.xrow = R.x[L]; b.drow = R.d[L]; b.w = net.w[L]; b.b = net.b[L];
    b.nkb = L == 0 ? S.pi.kb0 : 4 * net.nt[L - 1]; b.first = L == 0; b.cols = L == 0 ? S.pi.D + 6 : ALL_COLUMNS;
    b.rows = R.rows; b.base = R.base;
    add_block(Y.blocks, blk, b);
  }
  Y.blocks.total = blk;
  return Y;
}

bool checked_work(const char* who, const float* work, int64_t work_floats, long long need) {
  if (!checked_buffer(who, work, "work")) return false;
  if (work_floats < need) {
    mcg_fail(MCG_ERR_ARG, "%s: work_floats is %lld, this entry needs %lld for this shape and B (mcg_td3_grad_work_floats covers both)", who,
             (long long)work_floats, need);
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

int64_t mcg_td3_grad_work_floats(const mcg_td3* td3, int64_t B) {
  Sac S = {};
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (!td3 || B < 1 || B * MAX_ACT >= (1ll << 31)) return 0;
  if (td3_plan(td3->obs_dim, td3->act_dim, td3->n_pi, td3->pi_width, td3->n_qf, td3->qf_width, td3->n_critics, &S, &actor, &critic, &why) == 0)
    return 0;
  const long long c = critic_layout(S, B, td3_widest(td3, false, true), critic, td3->n_critics).need;
  const long long a = actor_layout(S, B, td3_widest(td3, true, false), actor).need;
  return c > a ? c : a;
}

int mcg_td3_critic_grad(const mcg_td3* td3, const mcg_sac_rows* rows, const float* y, int64_t B, float* work, int64_t work_floats,
                        float* grad, float* stats, void* stream) {
  const char* who = "mcg_td3_critic_grad";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_CRITIC, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B)) return MCG_ERR_ARG;
  if (!rows) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac_rows", who);
  if (!rows->obs || !rows->achieved || !rows->desired || !rows->action)
    return mcg_fail(MCG_ERR_ARG, "%s: obs, achieved, desired and action of the rows are required", who);
  if (!y) return mcg_fail(MCG_ERR_ARG, "%s: y is null", who);
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const int wq = td3_widest(td3, false, true);
  const Layout Y = critic_layout(S, B, wq, td3->critic_floats, td3->n_critics);
  if (!checked_work(who, work, work_floats, Y.need)) return MCG_ERR_ARG;
  set_critics(S, td3, td3->critic);
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, rows->action};
  const float inv_b = (float)(1.0 / (double)B);
  const dim3 grid(Y.ntiles, td3->n_critics), block(WAVE);
  if (wq <= 64) hipLaunchKernelGGL(td3_critic_tile_kernel<4>, grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  else hipLaunchKernelGGL(td3_critic_tile_kernel<16>, grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  hipLaunchKernelGGL(td3_dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)td3->critic_floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(td3_reduce_kernel, dim3(blocks(td3->critic_floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)td3->critic_floats, Y.ntiles, 0, (int)td3->n_critics, inv_b, grad, stats);
  return launched(who);
}

int mcg_td3_actor_grad(const mcg_td3* td3, const mcg_sac_rows* rows, int64_t B, float* work, int64_t work_floats, float* grad, float* stats,
                       const mcg_td3_actor_grad_out* out, void* stream) {
  const char* who = "mcg_td3_actor_grad";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_ACTOR | TD3_CRITIC, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B)) return MCG_ERR_ARG;
  if (!rows) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac_rows", who);
  if (!rows->obs || !rows->achieved || !rows->desired) return mcg_fail(MCG_ERR_ARG, "%s: obs, achieved and desired of the rows are required", who);
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const Layout Y = actor_layout(S, B, td3_widest(td3, true, false), td3->actor_floats);
  if (!checked_work(who, work, work_floats, Y.need)) return MCG_ERR_ARG;
  S.pi.blob = td3->actor;
  set_critics(S, td3, td3->critic);
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, nullptr};
  ActorOut O = {nullptr, nullptr, nullptr};
  if (out) { O.action = out->action; O.q_pi = out->q_pi; O.dq_da = out->dq_da; }
  const double inv_b = 1.0 / (double)B;
  const dim3 grid(Y.ntiles), block(WAVE);
  if (td3_widest(td3, true, true) <= 64) hipLaunchKernelGGL(td3_actor_tile_kernel<4>, grid, block, 0, st, S, Y.a, Y.q, X, (int)B, inv_b, work, O);
  else hipLaunchKernelGGL(td3_actor_tile_kernel<16>, grid, block, 0, st, S, Y.a, Y.q, X, (int)B, inv_b, work, O);
  hipLaunchKernelGGL(td3_dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)td3->actor_floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(td3_reduce_kernel, dim3(blocks(td3->actor_floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)td3->actor_floats, Y.ntiles, 1, (int)td3->n_critics, (float)inv_b, grad,
                     stats);
  return launched(who);
}

}  // extern "C"
