// mcg_td3_grad.hip -- TD3's and DDPG's update (include/mcg.h: mcg_td3_critic_grad, mcg_td3_actor_grad; Adam is mcg_sac_adam): the
// critic loss's gradient over the critic blob and the deterministic actor loss's gradient over the actor blob through qf0 as a
// constant.  A code object of its own, as mcg_td3.hip, whose host checks it shares (mcg_td3.hpp); the critic's forward, the critic
// tile kernel and both entries' layouts of `work` are mcg_sac_grad.hpp's single definitions; the row map, the block list, the forward
// with its rows kept, the walk back, the dW kernel and the reduce's helpers are mcg_grad.hpp's, shared with PPO as well
// (mcg_sac_grad.hip's and mcg_policy_grad.hip's heads state the work split).  Here: TD3's actor tile kernel and its reduce's
// statistics.  Float32 throughout on
// v_mfma_f32_16x16x4_f32; deterministic: no atomics, every sum in an order that the shape and B alone fix.
//
// ---- The critic tile kernel: critic_tile_kernel<MT, true> (mcg_sac_grad.hpp), one wave per (tile of 16 samples, critic), with the
// loss sum_k mean((q_k - y)^2): dq = 2 (q - y) / B at the head, the doubling exact.
//
// ---- The actor tile kernel: one wave per tile.  The actor forward with its rows kept; tanh of the head; qf0 on the action in its
// registers with its activation rows kept; the walk back from dq = 1 down to the 16 action columns (dX only: no critic dW is
// formed); the head's dZ = -dQ/da (1 - a^2) / B, in double from the float32 values, rounded once; the walk back through the actor.
//
// ---- `work` (floats): [0..3] unused; [4 + 8 tile + s] the tile's sums (critic entry: s = k the squared errors of critic k, s = 2 + k
// its q sum; actor entry: s = 0 the q sum); then the row chunks per net and tile; then `parts` partial blobs.  Every float that is read
// was written by the same call.  A ragged last tile's extra lanes read the last valid sample and get dZ = +-0 at the head.
#include "mcg_sac_grad.hpp"     // SRows, critic_forward, critic_tile_kernel, Layout, critic_layout, actor_layout; mcg_grad.hpp: GRows,
                                // store_features, hidden_rows, walk_back, wt_acc, dw_kernel, reduced_parts, sum64, checked_buffer, checked_work
#include "mcg_td3.hpp"          // checked_td3, set_critics, tanh_head

using namespace mcg;

namespace {

struct ActorOut { float *action, *q_pi, *dq_da; };

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
  // ---- the actor, as mcg_td3.hpp's td3_actor(), with its rows kept
  f4 z[1];
  {
    f4 a[MT];
    first_layer<MT, float>(PA, net, X.obs, X.ach, X.des, row, g, lane, a);
    store_features(chunk, RA.x[0], RA.fr, PA.D, X.obs, X.ach, X.des, row, g, i);
    hidden_rows<MT>(PA, net, RA, chunk, true, a, g, i, lane);
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

// grad[p] = the partial blobs' sum in part order; the last block: the tiles' sums -> stats (include/mcg.h names the slots).
__global__ __launch_bounds__(256) void td3_reduce_kernel(const float* __restrict__ work, const float* __restrict__ partials, int parts,
                                                         long long blob_floats, int ntiles, int actor, int n_critics, float inv_b,
                                                         float* __restrict__ grad, float* __restrict__ stats) {
  if (reduced_parts(partials, parts, blob_floats, grad) || threadIdx.x >= WAVE) return;
  const bool two = !actor && n_critics == 2;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = threadIdx.x; t < ntiles; t += WAVE) {
    const float* w = work + 4 + 8 * (size_t)t;
    acc[0] += w[0];
    if (!actor) acc[2] += w[2];
    if (two) { acc[1] += w[1]; acc[3] += w[3]; }
  }
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = sum64(acc[j]);
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

}  // namespace

extern "C" {

int64_t mcg_td3_grad_work_floats(const mcg_td3* td3, int64_t B) {
  Sac S = {};
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (!td3 || !rows_in_range(B)) return 0;
  if (blob_plan(td3->obs_dim, td3->act_dim, td3->n_pi, td3->pi_width, td3->n_qf, td3->qf_width, td3->n_critics, false, &S, &actor, &critic,
                &why) == 0)
    return 0;
  const long long c = critic_layout(S, B, widest(td3, false, true), critic, td3->n_critics).need;
  const long long a = actor_layout(S, B, widest(td3, true, false), actor, false, 1).need;
  return c > a ? c : a;
}

int mcg_td3_critic_grad(const mcg_td3* td3, const mcg_sac_rows* rows, const float* y, int64_t B, float* work, int64_t work_floats,
                        float* grad, float* stats, void* stream) {
  const char* who = "mcg_td3_critic_grad";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_CRITIC, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, true)) return MCG_ERR_ARG;
  if (!y) return mcg_fail(MCG_ERR_ARG, "%s: y is null", who);
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const int wq = widest(td3, false, true);
  const Layout Y = critic_layout(S, B, wq, td3->critic_floats, td3->n_critics);
  if (!checked_work(who, work, work_floats, Y.need, "mcg_td3_grad_work_floats")) return MCG_ERR_ARG;
  set_critics(S, td3, td3->critic);
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, rows->action};
  const float inv_b = (float)(1.0 / (double)B);
  const dim3 grid(Y.ntiles, td3->n_critics), block(WAVE);
  if (wq <= 64) hipLaunchKernelGGL((critic_tile_kernel<4, true>), grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  else hipLaunchKernelGGL((critic_tile_kernel<16, true>), grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  hipLaunchKernelGGL(dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
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
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, false)) return MCG_ERR_ARG;
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const Layout Y = actor_layout(S, B, widest(td3, true, false), td3->actor_floats, false, 1);
  if (!checked_work(who, work, work_floats, Y.need, "mcg_td3_grad_work_floats")) return MCG_ERR_ARG;
  S.pi.blob = td3->actor;
  set_critics(S, td3, td3->critic);
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, nullptr};
  ActorOut O = {nullptr, nullptr, nullptr};
  if (out) { O.action = out->action; O.q_pi = out->q_pi; O.dq_da = out->dq_da; }
  const double inv_b = 1.0 / (double)B;
  const dim3 grid(Y.ntiles), block(WAVE);
  if (widest(td3, true, true) <= 64) hipLaunchKernelGGL(td3_actor_tile_kernel<4>, grid, block, 0, st, S, Y.a, Y.q, X, (int)B, inv_b, work, O);
  else hipLaunchKernelGGL(td3_actor_tile_kernel<16>, grid, block, 0, st, S, Y.a, Y.q, X, (int)B, inv_b, work, O);
  hipLaunchKernelGGL(dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)td3->actor_floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(td3_reduce_kernel, dim3(blocks(td3->actor_floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)td3->actor_floats, Y.ntiles, 1, (int)td3->n_critics, (float)inv_b, grad,
                     stats);
  return launched(who);
}

}  // extern "C"
