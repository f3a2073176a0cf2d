// mcg_sac_grad.hip -- SAC's update (include/mcg.h: mcg_sac_critic_grad, mcg_sac_actor_grad, mcg_sac_alpha_step, mcg_sac_adam): the
// critic loss's gradient over the critic blob, the actor loss's gradient over the actor blob through the twin critics as constants,
// the entropy coefficient's step, and Adam on a bare blob.  A code object of its own, as mcg_sac.hip, whose plan, actor draw and host
// checks it shares (mcg_sac.hpp); the critic's forward, the critic tile kernel and both entries' layouts of `work` are
// mcg_sac_grad.hpp's, shared with TD3 / DDPG (mcg_td3_grad.hip); the row map, the forward with rows kept, the walk back, the dW kernel,
// the reduce's helpers and Adam's kernel are mcg_grad.hpp's, shared with PPO as well; the three products of a layer and the work split
// (a tile kernel, a dW kernel per block and part, a reduce in part order) are stated at mcg_policy_grad.hip's head.  Here: SAC's actor
// tile kernel, its reduce's statistics, the alpha step and Adam's entry.
// Float32 throughout on v_mfma_f32_16x16x4_f32; deterministic: no atomics, every sum in an order that the shape and B alone fix.
//
// ---- The critic tile kernel (critic_tile_kernel<MT, false>, mcg_sac_grad.hpp): one wave per (tile of 16 samples, critic).  The forward on (features, action) with mcg_sac.hip's
// action-as-operand layout, every layer's input kept as rows in `work` (the features, the action padded to 16 rows, the activations);
// dq = (q - y) / B at the head; the backward pass to every layer's dZ rows.  The first layer's dW has two column groups, the feature
// tiles (first-layer order) and the action tile (later-layer order, 4 k-blocks): two entries of the block list, the second without a
// bias, each landing where the blob keeps it.
//
// ---- The actor tile kernel: one workgroup of two waves per tile, as sac_target_kernel.  Both waves run the actor on the tile -- the
// same instructions on the same inputs as mcg_sac_act and mcg_sac_target, so the same bits -- and wave 0 keeps its rows.  Wave q runs
// critic q on the action in its registers and keeps that critic's activation rows; the two Q rows meet through LDS; each sample picks
// c = (q1 < q0); wave q walks back through critic q from dq = [c == q] down to the 16 action columns (dX only: no critic dW is
// formed); the two dQ/da meet through LDS -- one of them is exactly zero per sample, so their sum has no order.  Wave 0 forms the head's
// derivative (include/mcg.h states it; in double from the float32 values, rounded once) and walks back through the actor: the two
// heads mu and log_std share the last hidden layer, whose dZ is act' (W_mu^T dmu + W_ls^T dls), the mu product first.
//
// ---- `work` (floats): [0..3] unused; [4 + 8 tile + s] the tile's sums (critic entry: s = 0, 1 the squared errors of qf0, qf1, s = 2, 3
// their q sums; actor entry: s = 0 the loss terms, 1 the log-probs); then the row chunks (struct GRows) per net and tile; then `parts`
// partial blobs.  Every float that is read was written by the same call.  A ragged last tile's extra lanes read the last valid sample
// and get dZ = +-0 at the head, so that every product they enter adds exactly nothing.
#include "mcg_sac_grad.hpp"     // SRows, critic_forward, critic_tile_kernel, Layout, critic_layout, actor_layout (shared with
                                // mcg_td3_grad.hip); mcg_sac.hpp; mcg_grad.hpp: GRows, store_features, hidden_rows, walk_back, wt_acc,
                                // act_prime, dw_kernel, reduced_parts, sum64, block_sum, adam_one, adam_kernel, adam_step, checked_buffer,
                                // checked_work

using namespace mcg;

namespace {

struct ActorOut { float *action, *noise, *q_pi, *dq_da, *logp; };

template <int MT>
__global__ __launch_bounds__(2 * WAVE) void sac_actor_tile_kernel(Sac S, GRows RA, GRows RQ, SRows X, int B, unsigned long long seed,
                                                                  unsigned long long call, float ent_coef,
                                                                  const float* __restrict__ log_ent_coef, double inv_b, float* work, ActorOut O) {
  __shared__ float qs[2][TILE];
  __shared__ float da[2][TILE][TILE];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int tile = blockIdx.x, s = tile * TILE + i;
  const bool live = s < B;
  const int row = live ? s : B - 1;
  const Pol& PA = S.pi;
  const Net& net = PA.net[1];
  const int n = net.n;
  float* chunk = work + RA.base + (size_t)tile * RA.rows * TILE;
  // ---- the actor, as mcg_sac.hip's actor() with hidden_rows for hidden(): both waves; wave 0 keeps the rows
  f4 mu[1], ls[1];
  {
    f4 a[MT];
    first_layer<MT, float>(PA, net, X.obs, X.ach, X.des, row, g, lane, a);
    if (wave == 0) store_features(chunk, RA.x[0], RA.fr, PA.D, X.obs, X.ach, X.des, row, g, i);
    hidden_rows<MT>(PA, net, RA, chunk, wave == 0, a, g, i, lane);
    dense<MT, 1>(PA, PA.net[1], n, last_tiles(net), 1, a, mu, g, lane);
    dense<MT, 1>(PA, PA.net[0], n, last_tiles(net), 1, a, ls, g, lane);
  }
  const Draw dr = squash(PA.A, mu[0], ls[0], g, seed, (unsigned long long)row, call, DOMAIN_SAC_ACTOR_LOSS, false);
  // ---- critic `wave` on the action where it lies; the min's choice; dQ/da of the chosen critic
  const Pol& PQ = wave ? S.qf[1] : S.qf[0];
  const Net& qnet = PQ.net[0];
  float* qchunk = work + RQ.base + (size_t)wave * RQ.stride + (size_t)tile * RQ.rows * TILE;
  const f4 h = critic_forward<MT, false>(PQ, S.qa, RQ, qchunk, X, row, dr.action, g, i, lane);
  if (g == 0) qs[wave][i] = h[0];
  __syncthreads();
  const float q0 = qs[0][i], q1 = qs[1][i];
  const int c = q1 < q0 ? 1 : 0;
  f4 d[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (live && g == 0 && c == wave) d[0][0] = 1.0f;
  walk_back<MT, false>(PQ, qnet, RQ, qchunk, qnet.n, 0, d, g, i);
  {
    const f4 dav = wt_acc<MT>(PQ.blob + S.qa, 4, 0, qnet.nt[0], d, f4{0.0f, 0.0f, 0.0f, 0.0f}, g, i);
#pragma unroll
    for (int r = 0; r < 4; r++) da[wave][4 * g + r][i] = dav[r];
  }
  __syncthreads();
  if (wave != 0) return;
  // ---- the head's derivative (include/mcg.h), and the outputs
  const float alpha = log_ent_coef ? (float)exp((double)*log_ent_coef) : ent_coef;
  f4 dmu = {0.0f, 0.0f, 0.0f, 0.0f}, dls = {0.0f, 0.0f, 0.0f, 0.0f}, dqda;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int comp = 4 * g + r;
    dqda[r] = da[0][comp][i] + da[1][comp][i];
    if (live && comp < PA.A) {
      const double a = (double)dr.action[r], sq = 1.0 - a * a;
      const double du = ((double)alpha * (2.0 * a * sq / (sq + 1e-6)) - (double)dqda[r] * sq) * inv_b;
      dmu[r] = (float)du;
      const bool clamped = ls[0][r] < LOG_STD_MIN || ls[0][r] > LOG_STD_MAX;
      dls[r] = clamped ? 0.0f : (float)(du * exp((double)dr.log_std[r]) * (double)dr.noise[r] - (double)alpha * inv_b);
      const size_t at = (size_t)s * PA.A + comp;
      if (O.action) O.action[at] = dr.action[r];
      if (O.noise) O.noise[at] = dr.noise[r];
      if (O.dq_da) O.dq_da[at] = dqda[r];
    }
  }
  const bool mine = live && g == 0;
  if (mine) {
    O.logp[s] = dr.log_prob;
    if (O.q_pi) { O.q_pi[s] = q0; O.q_pi[(size_t)B + s] = q1; }
  }
  const float term = sum16(mine ? fmaf(alpha, dr.log_prob, -fminf(q0, q1)) : 0.0f), lps = sum16(mine ? dr.log_prob : 0.0f);
  if (lane == 0) { work[4 + 8 * (size_t)tile] = term; work[4 + 8 * (size_t)tile + 1] = lps; }
  // ---- the actor's backward pass: the two heads onto the last hidden layer, then down the trunk
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  d[0] = dmu;
  store_rows<MT>(chunk, sel4(RA.d, n), 1, d, g, i);
  f4 d2[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d2[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  d2[0] = dls;
  store_rows<MT>(chunk, RA.d2, 1, d2, g, i);
  {
    const int nti = last_tiles(net);
    const float* __restrict__ Wmu = PA.blob + sel4(PA.net[1].w, n);
    const float* __restrict__ Wls = PA.blob + sel4(PA.net[0].w, n);
    const float* yv = chunk + (size_t)sel4(RA.x, n) * TILE;
    f4 e[MT];
#pragma unroll
    for (int T = 0; T < MT; T++) {
      e[T] = f4{0.0f, 0.0f, 0.0f, 0.0f};
      if (T < nti) {
        f4 cc = wt_acc<MT>(Wmu, 4 * nti, T, 1, d, f4{0.0f, 0.0f, 0.0f, 0.0f}, g, i);
        cc = wt_acc<MT>(Wls, 4 * nti, T, 1, d2, cc, g, i);
#pragma unroll
        for (int r = 0; r < 4; r++) cc[r] *= act_prime(PA.act, yv[(size_t)(16 * T + 4 * g + r) * TILE + i]);
        e[T] = cc;
      }
    }
    store_rows<MT>(chunk, sel4(RA.d, n - 1), nti, e, g, i);
#pragma unroll
    for (int t = 0; t < MT; t++) d[t] = e[t];
  }
  walk_back<MT, true>(PA, net, RA, chunk, n - 1, 0, d, g, i);
}

// grad[p] = the partial blobs' sum in part order; the last block: the tiles' sums -> stats (actor: 0 the critic entry, 1 the actor's).
__global__ __launch_bounds__(256) void sac_reduce_kernel(const float* __restrict__ work, const float* __restrict__ partials, int parts,
                                                         long long blob_floats, int ntiles, int actor, float inv_b, float ent_coef,
                                                         const float* __restrict__ log_ent_coef, float* __restrict__ grad,
                                                         float* __restrict__ stats) {
  if (reduced_parts(partials, parts, blob_floats, grad) || threadIdx.x >= WAVE) return;
  float acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
  for (int t = threadIdx.x; t < ntiles; t += WAVE)
#pragma unroll
    for (int j = 0; j < 4; j++) acc[j] += work[4 + 8 * (size_t)t + j];
#pragma unroll
  for (int j = 0; j < 4; j++) acc[j] = sum64(acc[j]);
  if (threadIdx.x != 0) return;
  if (actor) {
    stats[1] = acc[0] * inv_b;
    stats[3] = log_ent_coef ? (float)exp((double)*log_ent_coef) : ent_coef;
    stats[6] = acc[1] * inv_b;
  } else {
    stats[0] = 0.5f * (acc[0] * inv_b + acc[1] * inv_b);
    stats[4] = acc[2] * inv_b; stats[5] = acc[3] * inv_b; stats[7] = 0.0f;
  }
}

// The mean of logp + target_entropy in double in a fixed tree; the loss, the gradient, and Adam's rule on the one float (lr > 0).
__global__ __launch_bounds__(1024) void sac_alpha_kernel(float* __restrict__ log_ent_coef, const float* __restrict__ logp, long long B,
                                                         float target_entropy, float* __restrict__ m, float* __restrict__ v, int adam,
                                                         float beta1, float beta2, float omb1, float omb2, float step_size, float bc2_sqrt, float eps,
                                                         float* __restrict__ grad_out, float* __restrict__ stats) {
  __shared__ double lds[1024];
  double sum = 0.0;
  for (long long j = threadIdx.x; j < B; j += 1024) sum += (double)logp[j] + (double)target_entropy;
  const double mean = block_sum(sum, lds) / (double)B;
  if (threadIdx.x != 0) return;
  const float gj = (float)(-mean);
  if (grad_out) grad_out[0] = gj;
  if (stats) stats[2] = (float)(-(double)log_ent_coef[0] * mean);
  if (adam) adam_one(log_ent_coef, gj, m, v, 0, beta1, beta2, omb1, omb2, step_size, bc2_sqrt, eps);
}

// ------------------------------------------------------------------------------------------------------- host side
bool checked_adam(const char* who, int64_t step, double lr, double beta1, double beta2, double eps) {
  if (step < 1) { mcg_fail(MCG_ERR_ARG, "%s: step must be >= 1", who); return false; }
  if (!(lr >= 0.0) || !std::isfinite(lr)) { mcg_fail(MCG_ERR_ARG, "%s: lr must be finite and >= 0", who); return false; }
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) {
    mcg_fail(MCG_ERR_ARG, "%s: beta1 and beta2 must be in [0, 1)", who); return false; }
  if (!(eps >= 0.0) || !std::isfinite(eps)) { mcg_fail(MCG_ERR_ARG, "%s: eps must be finite and >= 0", who); return false; }
  return true;
}

}  // namespace

extern "C" {

int64_t mcg_sac_grad_work_floats(const mcg_sac* sac, int64_t B) {
  Sac S = {};
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (!sac || !rows_in_range(B)) return 0;
  if (blob_plan(sac->obs_dim, sac->act_dim, sac->n_pi, sac->pi_width, sac->n_qf, sac->qf_width, 2, true, &S, &actor, &critic, &why) == 0) return 0;
  const long long c = critic_layout(S, B, widest(sac, false, true), critic, 2).need;
  const long long a = actor_layout(S, B, widest(sac, true, false), actor, true, 2).need;
  return c > a ? c : a;
}

int mcg_sac_critic_grad(const mcg_sac* sac, const mcg_sac_rows* rows, const float* y, int64_t B, float* work, int64_t work_floats,
                        float* grad, float* stats, void* stream) {
  const char* who = "mcg_sac_critic_grad";
  Sac S = {};
  if (!checked_sac(who, sac, NEED_CRITIC, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, true)) return MCG_ERR_ARG;
  if (!y) return mcg_fail(MCG_ERR_ARG, "%s: y is null", who);
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const int wq = widest(sac, false, true);
  const Layout Y = critic_layout(S, B, wq, sac->critic_floats, 2);
  if (!checked_work(who, work, work_floats, Y.need, "mcg_sac_grad_work_floats")) return MCG_ERR_ARG;
  S.qf[0].blob = sac->critic;
  S.qf[1].blob = sac->critic + sac->critic_floats / 2;
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, rows->action};
  const float inv_b = (float)(1.0 / (double)B);
  const dim3 grid(Y.ntiles, 2), block(WAVE);
  if (wq <= 64) hipLaunchKernelGGL((critic_tile_kernel<4, false>), grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  else hipLaunchKernelGGL((critic_tile_kernel<16, false>), grid, block, 0, st, S, Y.q, X, y, (int)B, inv_b, work);
  hipLaunchKernelGGL(dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)sac->critic_floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(sac_reduce_kernel, dim3(blocks(sac->critic_floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)sac->critic_floats, Y.ntiles, 0, inv_b, 0.0f,
                     (const float*)nullptr, grad, stats);
  return launched(who);
}

int mcg_sac_actor_grad(const mcg_sac* sac, const mcg_sac_rows* rows, int64_t B, uint64_t seed, uint64_t call, float ent_coef,
                       const float* log_ent_coef, float* work, int64_t work_floats, float* grad, float* logp_out, float* stats,
                       const mcg_sac_actor_grad_out* out, void* stream) {
  const char* who = "mcg_sac_actor_grad";
  Sac S = {};
  if (!checked_sac(who, sac, NEED_ACTOR | NEED_CRITIC, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, false)) return MCG_ERR_ARG;
  if (!log_ent_coef && !(ent_coef >= 0.0f && ent_coef <= 3.0e38f))
    return mcg_fail(MCG_ERR_ARG, "%s: ent_coef must be finite and >= 0 where log_ent_coef is null", who);
  if (!logp_out) return mcg_fail(MCG_ERR_ARG, "%s: logp_out is null", who);
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  if (!checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  const Layout Y = actor_layout(S, B, widest(sac, true, false), sac->actor_floats, true, 2);
  if (!checked_work(who, work, work_floats, Y.need, "mcg_sac_grad_work_floats")) return MCG_ERR_ARG;
  S.qf[0].blob = sac->critic;
  S.qf[1].blob = sac->critic + sac->critic_floats / 2;
  const hipStream_t st = (hipStream_t)stream;
  const SRows X = {rows->obs, rows->achieved, rows->desired, nullptr};
  ActorOut O = {nullptr, nullptr, nullptr, nullptr, logp_out};
  if (out) { O.action = out->action; O.noise = out->noise; O.q_pi = out->q_pi; O.dq_da = out->dq_da; }
  const double inv_b = 1.0 / (double)B;
  const dim3 grid(Y.ntiles), block(2 * WAVE);
#define MCG_SAC_ACTOR_TILE(MT) hipLaunchKernelGGL(sac_actor_tile_kernel<MT>, grid, block, 0, st, S, Y.a, Y.q, X, (int)B, (unsigned long long)seed, \
                                                  (unsigned long long)call, ent_coef, log_ent_coef, inv_b, work, O)
  if (widest(sac, true, true) <= 64) MCG_SAC_ACTOR_TILE(4);
  else MCG_SAC_ACTOR_TILE(16);
#undef MCG_SAC_ACTOR_TILE
  hipLaunchKernelGGL(dw_kernel, dim3(Y.blocks.total, Y.parts), dim3(WAVE), 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)sac->actor_floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(sac_reduce_kernel, dim3(blocks(sac->actor_floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)sac->actor_floats, Y.ntiles, 1, (float)inv_b, ent_coef,
                     log_ent_coef, grad, stats);
  return launched(who);
}

int mcg_sac_alpha_step(float* log_ent_coef, const float* logp, int64_t B, float target_entropy, float* m, float* v, int64_t step,
                       double lr, double beta1, double beta2, double eps, float* grad_out, float* stats, void* stream) {
  const char* who = "mcg_sac_alpha_step";
  if (!log_ent_coef) return mcg_fail(MCG_ERR_ARG, "%s: log_ent_coef is null", who);
  if (!logp) return mcg_fail(MCG_ERR_ARG, "%s: logp is null", who);
  if (!checked_rows(who, B)) return MCG_ERR_ARG;
  if (!std::isfinite(target_entropy)) return mcg_fail(MCG_ERR_ARG, "%s: target_entropy must be finite", who);
  if (!checked_adam(who, step, lr, beta1, beta2, eps)) return MCG_ERR_ARG;
  const int adam = lr > 0.0;
  if (adam && (!m || !v)) return mcg_fail(MCG_ERR_ARG, "%s: m and v are required where lr > 0", who);
  const AdamStep a = adam_step(step, lr, beta1, beta2);
  hipLaunchKernelGGL(sac_alpha_kernel, dim3(1), dim3(1024), 0, (hipStream_t)stream, log_ent_coef, logp, (long long)B, target_entropy, m, v, adam,
                     (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), a.step_size, a.bc2_sqrt, (float)eps, grad_out, stats);
  return launched(who);
}

int mcg_sac_adam(float* blob, const float* grad, float* m, float* v, int64_t floats, int64_t step, double lr, double beta1, double beta2,
                 double eps, void* stream) {
  const char* who = "mcg_sac_adam";
  if (!checked_buffer(who, blob, "blob") || !checked_buffer(who, grad, "grad") || !checked_buffer(who, m, "m") || !checked_buffer(who, v, "v"))
    return MCG_ERR_ARG;
  if (floats < 1 || floats >= (1ll << 31)) return mcg_fail(MCG_ERR_ARG, "%s: floats must be in [1, 2^31)", who);
  if (!checked_adam(who, step, lr, beta1, beta2, eps)) return MCG_ERR_ARG;
  const AdamStep a = adam_step(step, lr, beta1, beta2);
  hipLaunchKernelGGL(adam_kernel<256>, dim3(blocks(floats, 256)), dim3(256), 0, (hipStream_t)stream, blob, grad, m, v, (long long)floats,
                     (const float*)nullptr, 0.0f, (float)beta1, (float)beta2, (float)(1.0 - beta1), (float)(1.0 - beta2), a.step_size,
                     a.bc2_sqrt, (float)eps);
  return launched(who);
}

}  // extern "C"
