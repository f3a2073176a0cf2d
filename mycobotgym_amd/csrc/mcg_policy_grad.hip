// mcg_policy_grad.hip -- the policy update (include/mcg.h: mcg_policy_evaluate, mcg_policy_grad, mcg_policy_adam): SB3's
// evaluate_actions, the PPO / A2C loss and its gradient with respect to every parameter of the blob, and clip-by-norm + Adam on the
// blob in place.  A code object of its own, as mcg_policy.hip, whose blob plan, operand map and forward helpers it shares
// (mcg_policy.hpp).  Float32 throughout on v_mfma_f32_16x16x4_f32; deterministic: no atomics, every sum in an order that the shape
// and B alone fix.
//
// ---- The three products of a layer, in tiles of 16 samples.  Lane l = 16 g + i holds A[i][g] and B[g][i], and afterwards D[4 g + r][i]
// in register r (mcg_policy.hip's head; the two arrangements below against a host product: tools/microbench/mfma_f32_grad.hip).
//   Z = W X          the forward as it stands: register r of tile t is the B operand of k-block 4 t + r of the next layer.
//   dX = W^T dZ      dZ is in the accumulator layout too (lane 16 g + i: units 16 t + 4 g + r of sample i), so register r of tile t is
//                    again the B operand of a k-block, the units {16 t + 4 g + r : g}.  The A operand of that block and output tile T'
//                    is W[16 t + 4 g + r][16 T' + i]: in the blob that is tile (t, 4 T' + (i & 3)), float 16 (i >> 2) + 4 g + r -- for
//                    r = 0..3 four consecutive floats, one 16-byte load per lane out of L2 (the blob is at most 620 KB).  No second
//                    packed copy of the weights exists.
//   dW = dZ X^T      the sum runs over samples, four per instruction.  Both operands are re-laid through memory as rows of 16 samples:
//                    row u = unit u (of dZ) or input column u (of X), float s = sample s of the tile.  Lane 16 g + i then reads the four
//                    floats 4 g .. 4 g + 3 of row 16 T + i (A) and of row 16 C + i (B) in one 16-byte load each, and instruction
//                    q = 0..3 sums the samples {4 g + q : g}: which four samples share an instruction does not matter to a sum.  The
//                    result, dW[16 T + 4 g + r][16 C + i] in register r, lies in the blob at four consecutive floats again.  A bias
//                    (and log_std) is the same product with X = 1.
//
// ---- Work split.  grad_tile_kernel: one wave per tile of 16 samples and net, as the forward.  It runs the forward, keeps every layer's
// activations as rows in `work` (not in registers: at [256, 256] they would not fit, and the dW product wants them re-laid anyway),
// forms the loss's derivative at the head, walks back through W^T, and leaves every layer's dZ rows beside the activations.  It re-reads
// its own activation rows for tanh' = 1 - y^2 / relu' = [y > 0].  dw_kernel: one wave per 16 x 16 block of a weight matrix (or
// 16 biases) and part: it walks the part's tiles of samples in order and writes its block of the part's partial blob.  The blob has
// few blocks (about 75 at [64, 64]), so the samples are split into at most 16 parts (4 at widths above 64): 4096 samples at [64, 64]
// are 256 tiles, 16 parts of 16 tiles, about 1200 waves.  grad_reduce_kernel adds the partial blobs in part order, adds the entropy
// term's exact -ent_coef to log_std, and sums the tiles' loss terms in a fixed tree into `stats`.  adv_stats_kernel (one workgroup,
// double accumulators, a fixed tree) writes the advantage's mean and std + 1e-8 first where they are used.
//
// ---- `work` (floats):  [0] advantage mean, [1] std + 1e-8, [2..3] unused, [4..5] and [6..7] the same two as doubles;
// [8 + 8 tile + s] the tile's sums: s = 2 squared value error, 4 kl term, 5 clipped count, 6..7 the policy term as one double;  then
// per net and tile `rows` rows of 16 floats (the row map: mcg_grad.hpp's struct GRows);  then `parts` partial blobs.  Every float that is read was
// written by the same call.
//
// ---- A2C's policy term in double.  Its summands adv * log_prob have the log-prob's magnitude (about -1.4 A: 13 on average at
// A = 13) and, the advantages being centred, a mean of a few tenths; `loss` then subtracts again.  The float32 mean of the advantages
// is off by up to 2^-25 of itself, which the normalisation turns into that much times mean(log_prob) / std in the term's mean, and
// the rounding of each normalised advantage enters times its log-prob.  So the statistic's term takes the advantage's mean and std,
// the normalised advantage, the log-prob (at hand in double already) and the sums over the tile and the tiles in double, and is
// rounded once.  PPO's term min(adv ratio, adv clip(ratio)) stays the float32 expression and goes through the same sums.  The
// gradient goes through neither: d loss / d log_prob keeps the float32 normalised advantage.
//
// ---- A ragged last tile: its extra lanes read the last valid sample, as in the forward, and their dZ is set to +-0 at the head, so
// that every product they enter adds exactly nothing.
//
// ---- Shared with SAC and TD3 / DDPG (mcg_grad.hpp): the row map, the rows' stores, the hidden layers' forward, the walk back through
// W^T, the dW kernel and its block list, the reduce's two helpers, Adam's kernel.  Shared with the forwards (mcg_policy.hpp): the
// Gaussian head's log-prob, its derivative and the entropy.  Here: the pick of one of the two nets, the PPO / A2C loss, the statistic in double, the advantage's and the gradient's norm kernels, the log_std block.
#include "mcg_grad.hpp"       // GRows, Blocks, sum16, sum64, store_rows, store_features, hidden_rows, walk_back, dw_kernel, reduced_parts,
                              // block_sum, adam_kernel, adam_step, number_rows, layer_block, add_block, split_parts, checked_buffer

using namespace mcg;

namespace {

constexpr int SUMS = 8;                                                 // the tiles' sums start here in `work`

struct Batch { const float *obs, *ach, *des, *action, *old_lp, *adv, *ret; };
struct Hyper { int kind, norm; float clip, ent_coef, vf_coef, inv_b; double inv_bd; };      // inv_bd: 1 / B for the sums held in double

// sum16 (mcg_grad.hpp) in double
MCG_DEV double sum16d(double x) {
  x += __shfl_xor(x, 8); x += __shfl_xor(x, 4); x += __shfl_xor(x, 2); x += __shfl_xor(x, 1);
  return x;
}

// R[k] by selects, as pick() of a Net (mcg_policy.hpp); a value net has no d2 rows
MCG_DEV GRows pick(const GRows& x, const GRows& y, int k) {
  GRows z = {};
#pragma unroll
  for (int L = 0; L <= MAX_LAYERS; L++) { z.x[L] = k ? y.x[L] : x.x[L]; z.d[L] = k ? y.d[L] : x.d[L]; }
  z.d2 = k ? y.d2 : x.d2; z.rows = k ? y.rows : x.rows; z.fr = k ? y.fr : x.fr; z.base = k ? y.base : x.base;
  return z;
}

// GRAD = false: mcg_policy_evaluate (no `work`);  true: the forward, the loss's derivative and the backward pass of one tile and net.
template <int MT, bool GRAD>
__global__ __launch_bounds__(WAVE) void grad_tile_kernel(Pol P, GRows R0, GRows R1, Batch X, Hyper H, float* work, EvalOut E) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int tile = blockIdx.x, s = tile * TILE + i;
  const bool live = s < P.N;
  const int row = live ? s : P.N - 1;    // a ragged tile's extra lanes read a valid row and contribute nothing
  const int k = blockIdx.y;              // 0: the value net; 1: the policy net
  if (!GRAD && k == 0 && !E.value) return;
  const Net net = pick(P.net[0], P.net[1], k);
  const GRows R = pick(R0, R1, k);
  float* chunk = GRAD ? work + R.base + (size_t)tile * R.rows * TILE : nullptr;
  const int n = net.n;
  // ---- forward
  f4 a[MT];
  first_layer<MT, float>(P, net, X.obs, X.ach, X.des, row, g, lane, a);
  if (GRAD) store_features(chunk, R.x[0], R.fr, P.D, X.obs, X.ach, X.des, row, g, i);
  hidden_rows<MT>(P, net, R, chunk, GRAD, a, g, i, lane);
  f4 head[1];
  dense<MT, 1>(P, net, n, n == 1 ? net.nt[0] : n == 2 ? net.nt[1] : net.nt[2], 1, a, head, g, lane);
  const f4 h = head[0];                  // lane 16 g + i: rows 4 g + r of the head, sample i
  // ---- the head: outputs (evaluate), or the loss's derivative dh with respect to the head's rows
  f4 dh = {0.0f, 0.0f, 0.0f, 0.0f};
  if (k == 0) {
    if (!GRAD) {
      if (live && g == 0) E.value[s] = h[0];
      return;
    }
    const float diff = h[0] - X.ret[row];                       // (lanes g == 0 hold the value: row 0 of the head)
    const bool mine = live && g == 0;
    if (mine) dh[0] = (2.0f * H.vf_coef * H.inv_b) * diff;
    const float sq = sum16(mine ? diff * diff : 0.0f);
    if (lane == 0) work[SUMS + 8 * (size_t)tile + 2] = sq;
  } else {
    const f4 ls = *reinterpret_cast<const f4*>(P.blob + P.log_std + 4 * g);
    f4 dmu, dls;                         // the Gaussian head (mcg_policy.hpp): the log-prob in double, rounded once, and its derivative
    const double lpd = gauss_log_prob(P.A, h, ls, X.action, (size_t)row, g, dmu, dls);
    if (!GRAD) {
      if (live && g == 0) {
        if (E.log_prob) E.log_prob[s] = (float)lpd;
        if (E.entropy) E.entropy[s] = gauss_entropy(P.A, P.blob + P.log_std);
      }
      return;
    }
    float adv = X.adv[row];
    double advd = (double)adv;                                  // (the statistic's: see the head)
    if (H.norm) {
      const double* __restrict__ nd = reinterpret_cast<const double*>(work + 4);
      advd = (advd - nd[0]) / nd[1];
      adv = (adv - work[0]) / work[1];
    }
    float dlp, kl = 0.0f, clipped = 0.0f;                      // d loss / d log_prob
    double term;                                                // the sample's policy term (its loss is -term)
    if (H.kind == MCG_LOSS_PPO) {
      const double lrd = lpd - (double)X.old_lp[row];
      const float lr = (float)lrd, ratio = expf(lr);
      const float s1 = adv * ratio, s2 = adv * fminf(fmaxf(ratio, 1.0f - H.clip), 1.0f + H.clip);
      term = (double)fminf(s1, s2);
      dlp = s1 <= s2 ? -(adv * ratio) * H.inv_b : 0.0f;         // the clipped branch is a constant
      kl = (float)(expm1(lrd) - lrd);
      clipped = fabsf(ratio - 1.0f) > H.clip ? 1.0f : 0.0f;
    } else {
      term = advd * lpd;
      dlp = -adv * H.inv_b;
    }
    if (!live) { term = 0.0; dlp = 0.0f; kl = 0.0f; clipped = 0.0f; }
    f4 dl;
#pragma unroll
    for (int r = 0; r < 4; r++) { dh[r] = dlp * dmu[r]; dl[r] = dlp * dls[r]; }
    const double st = sum16d(term);
    const float sk = sum16(kl), sc = sum16(clipped);
    if (lane == 0) {
      *reinterpret_cast<double*>(work + SUMS + 8 * (size_t)tile + 6) = st;       // (8-byte aligned: `work` is 16-byte aligned)
      work[SUMS + 8 * (size_t)tile + 4] = sk; work[SUMS + 8 * (size_t)tile + 5] = sc;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) chunk[(size_t)(R.d2 + 4 * g + r) * TILE + i] = dl[r];
  }
  // ---- backward: d[t] is dZ of layer L in the accumulator layout; dZ of layer L - 1 = act'(y) * (W_L^T dZ_L)
  f4 d[MT];
#pragma unroll
  for (int t = 0; t < MT; t++) d[t] = f4{0.0f, 0.0f, 0.0f, 0.0f};
  d[0] = dh;
  store_rows<MT>(chunk, sel4(R.d, n), 1, d, g, i);
  walk_back<MT, true>(P, net, R, chunk, n, 0, d, g, i);
}

// grad[p] = the partial blobs' sum in part order (log_std: and the entropy term's -ent_coef); the last block: the tiles' sums -> stats.
__global__ __launch_bounds__(256) void grad_reduce_kernel(const float* __restrict__ work, const float* __restrict__ partials, int parts,
                                                          long long blob_floats, int ntiles, const float* __restrict__ blob, int log_std,
                                                          int A, Hyper H, float* __restrict__ grad, float* __restrict__ stats) {
  if (reduced_parts(partials, parts, blob_floats, grad, log_std, A, H.ent_coef) || threadIdx.x >= WAVE) return;
  float acc[3] = {0.0f, 0.0f, 0.0f};
  double term = 0.0;
  constexpr int slot[3] = {2, 4, 5};
  for (int t = threadIdx.x; t < ntiles; t += WAVE) {
#pragma unroll
    for (int j = 0; j < 3; j++) acc[j] += work[SUMS + 8 * (size_t)t + slot[j]];
    term += *reinterpret_cast<const double*>(work + SUMS + 8 * (size_t)t + 6);
  }
#pragma unroll
  for (int j = 0; j < 3; j++) acc[j] = sum64(acc[j]);
  term = sum64(term);
  if (threadIdx.x == 0) {
    const float ent = gauss_entropy(A, blob + log_std);
    const double policy_loss = -term * H.inv_bd;
    const float value_loss = acc[0] * H.inv_b, entropy_loss = -ent;
    stats[0] = (float)(policy_loss + (double)H.ent_coef * (double)entropy_loss + (double)H.vf_coef * (double)value_loss);
    stats[1] = (float)policy_loss; stats[2] = value_loss; stats[3] = entropy_loss;
    stats[4] = acc[1] * H.inv_b; stats[5] = acc[2] * H.inv_b; stats[6] = 0.0f; stats[7] = 0.0f;
  }
}

// out[0] = mean, out[1] = std + 1e-8 (the unbiased deviation, as torch.std) of adv[0..B); out[4..5] and out[6..7]: the two as doubles
__global__ __launch_bounds__(1024) void adv_stats_kernel(const float* __restrict__ adv, long long B, float* __restrict__ out) {
  __shared__ double lds[1024];
  double s = 0.0;
  for (long long j = threadIdx.x; j < B; j += 1024) s += (double)adv[j];
  const double mean = block_sum(s, lds) / (double)B;
  double q = 0.0;
  for (long long j = threadIdx.x; j < B; j += 1024) { const double c = (double)adv[j] - mean; q += c * c; }
  const double var = block_sum(q, lds) / (double)(B - 1);
  if (threadIdx.x == 0) {
    out[0] = (float)mean; out[1] = (float)sqrt(var) + 1e-8f;
    double* outd = reinterpret_cast<double*>(out + 4);
    outd[0] = mean; outd[1] = sqrt(var) + 1e-8;
  }
}

__global__ __launch_bounds__(1024) void grad_norm_kernel(const float* __restrict__ grad, long long n, float* __restrict__ norm_out) {
  __shared__ double lds[1024];
  double s = 0.0;
  for (long long j = threadIdx.x; j < n; j += 1024) { const double x = (double)grad[j]; s += x * x; }
  const double sum = block_sum(s, lds);
  if (threadIdx.x == 0) norm_out[0] = (float)sqrt(sum);
}

// ------------------------------------------------------------------------------------------------------- host side
struct Layout { GRows rows[2]; Blocks blocks; int ntiles, tpp, parts; long long partials, floats; };

// The row map, the block list and the split of `work` for a planned shape and B.
Layout layout(const Pol& P, int64_t B, int widest) {
  Layout Y = {};
  Y.ntiles = (int)((B + TILE - 1) / TILE);
  split_parts(Y.ntiles, widest, &Y.tpp, &Y.parts);
  const int fr = (P.D + 6 + 15) / 16 * 16;
  long long at = SUMS + 8ll * Y.ntiles;
  for (int k = 0; k < 2; k++) {
    GRows& R = Y.rows[k];
    R.rows = number_rows(R, P.net[k], fr, false);
    if (k == 1) { R.d2 = R.rows; R.rows += 16; }               // the log_std terms: a second head's dZ rows
    R.base = at;
    at += (long long)Y.ntiles * R.rows * TILE;
  }
  Y.partials = at;
  int blk = 0;
  for (int k = 1; k >= 0; k--) {         // the blob's order: the policy net first
    const Net& net = P.net[k];
    const GRows& R = Y.rows[k];
    for (int L = 0; L <= net.n; L++) add_block(Y.blocks, blk, layer_block(P, net, R, L));
    if (k == 1) {                        // log_std: a bias whose dZ is the policy net's log_std rows
      Block b = {};
      b.nT = 1; b.ncb = 0; b.nb = 1; b.drow = R.d2; b.b = P.log_std; b.rows = R.rows; b.base = R.base;
      add_block(Y.blocks, blk, b);
    }
  }
  Y.blocks.total = blk;
  return Y;
}

int check_batch(const char* who, const mcg_rollout_batch* batch, int64_t B) {
  if (!batch) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_rollout_batch", who);
  if (!batch->obs || !batch->achieved || !batch->desired || !batch->action)
    return mcg_fail(MCG_ERR_ARG, "%s: obs, achieved, desired and action of the batch are required", who);
  return checked_rows(who, B) ? MCG_OK : MCG_ERR_ARG;
}

}  // namespace

extern "C" {

int mcg_policy_evaluate(const mcg_policy* pol, const mcg_rollout_batch* batch, int64_t B, const mcg_policy_eval_out* out, void* stream) {
  const char* who = "mcg_policy_evaluate";
  Pol P = {};
  if (checked_plan(who, pol, &P) == 0) return MCG_ERR_ARG;
  if (const int e = check_batch(who, batch, B)) return e;
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy_eval_out", who);
  if (!out->value && !out->log_prob && !out->entropy) return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  P.N = (int)B;
  const Batch X = {batch->obs, batch->achieved, batch->desired, batch->action, nullptr, nullptr, nullptr};
  const EvalOut E = {out->value, out->log_prob, out->entropy};
  const GRows none = {};
  const dim3 grid(blocks(B, TILE), (out->log_prob || out->entropy) ? 2 : 1), block(WAVE);
  if (widest_layer(pol) <= 64) hipLaunchKernelGGL((grad_tile_kernel<4, false>), grid, block, 0, (hipStream_t)stream, P, none, none, X, Hyper{}, nullptr, E);
  else hipLaunchKernelGGL((grad_tile_kernel<16, false>), grid, block, 0, (hipStream_t)stream, P, none, none, X, Hyper{}, nullptr, E);
  return launched("mcg_policy_evaluate");
}

int64_t mcg_policy_grad_work_floats(const mcg_policy* pol, int64_t B) {
  Pol P = {};
  const char* why = nullptr;
  if (!pol || !rows_in_range(B)) return 0;
  const int64_t floats = plan(pol->obs_dim, pol->act_dim, pol->n_pi, pol->pi_width, pol->n_vf, pol->vf_width, &P, &why);
  if (floats == 0) return 0;
  const Layout Y = layout(P, B, widest_layer(pol));
  return Y.partials + (int64_t)Y.parts * floats;
}

int mcg_policy_grad(const mcg_policy* pol, const mcg_rollout_batch* batch, int64_t B, const mcg_policy_hyper* hyper, float* work,
                    int64_t work_floats, float* grad, float* stats, void* stream) {
  const char* who = "mcg_policy_grad";
  Pol P = {};
  const int64_t floats = checked_plan(who, pol, &P);
  if (floats == 0) return MCG_ERR_ARG;
  if (const int e = check_batch(who, batch, B)) return e;
  if (!hyper) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy_hyper", who);
  if (hyper->loss_kind != MCG_LOSS_PPO && hyper->loss_kind != MCG_LOSS_A2C)
    return mcg_fail(MCG_ERR_ARG, "%s: loss_kind must be MCG_LOSS_PPO or MCG_LOSS_A2C", who);
  if (hyper->loss_kind == MCG_LOSS_PPO && !(hyper->clip_range > 0.0f)) return mcg_fail(MCG_ERR_ARG, "%s: clip_range must be > 0 for MCG_LOSS_PPO", who);
  if (!batch->advantage || !batch->returns) return mcg_fail(MCG_ERR_ARG, "%s: advantage and returns of the batch are required", who);
  if (hyper->loss_kind == MCG_LOSS_PPO && !batch->old_log_prob) return mcg_fail(MCG_ERR_ARG, "%s: old_log_prob of the batch is required for MCG_LOSS_PPO", who);
  if (!checked_buffer(who, work, "work") || !checked_buffer(who, grad, "grad")) return MCG_ERR_ARG;
  if (!stats) return mcg_fail(MCG_ERR_ARG, "%s: stats is null", who);
  const int widest = widest_layer(pol);
  const Layout Y = layout(P, B, widest);
  const int64_t need = Y.partials + (int64_t)Y.parts * floats;
  if (work_floats < need)
    return mcg_fail(MCG_ERR_ARG, "%s: work_floats is %lld, mcg_policy_grad_work_floats gives %lld for this shape and B", who,
                    (long long)work_floats, (long long)need);
  P.N = (int)B;
  const hipStream_t st = (hipStream_t)stream;
  const Batch X = {batch->obs, batch->achieved, batch->desired, batch->action, batch->old_log_prob, batch->advantage, batch->returns};
  const Hyper H = {hyper->loss_kind, hyper->normalize_advantage != 0 && B > 1, hyper->clip_range, hyper->ent_coef, hyper->vf_coef,
                   (float)(1.0 / (double)B), 1.0 / (double)B};
  if (H.norm) hipLaunchKernelGGL(adv_stats_kernel, dim3(1), dim3(1024), 0, st, batch->advantage, (long long)B, work);
  const dim3 grid(Y.ntiles, 2), block(WAVE);
  if (widest <= 64) hipLaunchKernelGGL((grad_tile_kernel<4, true>), grid, block, 0, st, P, Y.rows[0], Y.rows[1], X, H, work, EvalOut{});
  else hipLaunchKernelGGL((grad_tile_kernel<16, true>), grid, block, 0, st, P, Y.rows[0], Y.rows[1], X, H, work, EvalOut{});
  hipLaunchKernelGGL(dw_kernel, dim3(Y.blocks.total, Y.parts), block, 0, st, Y.blocks, (const float*)work, work + Y.partials,
                     (long long)floats, Y.ntiles, Y.tpp);
  hipLaunchKernelGGL(grad_reduce_kernel, dim3(blocks(floats, 256) + 1), dim3(256), 0, st, (const float*)work,
                     (const float*)(work + Y.partials), Y.parts, (long long)floats, Y.ntiles, pol->blob, P.log_std, P.A, H, grad, stats);
  return launched("mcg_policy_grad");
}

int mcg_policy_adam(const mcg_policy* pol, const float* grad, float* m, float* v, int64_t step, double lr, double beta1, double beta2,
                    double eps, double max_grad_norm, float* norm_out, void* stream) {
  const char* who = "mcg_policy_adam";
  Pol P = {};
  const int64_t floats = checked_plan(who, pol, &P);
  if (floats == 0) return MCG_ERR_ARG;
  if (!checked_buffer(who, grad, "grad") || !checked_buffer(who, m, "m") || !checked_buffer(who, v, "v")) return MCG_ERR_ARG;
  if (!norm_out) return mcg_fail(MCG_ERR_ARG, "%s: norm_out is null", who);
  if (step < 1) return mcg_fail(MCG_ERR_ARG, "%s: step must be >= 1", who);
  if (!(beta1 >= 0.0 && beta1 < 1.0) || !(beta2 >= 0.0 && beta2 < 1.0)) return mcg_fail(MCG_ERR_ARG, "%s: beta1 and beta2 must be in [0, 1)", who);
  if (!std::isfinite(lr) || !(eps >= 0.0) || !std::isfinite(max_grad_norm)) return mcg_fail(MCG_ERR_ARG, "%s: lr, eps and max_grad_norm must be finite, eps >= 0", who);
  const AdamStep a = adam_step(step, lr, beta1, beta2);
  const float max_norm = (float)max_grad_norm, b1 = (float)beta1, b2 = (float)beta2;
  const hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(grad_norm_kernel, dim3(1), dim3(1024), 0, st, grad, (long long)floats, norm_out);
  hipLaunchKernelGGL(adam_kernel<256>, dim3(blocks(floats, 256)), dim3(256), 0, st, const_cast<float*>(pol->blob), grad, m, v, (long long)floats,
                     max_norm > 0.0f ? (const float*)norm_out : nullptr, max_norm, b1, b2, 1.0f - b1, 1.0f - b2, a.step_size, a.bc2_sqrt,
                     (float)eps);
  return launched("mcg_policy_adam");
}

}  // extern "C"
