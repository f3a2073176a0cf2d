// mcg_policy.hip -- the actor-critic policy forward of on-policy collection (include/mcg.h: mcg_policy_*): SB3's MultiInputPolicy for a
// Dict space of Boxes -- two MLP trunks without shared layers, a diagonal Gaussian -- as one launch that reads the engine's float64
// observation in place and writes action, value and log-prob in the forms mcg_rollout_add takes.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  Kernel and C entries are both here.  The
// C side is stateless; of mcg_engine.hpp it uses the error reporting alone.
//
// ---- Work split.  One wave per tile of 16 environments and net, one wave per workgroup: the value net and the policy net of a tile
// share nothing but the input, so they are two workgroups (grid.y), and 8192 environments are 1024 waves, about one per SIMD; the
// value-only call launches the value net's half.  Every layer is the transposed product on v_mfma_f32_16x16x4_f32, float32 in and out:
//     D[unit][env] += W[unit][k] * X[k][env]        A operand: 16 units x 4 k of the weights, B operand: 4 k x 16 environments
// Lane l = 16 g + i holds A[i][g] and B[g][i], and after the instruction D[4 g + r][i] in register r = 0..3 (checked against a host
// product: tools/microbench/mfma_f32.hip).  So lane l holds, of output tile t, the units 16 t + 4 g + r of environment i: and since a
// sum over k has no order, the next layer takes register r of tile t as the B operand of its k-block 4 t + r as it stands, provided
// its weights were packed with that k-block being the units {16 t + 4 g + r : g = 0..3}.  No activation ever leaves the registers; the
// kernel uses no LDS and no barrier.
//
// ---- Operand staging.  The weights are read as A operands straight from global memory: one coalesced 256-byte load per instruction,
// at an address that depends on nothing computed, so the loads run ahead of the matrix instructions.  The blob of a [64, 64] policy is
// about 50 KB and of a [256, 256] one about 620 KB: both stay in L2 (4 MiB per XCD), the first in L1 as well.  One code path serves
// all widths; the kernel is instantiated for trunks of at most 64 units (4 tiles of registers per layer) and of at most 256 (16).
//
// ---- The blob (float32; mycobotgym_amd/policy.py: pack / unpack restate it).  In this order: the policy net's layers, its head
// (action_net, A rows padded with zeros to 16), the value net's layers, its head (value_net, 1 row padded to 16), log_std padded to
// 16.  A layer of `out` units (a multiple of 16; a head: 16) over `nkb` k-blocks is out / 16 * nkb tiles of 64 floats, then its bias,
// `out` floats:
//     tile (T, kb), float l = 16 g + i:   W[16 T + i][k(kb, g)]
//     first layer   nkb = ceil((D + 6) / 4),  k(kb, g) = 4 kb + g: column of [achieved_goal(3), desired_goal(3), observation(D)], the
//                   sorted key order of SB3's CombinedExtractor; columns from D + 6 on are zeros
//     later layers  nkb = in / 4,             k(4 t + r, g) = 16 t + 4 g + r
// Every piece is a multiple of 16 floats, so with a 16-byte aligned blob every bias row of 4 is one aligned 16-byte load.
//
// ---- The noise: the counter layout of gauss4 (mcg_policy.hpp).  Philox4x32-10 (mcg_philox.hpp), key = seed, counter
//     ((uint32)gid, (uint32)call, pair ^ ((uint32)(call >> 32) << 8), DOMAIN_POLICY ^ ((uint32)(gid >> 32) << 8))
// gid = env_id_offset + i the global environment id, `call` the caller's count of sampling calls, pair = 0 .. ceil(A / 2) - 1.  The low
// byte of the last word is the domain (enum Domain, mcg_philox.hpp: the one list).  One block is two uniforms u0, u1 of 53 bits
// (philox_pair) and serves two action components by Box-Muller, evaluated in double and rounded to float32 once:
//     eps[2 pair] = sqrt(-2 ln(1 - u0)) cos(2 pi u1),   eps[2 pair + 1] = sqrt(-2 ln(1 - u0)) sin(2 pi u1)
// An environment's draws depend on (seed, gid, call) alone: not on the tile it falls into, nor on how many ranks share the job.
#include "mcg_policy.hpp"       // plan, Net, Pol, mfma, activate, first_layer, dense, pick: shared with mcg_policy_grad.hip

using namespace mcg;

namespace {

struct Out { float *action, *value, *log_prob, *mean, *noise; };

// MT: tiles of 16 units that a trunk layer may have (the host picks 4 or 16 by the widest layer).
template <int MT>
__global__ __launch_bounds__(WAVE) void policy_kernel(Pol P, const double* __restrict__ obs, const double* __restrict__ ach,
                                                      const double* __restrict__ des, unsigned long long seed, unsigned long long call,
                                                      long long env_id_offset, int deterministic, Out O) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < P.N;
  const int env = live ? e : P.N - 1;    // a ragged tile's extra rows read a valid row and store nothing
  const int k = blockIdx.y;              // 0: the value net; 1: the policy net (grid.y == 1: mcg_policy_forward's value-only call)
  if (k == 0 && !O.value) return;        // (the value is not asked for)
  const Net net = pick(P.net[0], P.net[1], k);
  f4 a[MT], b[MT];
  first_layer<MT, double>(P, net, obs, ach, des, env, g, lane, a);
#pragma unroll
  for (int t = 0; t < MT; t++)
#pragma unroll
    for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, a[t][r]);
  for (int L = 1; L < net.n; L++) {
    dense<MT, MT>(P, net, L, L == 1 ? net.nt[0] : net.nt[1], L == 1 ? net.nt[1] : net.nt[2], a, b, g, lane);
#pragma unroll
    for (int t = 0; t < MT; t++)
#pragma unroll
      for (int r = 0; r < 4; r++) a[t][r] = activate(P.act, b[t][r]);
  }
  f4 head[1];
  dense<MT, 1>(P, net, net.n, net.n == 1 ? net.nt[0] : net.n == 2 ? net.nt[1] : net.nt[2], 1, a, head, g, lane);
  const f4 h = head[0];                  // lane 16 g + i: rows 4 g + r of the head, environment i
  if (k == 0) {
    if (O.value && live && g == 0) O.value[e] = h[0];
    return;
  }
  // ---- the diagonal Gaussian (mcg_policy.hpp): this lane has components 4 g .. 4 g + 3
  const f4 ls = *reinterpret_cast<const f4*>(P.blob + P.log_std + 4 * g);
  const Sampled d = gauss_sample(P.A, h, ls, g, seed, (unsigned long long)(env_id_offset + env), call, DOMAIN_POLICY, deterministic);
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < P.A && live) {
      const size_t at = (size_t)e * P.A + c;
      if (O.action) O.action[at] = d.action[r];
      if (O.mean) O.mean[at] = d.mean[r];
      if (O.noise) O.noise[at] = d.noise[r];
    }
  }
  if (O.log_prob && live && g == 0) O.log_prob[e] = d.log_prob;
}

}  // namespace

extern "C" {

int64_t mcg_policy_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_vf, const int32_t* vf_width) {
  const char* why;
  return plan(obs_dim, act_dim, n_pi, pi_width, n_vf, vf_width, nullptr, &why);
}

int mcg_policy_forward(const mcg_policy* pol, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset,
                       int deterministic, const mcg_policy_out* out, void* stream) {
  const char* who = "mcg_policy_forward";
  if (!pol) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy", who);
  if (!pol->blob) return mcg_fail(MCG_ERR_ARG, "%s: blob is null", who);
  if (pol->n_envs < 1) return mcg_fail(MCG_ERR_ARG, "%s: n_envs must be >= 1", who);
  if ((long long)pol->n_envs * MAX_ACT >= (1ll << 31)) return mcg_fail(MCG_ERR_ARG, "%s: n_envs must be below 2^27", who);
  Pol P = {};
  const char* why = nullptr;
  const int64_t floats = plan(pol->obs_dim, pol->act_dim, pol->n_pi, pol->pi_width, pol->n_vf, pol->vf_width, &P, &why);
  if (floats == 0) return mcg_fail(MCG_ERR_ARG, "%s: %s", who, why);
  if (pol->activation != MCG_POLICY_TANH && pol->activation != MCG_POLICY_RELU)
    return mcg_fail(MCG_ERR_ARG, "%s: activation must be MCG_POLICY_TANH or MCG_POLICY_RELU", who);
  if (pol->blob_floats != floats)
    return mcg_fail(MCG_ERR_ARG, "%s: blob_floats is %lld, mcg_policy_blob_floats gives %lld for this shape", who, (long long)pol->blob_floats,
                    (long long)floats);
  if (((uintptr_t)pol->blob & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: blob is not 16-byte aligned", who);
  if (!obs) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_step_out", who);
  if (!obs->obs || !obs->achieved_goal || !obs->desired_goal)
    return mcg_fail(MCG_ERR_ARG, "%s: obs, achieved_goal and desired_goal of the observation are required", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_policy_out", who);
  if (!out->action && !out->value && !out->log_prob && !out->mean && !out->noise)
    return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  P.blob = pol->blob; P.N = pol->n_envs; P.act = pol->activation;
  const int nets = (out->action || out->log_prob || out->mean || out->noise) ? 2 : 1;      // value alone: the policy net is not evaluated
  const Out O = {out->action, out->value, out->log_prob, out->mean, out->noise};
  const int widest = widest_layer(pol);
  const dim3 grid(blocks(P.N, TILE), nets), block(WAVE);
#define MCG_POLICY(MT) hipLaunchKernelGGL(policy_kernel<MT>, grid, block, 0, (hipStream_t)stream, P, obs->obs, obs->achieved_goal, \
                                          obs->desired_goal, (unsigned long long)seed, (unsigned long long)call, (long long)env_id_offset, \
                                          deterministic != 0, O)
  if (widest <= 64) MCG_POLICY(4);
  else MCG_POLICY(16);
#undef MCG_POLICY
  return launched("mcg_policy");
}

}  // extern "C"
