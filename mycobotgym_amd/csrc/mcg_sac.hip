// mcg_sac.hip -- the gradient-free half of SAC (include/mcg.h: mcg_sac_*): SB3's SACPolicy for a Dict space of Boxes -- a squashed
// Gaussian actor with a state-dependent log_std and twin critics with a target copy -- as the collection action (mcg_sac_act), the
// twin-critic forward (mcg_sac_q), the fused TD target of a replay batch (mcg_sac_target) and the Polyak step (mcg_sac_polyak).
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  The C entries and SAC's own kernels (the
// action, the TD target) are here; the critic's forward, the critics' kernel (q_kernel) and the Polyak kernel are mcg_sac.hpp's, which
// TD3 / DDPG (mcg_td3.hip) instantiates too; the matrix instruction, its operand map and the layer helpers are mcg_policy.hpp's,
// unchanged, and mcg_policy.hip's head states them.  The C side is stateless and no entry synchronises.
//
// ---- Work split.  mcg_sac_act: one wave per tile of 16 environments.  mcg_sac_q: one wave per (tile of 16 rows, critic), grid.y = 2.
// mcg_sac_target: one workgroup of two waves per tile of 16 samples; wave q evaluates the actor on the next observation -- both waves
// the same instructions on the same inputs, so the same bits -- and then target critic q with the action it holds in registers; the
// two Q rows meet through 2 x 16 floats of LDS and one barrier, and wave 0 forms and stores everything.  mcg_sac_polyak: one lane per
// four floats of the blob.
//
// ---- The action as a matrix operand.  After the actor's head lane 16 g + i holds, in register r, component 4 g + r of sample i: the
// accumulator layout, which is the B operand of a later layer's k-block r (mcg_policy.hip's head).  So the critics' first layer keeps
// its action columns as four k-blocks in the later-layer order and takes the action where it lies; an action that comes from memory
// (mcg_sac_q) is loaded into the same registers (load_action), lane (g, i) reading components 4 g .. 4 g + 3 of row i, those >= A as zeros.
//
// ---- The blobs (float32, 16-byte aligned; mycobotgym_amd/_offpolicy.py: pack_net / unpack_net restate them).  Tiles and biases as in
// mcg_policy.hip's head: tile (T, kb), float l = 16 g + i: W[16 T + i][k(kb, g)].
//   actor    latent_pi's layers (the first over the D + 6 feature columns, k(kb, g) = 4 kb + g; later ones k(4 t + r, g) = 16 t + 4 g + r),
//            then the head mu and the head log_std: each one tile row of 16 (A rows, the rest zeros) over H / 4 k-blocks and 16 biases.
//   critic   qf0 then qf1.  A first layer of `out` units is out / 16 * ceil((D + 6) / 4) tiles over the feature columns (k(kb, g) =
//            4 kb + g), then out / 16 * 4 tiles over the action padded with zero columns to 16 (k(r, g) = 4 g + r), then `out` biases;
//            the later layers; a head of one row padded to 16.
//   critic_target   the critic's layout.
//
// ---- The noise.  Philox4x32-10, mcg_policy.hip's counter layout with the domain byte DOMAIN_SAC_ACT for mcg_sac_act, id = the global
// environment id, and DOMAIN_SAC_TARGET for mcg_sac_target, id = the sample's index in the batch (the bytes' list: enum Domain,
// mcg_philox.hpp).  One block serves two components by Box-Muller in double, as there: gauss4 (mcg_policy.hpp) is the one place that
// forms the counter words, for every policy's draws.
#include "mcg_sac.hpp"          // Sac, Rows, Batch, Draw, hidden, squash, critic, q_kernel, polyak_kernel, blob_plan, the host checks (shared
                                // with mcg_sac_grad.hip and, through mcg_td3.hpp, with TD3 / DDPG); mcg_policy.hpp

using namespace mcg;

namespace {

struct ActOut { float *action, *log_prob, *mean, *log_std, *noise; };
struct TargetOut { float *target, *next_action, *next_log_prob, *next_q, *noise; };

// SB3's actor.action_log_prob on one row (include/mcg.h states every rounding).  `id`, `call`, `stream`: the noise's counter.
template <int MT, class In>
MCG_DEV Draw actor(const Pol& P, const In* __restrict__ obs, const In* __restrict__ ach, const In* __restrict__ des, int row, int g, int lane,
                   unsigned long long seed, unsigned long long id, unsigned long long call, uint32_t stream, bool deterministic) {
  f4 a[MT], mu[1], ls[1];
  first_layer<MT, In>(P, P.net[1], obs, ach, des, row, g, lane, a);
  hidden<MT>(P, P.net[1], a, g, lane);
  dense<MT, 1>(P, P.net[1], P.net[1].n, last_tiles(P.net[1]), 1, a, mu, g, lane);
  dense<MT, 1>(P, P.net[0], P.net[0].n, last_tiles(P.net[0]), 1, a, ls, g, lane);
  return squash(P.A, mu[0], ls[0], g, seed, id, call, stream, deterministic);
}

template <int MT>
__global__ __launch_bounds__(WAVE) void sac_act_kernel(Sac S, const double* __restrict__ obs, const double* __restrict__ ach,
                                                       const double* __restrict__ des, unsigned long long seed, unsigned long long call,
                                                       long long env_id_offset, int deterministic, ActOut O) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < S.pi.N;
  const int env = live ? e : S.pi.N - 1;   // a ragged tile's extra rows read a valid row and store nothing
  const Draw d = actor<MT, double>(S.pi, obs, ach, des, env, g, lane, seed, (unsigned long long)(env_id_offset + env), call, DOMAIN_SAC_ACT,
                                   deterministic != 0);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < S.pi.A) {
      const size_t at = (size_t)e * S.pi.A + c;
      O.action[at] = d.action[r];
      if (O.mean) O.mean[at] = d.mean[r];
      if (O.log_std) O.log_std[at] = d.log_std[r];
      if (O.noise) O.noise[at] = d.noise[r];
    }
  }
  if (O.log_prob && g == 0) O.log_prob[e] = d.log_prob;
}

template <int MT>
__global__ __launch_bounds__(2 * WAVE) void sac_target_kernel(Sac S, Batch X, int B, unsigned long long seed, unsigned long long call, float gamma,
                                                              float ent_coef, const float* __restrict__ log_ent_coef, TargetOut O) {
  __shared__ float qs[2][TILE];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < B;
  const int row = live ? e : B - 1;
  const Draw d = actor<MT, float>(S.pi, X.next_obs, X.next_achieved, X.desired, row, g, lane, seed, (unsigned long long)row, call,
                                  DOMAIN_SAC_TARGET, false);
  const float v = critic<MT, float>(S, wave, X.next_obs, X.next_achieved, X.desired, row, d.action, g, lane);
  if (g == 0) qs[wave][i] = v;
  __syncthreads();
  if (wave != 0 || !live) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < S.pi.A) {
      const size_t at = (size_t)e * S.pi.A + c;
      if (O.next_action) O.next_action[at] = d.action[r];
      if (O.noise) O.noise[at] = d.noise[r];
    }
  }
  if (g != 0) return;
  const float q0 = qs[0][i], q1 = qs[1][i];
  const float alpha = log_ent_coef ? (float)exp((double)*log_ent_coef) : ent_coef;
  const float next_q = fmaf(-alpha, d.log_prob, fminf(q0, q1));
  O.target[e] = fmaf(__fmul_rn(1.0f - X.done[e], gamma), next_q, X.reward[e]);
  if (O.next_log_prob) O.next_log_prob[e] = d.log_prob;
  if (O.next_q) { O.next_q[e] = q0; O.next_q[(size_t)B + e] = q1; }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------- host side (the plan and the checks: mcg_sac.hpp)

extern "C" {

int64_t mcg_sac_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int64_t* actor_floats,
                            int64_t* critic_floats) {
  const char* why;
  if (actor_floats) *actor_floats = 0;
  if (critic_floats) *critic_floats = 0;
  return blob_plan(obs_dim, act_dim, n_pi, pi_width, n_qf, qf_width, 2, true, nullptr, actor_floats, critic_floats, &why);
}

int mcg_sac_act(const mcg_sac* sac, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset, int deterministic,
                const mcg_sac_act_out* out, void* stream) {
  const char* who = "mcg_sac_act";
  Sac S = {};
  if (!checked_sac(who, sac, NEED_ACTOR, &S)) return MCG_ERR_ARG;
  if (!checked_envs(who, sac->n_envs) || !checked_obs(who, obs)) return MCG_ERR_ARG;
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac_act_out", who);
  if (!out->action) return mcg_fail(MCG_ERR_ARG, "%s: action is required", who);
  S.pi.N = sac->n_envs;
  const ActOut O = {out->action, out->log_prob, out->mean, out->log_std, out->noise};
  const dim3 grid(blocks(S.pi.N, TILE)), block(WAVE);
#define MCG_SAC_ACT(MT) hipLaunchKernelGGL(sac_act_kernel<MT>, grid, block, 0, (hipStream_t)stream, S, obs->obs, obs->achieved_goal, \
                                           obs->desired_goal, (unsigned long long)seed, (unsigned long long)call, (long long)env_id_offset, \
                                           deterministic != 0, O)
  if (widest(sac, true, false) <= 64) MCG_SAC_ACT(4);
  else MCG_SAC_ACT(16);
#undef MCG_SAC_ACT
  return launched("mcg_sac_act");
}

int mcg_sac_q(const mcg_sac* sac, int which, const mcg_sac_rows* rows, int64_t B, float* q, void* stream) {
  const char* who = "mcg_sac_q";
  if (which != MCG_SAC_CRITIC && which != MCG_SAC_CRITIC_TARGET)
    return mcg_fail(MCG_ERR_ARG, "%s: which must be MCG_SAC_CRITIC or MCG_SAC_CRITIC_TARGET", who);
  Sac S = {};
  if (!checked_sac(who, sac, which == MCG_SAC_CRITIC ? NEED_CRITIC : NEED_TARGET, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, true)) return MCG_ERR_ARG;
  if (!q) return mcg_fail(MCG_ERR_ARG, "%s: q is null", who);
  S.qf[0].blob = which == MCG_SAC_CRITIC ? sac->critic : sac->critic_target;
  S.qf[1].blob = S.qf[0].blob + sac->critic_floats / 2;
  const Rows R = {rows->obs, rows->achieved, rows->desired, rows->action};
  const dim3 grid(blocks(B, TILE), 2), block(WAVE);
  if (widest(sac, false, true) <= 64) hipLaunchKernelGGL(q_kernel<4>, grid, block, 0, (hipStream_t)stream, S, R, (int)B, q);
  else hipLaunchKernelGGL(q_kernel<16>, grid, block, 0, (hipStream_t)stream, S, R, (int)B, q);
  return launched("mcg_sac_q");
}

int mcg_sac_target(const mcg_sac* sac, const mcg_her_batch* batch, int64_t B, uint64_t seed, uint64_t call, float gamma, float ent_coef,
                   const float* log_ent_coef, const mcg_sac_target_out* out, void* stream) {
  const char* who = "mcg_sac_target";
  Sac S = {};
  if (!checked_sac(who, sac, NEED_ACTOR | NEED_TARGET, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_batch(who, batch)) return MCG_ERR_ARG;
  if (!(gamma >= 0.0f && gamma <= 1.0f)) return mcg_fail(MCG_ERR_ARG, "%s: gamma must be in [0, 1]", who);
  if (!log_ent_coef && !(ent_coef >= 0.0f && ent_coef <= 3.0e38f))
    return mcg_fail(MCG_ERR_ARG, "%s: ent_coef must be finite and >= 0 where log_ent_coef is null", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac_target_out", who);
  if (!out->target) return mcg_fail(MCG_ERR_ARG, "%s: target is required", who);
  S.qf[0].blob = sac->critic_target;
  S.qf[1].blob = S.qf[0].blob + sac->critic_floats / 2;
  const Batch X = {batch->next_obs, batch->next_achieved, batch->desired, batch->reward, batch->done};
  const TargetOut O = {out->target, out->next_action, out->next_log_prob, out->next_q, out->noise};
  const dim3 grid(blocks(B, TILE)), block(2 * WAVE);
#define MCG_SAC_TARGET(MT) hipLaunchKernelGGL(sac_target_kernel<MT>, grid, block, 0, (hipStream_t)stream, S, X, (int)B, (unsigned long long)seed, \
                                              (unsigned long long)call, gamma, ent_coef, log_ent_coef, O)
  if (widest(sac, true, true) <= 64) MCG_SAC_TARGET(4);
  else MCG_SAC_TARGET(16);
#undef MCG_SAC_TARGET
  return launched("mcg_sac_target");
}

int mcg_sac_polyak(const mcg_sac* sac, double tau, void* stream) {
  const char* who = "mcg_sac_polyak";
  Sac S = {};
  if (!checked_sac(who, sac, NEED_CRITIC | NEED_TARGET, &S)) return MCG_ERR_ARG;
  if (!(tau >= 0.0 && tau <= 1.0)) return mcg_fail(MCG_ERR_ARG, "%s: tau must be in [0, 1]", who);
  if (sac->critic == sac->critic_target) return mcg_fail(MCG_ERR_ARG, "%s: critic and critic_target are the same blob", who);
  const int quads = (int)(sac->critic_floats / 4);      // every piece of a blob is a multiple of 16 floats
  hipLaunchKernelGGL(polyak_kernel<256>, dim3(blocks(quads, 256)), dim3(256), 0, (hipStream_t)stream, sac->critic, sac->critic_target, quads, tau,
                     1.0 - tau);
  return launched("mcg_sac_polyak");
}

}  // extern "C"
