// mcg_td3.hip -- the gradient-free half of TD3 and DDPG (include/mcg.h: mcg_td3_*): SB3's TD3Policy for a Dict space of Boxes -- a
// deterministic actor with a target copy and one or two critics with a target copy -- as the collection action (mcg_td3_act), the
// critics' forward (mcg_td3_q), the smoothed TD target of a replay batch (mcg_td3_target) and the Polyak step of both target pairs
// (mcg_td3_polyak).  DDPG is n_critics = 1 with sigma = 0.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  The matrix instruction, its operand map
// and the layer helpers are mcg_policy.hpp's; the critic's forward, the critics' kernel (q_kernel), the Polyak kernel, the Gaussian draw
// and the blobs' plan are mcg_sac.hpp's, instantiated here a second time; the action-as-operand rule and the critic's layout are
// stated at mcg_sac.hip's head.  Here: TD3's own kernels (the action, the smoothed target) and the C entries.  The C side is stateless
// and no entry synchronises.
//
// ---- Work split.  mcg_td3_act: one wave per tile of 16 environments.  mcg_td3_q: one wave per (tile of 16 rows, critic), grid.y =
// n_critics.  mcg_td3_target: one workgroup of n_critics waves per tile of 16 samples; each wave evaluates actor_target on the next
// observation -- the same instructions on the same inputs, so the same bits -- adds the clipped noise and clamps while the action is
// in its registers, and then runs target critic `wave` on it; the Q rows meet through LDS and one barrier, and wave 0 forms and stores
// everything.  mcg_td3_polyak: one lane per four floats of a blob, one launch per pair.
//
// ---- The blobs (float32, 16-byte aligned; mycobotgym_amd/_offpolicy.py: pack_net / unpack_net restate them), tiles and biases as in
// mcg_sac.hip's head.
//   actor, actor_target    the trunk's layers, then the one head (A rows, the rest zeros) over H / 4 k-blocks and 16 biases.
//   critic, critic_target  qf0 alone (n_critics = 1) or qf0 then qf1, each in mcg_sac.hip's critic layout.
//
// ---- The noise.  mcg_policy.hpp's gauss4 (Philox4x32-10, Box-Muller in double: the draw of mcg_sac_act), with the domain byte DOMAIN_TD3_ACT
// for mcg_td3_act, id = the global environment id, and DOMAIN_TD3_TARGET for mcg_td3_target, id = the sample's index in the batch.  Scaled in float32:
// __fmul_rn(sigma, eps).  sigma == 0: the noise is +0 and no block is computed.
#include "mcg_td3.hpp"          // checked_td3, scaled_noise, td3_actor, add_clamped; mcg_sac.hpp (q_kernel, polyak_kernel, blob_plan), mcg_policy.hpp

using namespace mcg;

namespace {

struct ActOut { float *action, *mean, *noise; };
struct TargetOut { float *target, *next_action, *next_q, *noise; };

template <int MT>
__global__ __launch_bounds__(WAVE) void td3_act_kernel(Sac S, const double* __restrict__ obs, const double* __restrict__ ach,
                                                       const double* __restrict__ des, unsigned long long seed, unsigned long long call,
                                                       long long env_id_offset, float noise_std, ActOut O) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < S.pi.N;
  const int env = live ? e : S.pi.N - 1;   // a ragged tile's extra rows read a valid row and store nothing
  const f4 mean = td3_actor<MT, double>(S.pi, obs, ach, des, env, g, lane);
  const f4 n = scaled_noise(S.pi.A, g, noise_std, seed, (unsigned long long)(env_id_offset + env), call, DOMAIN_TD3_ACT);
  const f4 a = add_clamped(mean, n);
  if (!live) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < S.pi.A) {
      const size_t at = (size_t)e * S.pi.A + c;
      O.action[at] = a[r];
      if (O.mean) O.mean[at] = mean[r];
      if (O.noise) O.noise[at] = n[r];
    }
  }
}

// blockDim.x = 64 n_critics
template <int MT>
__global__ __launch_bounds__(2 * WAVE) void td3_target_kernel(Sac S, Batch X, int B, int n_critics, unsigned long long seed,
                                                              unsigned long long call, float gamma, float sigma, float clip, TargetOut O) {
  __shared__ float qs[2][TILE];
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int lane = threadIdx.x & 63, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < B;
  const int row = live ? e : B - 1;
  const f4 mean = td3_actor<MT, float>(S.pi, X.next_obs, X.next_achieved, X.desired, row, g, lane);
  f4 n = scaled_noise(S.pi.A, g, sigma, seed, (unsigned long long)row, call, DOMAIN_TD3_TARGET);
  if (sigma != 0.0f) {
#pragma unroll
    for (int r = 0; r < 4; r++) n[r] = fminf(fmaxf(n[r], -clip), clip);
  }
  const f4 a = add_clamped(mean, n);
  const float v = critic<MT, float>(S, wave, X.next_obs, X.next_achieved, X.desired, row, a, g, lane);
  if (g == 0) qs[wave][i] = v;
  __syncthreads();
  if (wave != 0 || !live) return;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    if (c < S.pi.A) {
      const size_t at = (size_t)e * S.pi.A + c;
      if (O.next_action) O.next_action[at] = a[r];
      if (O.noise) O.noise[at] = n[r];
    }
  }
  if (g != 0) return;
  const float q0 = qs[0][i], q1 = n_critics == 2 ? qs[1][i] : q0;
  O.target[e] = fmaf(__fmul_rn(1.0f - X.done[e], gamma), fminf(q0, q1), X.reward[e]);
  if (O.next_q) {
    O.next_q[e] = q0;
    if (n_critics == 2) O.next_q[(size_t)B + e] = q1;
  }
}

}  // namespace

// ------------------------------------------------------------------------------------------------------- host side (the plan and the checks: mcg_td3.hpp)

extern "C" {

int64_t mcg_td3_blob_floats(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int n_critics,
                            int64_t* actor_floats, int64_t* critic_floats) {
  const char* why;
  if (actor_floats) *actor_floats = 0;
  if (critic_floats) *critic_floats = 0;
  return blob_plan(obs_dim, act_dim, n_pi, pi_width, n_qf, qf_width, n_critics, false, nullptr, actor_floats, critic_floats, &why);
}

int mcg_td3_act(const mcg_td3* td3, const mcg_step_out* obs, uint64_t seed, uint64_t call, int64_t env_id_offset, float noise_std,
                const mcg_td3_act_out* out, void* stream) {
  const char* who = "mcg_td3_act";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_ACTOR, &S)) return MCG_ERR_ARG;
  if (!checked_envs(who, td3->n_envs) || !checked_obs(who, obs)) return MCG_ERR_ARG;
  if (!finite_nonneg(noise_std)) return mcg_fail(MCG_ERR_ARG, "%s: noise_std must be finite and >= 0", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_td3_act_out", who);
  if (!out->action) return mcg_fail(MCG_ERR_ARG, "%s: action is required", who);
  S.pi.blob = td3->actor;
  S.pi.N = td3->n_envs;
  const ActOut O = {out->action, out->mean, out->noise};
  const dim3 grid(blocks(S.pi.N, TILE)), block(WAVE);
#define MCG_TD3_ACT(MT) hipLaunchKernelGGL(td3_act_kernel<MT>, grid, block, 0, (hipStream_t)stream, S, obs->obs, obs->achieved_goal, \
                                           obs->desired_goal, (unsigned long long)seed, (unsigned long long)call, (long long)env_id_offset, \
                                           noise_std, O)
  if (widest(td3, true, false) <= 64) MCG_TD3_ACT(4);
  else MCG_TD3_ACT(16);
#undef MCG_TD3_ACT
  return launched(who);
}

int mcg_td3_q(const mcg_td3* td3, int which, const mcg_sac_rows* rows, int64_t B, float* q, void* stream) {
  const char* who = "mcg_td3_q";
  if (which != MCG_TD3_CRITIC && which != MCG_TD3_CRITIC_TARGET)
    return mcg_fail(MCG_ERR_ARG, "%s: which must be MCG_TD3_CRITIC or MCG_TD3_CRITIC_TARGET", who);
  Sac S = {};
  if (!checked_td3(who, td3, which == MCG_TD3_CRITIC ? TD3_CRITIC : TD3_CRITIC_TARGET, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_rows_arg(who, rows, true)) return MCG_ERR_ARG;
  if (!q) return mcg_fail(MCG_ERR_ARG, "%s: q is null", who);
  set_critics(S, td3, which == MCG_TD3_CRITIC ? td3->critic : td3->critic_target);
  const Rows R = {rows->obs, rows->achieved, rows->desired, rows->action};
  const dim3 grid(blocks(B, TILE), td3->n_critics), block(WAVE);
  if (widest(td3, false, true) <= 64) hipLaunchKernelGGL(q_kernel<4>, grid, block, 0, (hipStream_t)stream, S, R, (int)B, q);
  else hipLaunchKernelGGL(q_kernel<16>, grid, block, 0, (hipStream_t)stream, S, R, (int)B, q);
  return launched(who);
}

int mcg_td3_target(const mcg_td3* td3, const mcg_her_batch* batch, int64_t B, uint64_t seed, uint64_t call, float gamma, float sigma,
                   float clip, const mcg_td3_target_out* out, void* stream) {
  const char* who = "mcg_td3_target";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_ACTOR_TARGET | TD3_CRITIC_TARGET, &S)) return MCG_ERR_ARG;
  if (!checked_rows(who, B) || !checked_batch(who, batch)) return MCG_ERR_ARG;
  if (!(gamma >= 0.0f && gamma <= 1.0f)) return mcg_fail(MCG_ERR_ARG, "%s: gamma must be in [0, 1]", who);
  if (!finite_nonneg(sigma)) return mcg_fail(MCG_ERR_ARG, "%s: sigma must be finite and >= 0", who);
  if (!finite_nonneg(clip)) return mcg_fail(MCG_ERR_ARG, "%s: clip must be finite and >= 0", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_td3_target_out", who);
  if (!out->target) return mcg_fail(MCG_ERR_ARG, "%s: target is required", who);
  S.pi.blob = td3->actor_target;
  set_critics(S, td3, td3->critic_target);
  const Batch X = {batch->next_obs, batch->next_achieved, batch->desired, batch->reward, batch->done};
  const TargetOut O = {out->target, out->next_action, out->next_q, out->noise};
  const dim3 grid(blocks(B, TILE)), block(td3->n_critics * WAVE);
#define MCG_TD3_TARGET(MT) hipLaunchKernelGGL(td3_target_kernel<MT>, grid, block, 0, (hipStream_t)stream, S, X, (int)B, (int)td3->n_critics, \
                                              (unsigned long long)seed, (unsigned long long)call, gamma, sigma, clip, O)
  if (widest(td3, true, true) <= 64) MCG_TD3_TARGET(4);
  else MCG_TD3_TARGET(16);
#undef MCG_TD3_TARGET
  return launched(who);
}

int mcg_td3_polyak(const mcg_td3* td3, double tau, void* stream) {
  const char* who = "mcg_td3_polyak";
  Sac S = {};
  if (!checked_td3(who, td3, TD3_ACTOR | TD3_ACTOR_TARGET | TD3_CRITIC | TD3_CRITIC_TARGET, &S)) return MCG_ERR_ARG;
  if (!(tau >= 0.0 && tau <= 1.0)) return mcg_fail(MCG_ERR_ARG, "%s: tau must be in [0, 1]", who);
  if (td3->critic == td3->critic_target) return mcg_fail(MCG_ERR_ARG, "%s: critic and critic_target are the same blob", who);
  if (td3->actor == td3->actor_target) return mcg_fail(MCG_ERR_ARG, "%s: actor and actor_target are the same blob", who);
  const int cq = (int)(td3->critic_floats / 4), aq = (int)(td3->actor_floats / 4);      // every piece of a blob is a multiple of 16 floats
  hipLaunchKernelGGL(polyak_kernel<256>, dim3(blocks(cq, 256)), dim3(256), 0, (hipStream_t)stream, td3->critic, td3->critic_target, cq, tau, 1.0 - tau);
  hipLaunchKernelGGL(polyak_kernel<256>, dim3(blocks(aq, 256)), dim3(256), 0, (hipStream_t)stream, td3->actor, td3->actor_target, aq, tau, 1.0 - tau);
  return launched(who);
}

}  // extern "C"
