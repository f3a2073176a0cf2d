// mcg_td3.hpp -- what mcg_td3.hip (the gradient-free half of TD3 / DDPG) and mcg_td3_grad.hip (the update) share: the blobs' plan and
// the host checks of an mcg_td3, the scaled noise, and the deterministic actor's output.  The kernels' view of the blobs is
// mcg_sac.hpp's `Sac` -- pi: the actor (or its target) with the one head as net[1]; qf[k]: critic k -- because the layouts are
// mcg_sac.hip's but for the missing log_std head and the number of critics (mcg_td3.hip's head).
#pragma once

#include "mcg_sac.hpp"          // Sac, hidden, last_tiles, sac_plan, checked_rows; mcg_policy.hpp

namespace {

constexpr uint32_t TD3_ACT_STREAM = 10, TD3_TARGET_STREAM = 11;

// sigma eps of a lane's four components (zeros from A on): eps as mcg_sac.hpp's squash draws it, each product rounded to float32
// once.  sigma == 0: +0 and no Philox block.
MCG_DEV f4 scaled_noise(int A, int g, float sigma, unsigned long long seed, unsigned long long id, unsigned long long call, uint32_t stream) {
  f4 n = {0.0f, 0.0f, 0.0f, 0.0f};
  if (sigma == 0.0f) return n;
#pragma unroll
  for (int q = 0; q < 2; q++) {
    if (4 * g + 2 * q < A) {
      double u0, u1, s, c;
      const uint32_t pair = (uint32_t)(2 * g + q);
      mcg::philox_pair((uint32_t)id, (uint32_t)call, pair ^ ((uint32_t)(call >> 32) << 8), stream ^ ((uint32_t)(id >> 32) << 8), seed, u0, u1);
      const double rad = sqrt(-2.0 * log(1.0 - u0));
      sincos(6.283185307179586476925 * u1, &s, &c);
      n[2 * q] = __fmul_rn(sigma, (float)(rad * c));
      if (4 * g + 2 * q + 1 < A) n[2 * q + 1] = __fmul_rn(sigma, (float)(rad * s));
    }
  }
  return n;
}

// the head's sums z -> the actor's output (float)tanh((double)z), zeros from A on
MCG_DEV f4 tanh_head(int A, const f4& z, int g) {
  f4 a;
#pragma unroll
  for (int r = 0; r < 4; r++) a[r] = 4 * g + r < A ? (float)tanh((double)z[r]) : 0.0f;
  return a;
}

// SB3's actor.mu on one row -> tanh of the head, in the accumulator layout
template <int MT, class In>
MCG_DEV f4 td3_actor(const Pol& P, const In* __restrict__ obs, const In* __restrict__ ach, const In* __restrict__ des, int row, int g, int lane) {
  f4 a[MT], z[1];
  first_layer<MT, In>(P, P.net[1], obs, ach, des, row, g, lane, a);
  hidden<MT>(P, P.net[1], a, g, lane);
  dense<MT, 1>(P, P.net[1], P.net[1].n, last_tiles(P.net[1]), 1, a, z, g, lane);
  return tanh_head(P.A, z[0], g);
}

// clamp(a + n, -1, 1) per component: the sum rounded to float32 once; zeros from A on stay zeros
MCG_DEV f4 add_clamped(const f4& a, const f4& n) {
  f4 o;
#pragma unroll
  for (int r = 0; r < 4; r++) o[r] = fminf(fmaxf(__fadd_rn(a[r], n[r]), -1.0f), 1.0f);
  return o;
}

// ------------------------------------------------------------------------------------------------------- host side
// The blobs' plan -> actor_floats + critic_floats; 0 and `why` for a refused shape.  The actor is sac_plan's without the log_std head;
// the critic blob is n_critics of sac_plan's critics.
inline int64_t td3_plan(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int n_critics, Sac* S,
                        int64_t* actor_floats, int64_t* critic_floats, const char** why) {
  if (n_critics != 1 && n_critics != 2) { *why = "n_critics must be 1 or 2"; return 0; }
  int64_t actor = 0, critic = 0;
  if (sac_plan(obs_dim, act_dim, n_pi, pi_width, n_qf, qf_width, S, &actor, &critic, why) == 0) return 0;
  actor -= (int64_t)(pi_width[n_pi - 1] / 4) * WAVE + 16;      // the second head
  critic = critic / 2 * n_critics;
  if (actor_floats) *actor_floats = actor;
  if (critic_floats) *critic_floats = critic;
  return actor + critic;
}

enum { TD3_ACTOR = 1, TD3_ACTOR_TARGET = 2, TD3_CRITIC = 4, TD3_CRITIC_TARGET = 8 };

// What every entry checks of an mcg_td3 before it launches, `need` naming the blobs the entry touches -> true, and S filled but for the
// blob pointers and N; false after mcg_fail.
inline bool checked_td3(const char* who, const mcg_td3* td3, int need, Sac* S) {
  if (!td3) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_td3", who); return false; }
  const struct { int bit; const void* p; const char* name; } blobs[4] = {{TD3_ACTOR, td3->actor, "actor"}, {TD3_ACTOR_TARGET, td3->actor_target, "actor_target"},
                                                                         {TD3_CRITIC, td3->critic, "critic"}, {TD3_CRITIC_TARGET, td3->critic_target, "critic_target"}};
  for (const auto& b : blobs)
    if ((need & b.bit) && !b.p) { mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is null", who, b.name); return false; }
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (td3_plan(td3->obs_dim, td3->act_dim, td3->n_pi, td3->pi_width, td3->n_qf, td3->qf_width, td3->n_critics, S, &actor, &critic, &why) == 0) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: %s", who, why); return false; }
  if (td3->activation != MCG_POLICY_TANH && td3->activation != MCG_POLICY_RELU) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: activation must be MCG_POLICY_TANH or MCG_POLICY_RELU", who); return false; }
  if (td3->actor_floats != actor || td3->critic_floats != critic) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: actor_floats / critic_floats are %lld / %lld, mcg_td3_blob_floats gives %lld / %lld for this shape", who,
                  (long long)td3->actor_floats, (long long)td3->critic_floats, (long long)actor, (long long)critic);
    return false;
  }
  for (const auto& b : blobs)
    if ((need & b.bit) && ((uintptr_t)b.p & 15)) { mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is not 16-byte aligned", who, b.name); return false; }
  S->pi.act = S->qf[0].act = S->qf[1].act = td3->activation;
  return true;
}

// critic k of the blob at `base`: with one critic both views are qf0
inline void set_critics(Sac& S, const mcg_td3* td3, const float* base) {
  S.qf[0].blob = base;
  S.qf[1].blob = td3->n_critics == 2 ? base + td3->critic_floats / 2 : base;
}

inline int td3_widest(const mcg_td3* td3, bool pi, bool qf) {
  int w = 0;
  for (int L = 0; pi && L < td3->n_pi; L++) w = td3->pi_width[L] > w ? td3->pi_width[L] : w;
  for (int L = 0; qf && L < td3->n_qf; L++) w = td3->qf_width[L] > w ? td3->qf_width[L] : w;
  return w;
}

inline bool finite_nonneg(float x) { return x >= 0.0f && x <= 3.0e38f; }

}  // namespace
