// mcg_td3.hpp -- what mcg_td3.hip (the gradient-free half of TD3 / DDPG) and mcg_td3_grad.hip (the update) share beyond mcg_sac.hpp: the
// host checks of an mcg_td3, the scaled noise, and the deterministic actor's output.  The kernels' view of the blobs (`Sac` -- pi: the
// actor or its target with the one head as net[1]; qf[k]: critic k), the critic's forward, the critics' and the
// Polyak kernel and the blobs' plan are mcg_sac.hpp's single definitions: the layouts are mcg_sac.hip's but for the missing log_std
// head and the number of critics (mcg_td3.hip's head).
#pragma once

#include "mcg_sac.hpp"          // Sac, hidden, last_tiles, critic, blob_plan, checked_blobs, widest; mcg_policy.hpp (gauss4)

namespace {

// sigma eps of a lane's four components (zeros from A on): eps is mcg_policy.hpp's gauss4, each product rounded to float32 once.
// sigma == 0: +0 and no Philox block.
MCG_DEV f4 scaled_noise(int A, int g, float sigma, unsigned long long seed, unsigned long long id, unsigned long long call, uint32_t stream) {
  f4 n = {0.0f, 0.0f, 0.0f, 0.0f};
  if (sigma == 0.0f) return n;
  gauss4(n, A, g, seed, id, call, stream);
#pragma unroll
  for (int r = 0; r < 4; r++) n[r] = __fmul_rn(sigma, n[r]);
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
enum { TD3_ACTOR = 1, TD3_ACTOR_TARGET = 2, TD3_CRITIC = 4, TD3_CRITIC_TARGET = 8 };

// checked_blobs (mcg_sac.hpp) of an mcg_td3's four blobs, each refused by its name
inline bool checked_td3(const char* who, const mcg_td3* td3, int need, Sac* S) {
  if (!td3) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_td3", who); return false; }
  const BlobArg blobs[4] = {{TD3_ACTOR, td3->actor, "actor"}, {TD3_ACTOR_TARGET, td3->actor_target, "actor_target"},
                            {TD3_CRITIC, td3->critic, "critic"}, {TD3_CRITIC_TARGET, td3->critic_target, "critic_target"}};
  return checked_blobs(who, "mcg_td3", td3, blobs, 4, need, td3->n_critics, false, true, S);
}

// critic k of the blob at `base`: with one critic both views are qf0
inline void set_critics(Sac& S, const mcg_td3* td3, const float* base) {
  S.qf[0].blob = base;
  S.qf[1].blob = td3->n_critics == 2 ? base + td3->critic_floats / 2 : base;
}

inline bool finite_nonneg(float x) { return x >= 0.0f && x <= 3.0e38f; }

}  // namespace
