// mcg_sac.hpp -- what mcg_sac.hip (the gradient-free half of SAC) and mcg_sac_grad.hip (the update) share: the kernels' view of an
// mcg_sac, the blobs' plan, the host checks, and the actor's draw from its two heads.  The blobs' layouts, the action-as-operand rule
// and the noise are stated at mcg_sac.hip's head.
#pragma once

#include "mcg_policy.hpp"       // Net, Pol, mfma, activate, first_layer, dense

namespace {

constexpr uint32_t SAC_ACT_STREAM = 7, SAC_TARGET_STREAM = 8, SAC_ACTOR_LOSS_STREAM = 9;
constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

// mcg_sac as the kernels see it.  pi: the actor blob; net[1] is latent_pi with the head mu, net[0] the same trunk with the head
// log_std.  qf[k]: critic k of the critic or the target blob -- the same plan, net[0], from its own base, so that a kernel picks a
// critic by an address in its arguments and copies nothing; qa: the first layer's action tiles.
struct Sac { Pol pi, qf[2]; int qa; };

// What the actor gives a lane: components 4 g + r of its sample (zeros from A on), and the sample's log-prob (on all four lanes).
struct Draw { f4 action, mean, log_std, noise; float log_prob; };

MCG_DEV int last_tiles(const Net& net) { return net.n == 1 ? net.nt[0] : net.n == 2 ? net.nt[1] : net.nt[2]; }

// a: a first layer's sums -> the last hidden layer's activations
template <int MT>
MCG_DEV void hidden(const Pol& P, const Net& net, f4 (&a)[MT], int g, int lane) {
  f4 b[MT];
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
}

// The two heads' rows of a lane (mu, log_std before the clamp) -> the noise, the squashed action and the log-prob (include/mcg.h
// states every rounding).  `id`, `call`, `stream`: the noise's counter.
MCG_DEV Draw squash(int A, const f4& mu, const f4& ls, int g, unsigned long long seed, unsigned long long id, unsigned long long call,
                    uint32_t stream, bool deterministic) {
  Draw d;
  d.noise = f4{0.0f, 0.0f, 0.0f, 0.0f};
  if (!deterministic) {
#pragma unroll
    for (int q = 0; q < 2; q++) {
      if (4 * g + 2 * q < A) {
        double u0, u1, s, c;
        const uint32_t pair = (uint32_t)(2 * g + q);
        mcg::philox_pair((uint32_t)id, (uint32_t)call, pair ^ ((uint32_t)(call >> 32) << 8), stream ^ ((uint32_t)(id >> 32) << 8), seed, u0, u1);
        const double rad = sqrt(-2.0 * log(1.0 - u0));
        sincos(6.283185307179586476925 * u1, &s, &c);
        d.noise[2 * q] = (float)(rad * c);
        if (4 * g + 2 * q + 1 < A) d.noise[2 * q + 1] = (float)(rad * s);
      }
    }
  }
  double lp = 0.0;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    d.action[r] = d.mean[r] = d.log_std[r] = 0.0f;
    if (4 * g + r < A) {
      const float l = fminf(fmaxf(ls[r], LOG_STD_MIN), LOG_STD_MAX), e = d.noise[r];
      const float u = deterministic ? mu[r] : (float)((double)mu[r] + exp((double)l) * (double)e);
      const float act = (float)tanh((double)u);
      lp += (-0.5 * (double)e * (double)e - (double)l - 0.91893853320467274178) - log(1.0 - (double)act * (double)act + 1e-6);
      d.action[r] = act; d.mean[r] = mu[r]; d.log_std[r] = l;
    }
  }
  lp += __shfl_xor(lp, 16);              // the four lanes of a sample, in an order that does not depend on the tile
  lp += __shfl_xor(lp, 32);
  d.log_prob = (float)lp;
  return d;
}

// ------------------------------------------------------------------------------------------------------- host side
// The blobs' plan for a shape -> actor_floats + critic_floats; 0 and `why` for a refused shape.  S (where given): filled but for the
// blob pointers, N and act.
inline int64_t sac_plan(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, Sac* S,
                        int64_t* actor_floats, int64_t* critic_floats, const char** why) {
  if (obs_dim < 1 || act_dim < 1) { *why = "obs_dim and act_dim must be >= 1"; return 0; }
  if (obs_dim > MAX_OBS) { *why = "obs_dim must be <= 4096"; return 0; }
  if (act_dim > MAX_ACT) { *why = "act_dim must be <= 16"; return 0; }
  if (n_pi < 1 || n_pi > MAX_LAYERS) { *why = "n_pi must be in [1, 3]"; return 0; }
  if (n_qf < 1 || n_qf > MAX_LAYERS) { *why = "n_qf must be in [1, 3]"; return 0; }
  if (!pi_width || !qf_width) { *why = "null pi_width or qf_width"; return 0; }
  for (int k = 0; k < 2; k++) {
    const int n = k ? n_qf : n_pi;
    const int32_t* w = k ? qf_width : pi_width;
    for (int L = 0; L < n; L++)
      if (w[L] < 16 || w[L] > MAX_WIDTH || w[L] % 16 != 0) {
        static thread_local char msg[80];
        snprintf(msg, sizeof msg, "%s_width[%d] must be a multiple of 16 in [16, 256]", k ? "qf" : "pi", L);
        *why = msg;
        return 0;
      }
  }
  const int kb0 = (obs_dim + 6 + 3) / 4;
  // the actor: the trunk, then the two heads
  int64_t at = 0;
  Net pi = {};
  pi.n = n_pi;
  for (int L = 0; L < n_pi; L++) {
    const int out_tiles = pi_width[L] / 16, nkb = L == 0 ? kb0 : pi_width[L - 1] / 4;
    pi.nt[L] = out_tiles;
    pi.w[L] = (int)at; at += (int64_t)out_tiles * nkb * WAVE;
    pi.b[L] = (int)at; at += (int64_t)out_tiles * 16;
  }
  Net mu = pi, ls = pi;
  const int64_t head = (int64_t)(pi_width[n_pi - 1] / 4) * WAVE;
  mu.w[n_pi] = (int)at; at += head;
  mu.b[n_pi] = (int)at; at += 16;
  ls.w[n_pi] = (int)at; at += head;
  ls.b[n_pi] = (int)at; at += 16;
  const int64_t actor = at;
  // the critics
  at = 0;
  Net qf = {};
  int qa = 0;
  qf.n = n_qf;
  for (int L = 0; L <= n_qf; L++) {
    const int out_tiles = L < n_qf ? qf_width[L] / 16 : 1, nkb = L == 0 ? kb0 : qf_width[L - 1] / 4;
    if (L < n_qf) qf.nt[L] = out_tiles;
    qf.w[L] = (int)at; at += (int64_t)out_tiles * nkb * WAVE;
    if (L == 0) { qa = (int)at; at += (int64_t)out_tiles * 4 * WAVE; }
    qf.b[L] = (int)at; at += (int64_t)out_tiles * 16;
  }
  at *= 2;                               // qf1: the same plan again
  if (S) {
    S->pi.net[1] = mu; S->pi.net[0] = ls; S->qf[0].net[0] = S->qf[1].net[0] = qf; S->qa = qa;
    S->pi.kb0 = S->qf[0].kb0 = S->qf[1].kb0 = kb0; S->pi.D = S->qf[0].D = S->qf[1].D = obs_dim; S->pi.A = S->qf[0].A = S->qf[1].A = act_dim;
  }
  if (actor_floats) *actor_floats = actor;
  if (critic_floats) *critic_floats = at;
  return actor + at;                     // < 2^21 floats at the largest shape
}

enum { NEED_ACTOR = 1, NEED_CRITIC = 2, NEED_TARGET = 4 };

// What every entry checks of an mcg_sac before it launches, `need` naming the blobs the entry touches -> true, and S filled but for the
// blob pointers and N; false after mcg_fail.
inline bool checked_sac(const char* who, const mcg_sac* sac, int need, Sac* S) {
  if (!sac) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac", who); return false; }
  if ((need & NEED_ACTOR) && !sac->actor) { mcg::mcg_fail(MCG_ERR_ARG, "%s: actor is null", who); return false; }
  if ((need & NEED_CRITIC) && !sac->critic) { mcg::mcg_fail(MCG_ERR_ARG, "%s: critic is null", who); return false; }
  if ((need & NEED_TARGET) && !sac->critic_target) { mcg::mcg_fail(MCG_ERR_ARG, "%s: critic_target is null", who); return false; }
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (sac_plan(sac->obs_dim, sac->act_dim, sac->n_pi, sac->pi_width, sac->n_qf, sac->qf_width, S, &actor, &critic, &why) == 0) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: %s", who, why); return false; }
  if (sac->activation != MCG_POLICY_TANH && sac->activation != MCG_POLICY_RELU) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: activation must be MCG_POLICY_TANH or MCG_POLICY_RELU", who); return false; }
  if (sac->actor_floats != actor || sac->critic_floats != critic) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: actor_floats / critic_floats are %lld / %lld, mcg_sac_blob_floats gives %lld / %lld for this shape", who,
                  (long long)sac->actor_floats, (long long)sac->critic_floats, (long long)actor, (long long)critic);
    return false;
  }
  if (((need & NEED_ACTOR) && ((uintptr_t)sac->actor & 15)) || ((need & NEED_CRITIC) && ((uintptr_t)sac->critic & 15)) ||
      ((need & NEED_TARGET) && ((uintptr_t)sac->critic_target & 15))) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: a blob is not 16-byte aligned", who); return false; }
  S->pi.blob = sac->actor; S->pi.act = S->qf[0].act = S->qf[1].act = sac->activation;
  return true;
}

inline bool checked_rows(const char* who, int64_t B) {
  if (B < 1) { mcg::mcg_fail(MCG_ERR_ARG, "%s: B must be >= 1", who); return false; }
  if (B * MAX_ACT >= (1ll << 31)) { mcg::mcg_fail(MCG_ERR_ARG, "%s: B must be below 2^27", who); return false; }
  return true;
}

inline int widest(const mcg_sac* sac, bool pi, bool qf) {
  int w = 0;
  for (int L = 0; pi && L < sac->n_pi; L++) w = sac->pi_width[L] > w ? sac->pi_width[L] : w;
  for (int L = 0; qf && L < sac->n_qf; L++) w = sac->qf_width[L] > w ? sac->qf_width[L] : w;
  return w;
}

}  // namespace
