// mcg_sac.hpp -- what the off-policy learners' code objects share, SAC's (mcg_sac.hip, mcg_sac_grad.hip) and TD3's / DDPG's (mcg_td3.hip,
// mcg_td3_grad.hip, through mcg_td3.hpp): the kernels' view of the blobs, SAC's squash of its two heads (its draw: mcg_policy.hpp's gauss4), the
// critic's forward with the action as an operand, the critics' kernel and the Polyak kernel (each code object instantiates its own),
// the blobs' plan and the host checks of an entry's arguments.  The blobs' layouts, the action-as-operand rule and the noise are stated
// at mcg_sac.hip's head; TD3's own pieces (one head, tanh, the scaled noise) are mcg_td3.hpp's.
#pragma once

#include "mcg_policy.hpp"       // Net, Pol, mfma, activate, first_layer, dense, gauss4, checked_shape

namespace {

constexpr float LOG_STD_MIN = -20.0f, LOG_STD_MAX = 2.0f;

// mcg_sac or mcg_td3 as the kernels see it.  pi: the actor blob (TD3: or its target); net[1] is the trunk with the head mu, net[0] the
// same trunk with SAC's head log_std.  qf[k]: critic k of the critic or the target blob -- the same plan, net[0], from its own base, so
// that a kernel picks a critic by an address in its arguments and copies nothing; qa: the first layer's action tiles.
struct Sac { Pol pi, qf[2]; int qa; };

struct Rows { const float *obs, *achieved, *desired, *action; };                          // mcg_sac_rows
struct Batch { const float *next_obs, *next_achieved, *desired, *reward, *done; };        // mcg_her_batch

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
  if (!deterministic) gauss4(d.noise, A, g, seed, id, call, stream);
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

// A stored action in the accumulator layout: lane (g, i) takes components 4 g .. 4 g + 3 of `row`, those >= A as zeros.
MCG_DEV f4 load_action(int A, const float* __restrict__ action, int row, int g) {
  f4 act;
#pragma unroll
  for (int r = 0; r < 4; r++) {
    const int c = 4 * g + r;
    act[r] = 0.0f;
    if (c < A) act[r] = action[(size_t)row * A + c];
  }
  return act;
}

// Critic k on one row: `act` is the action in the accumulator layout.  The value is row 0 of the head: valid on the lanes g == 0.
template <int MT, class In>
MCG_DEV float critic(const Sac& S, int k, const In* __restrict__ obs, const In* __restrict__ ach, const In* __restrict__ des,
                     int row, const f4& act, int g, int lane) {
  const Pol& P = k ? S.qf[1] : S.qf[0];
  const Net& net = P.net[0];
  f4 a[MT], head[1];
  first_layer<MT, In>(P, net, obs, ach, des, row, g, lane, a);
  const float* __restrict__ Wa = P.blob + S.qa;
#pragma unroll
  for (int t = 0; t < MT; t++) {
    if (t < net.nt[0]) {
#pragma unroll
      for (int r = 0; r < 4; r++) a[t] = mfma(Wa[(t * 4 + r) * WAVE + lane], act[r], a[t]);
    }
  }
  hidden<MT>(P, net, a, g, lane);
  dense<MT, 1>(P, net, net.n, last_tiles(net), 1, a, head, g, lane);
  return head[0][0];
}

// mcg_sac_q and mcg_td3_q: one wave per (tile of 16 rows, critic); gridDim.y is the number of critics.
template <int MT>
__global__ __launch_bounds__(WAVE) void q_kernel(Sac S, Rows R, int B, float* __restrict__ q) {
  const int lane = threadIdx.x, g = lane >> 4, i = lane & 15;
  const int e = blockIdx.x * TILE + i;
  const bool live = e < B;
  const int row = live ? e : B - 1;
  const int k = blockIdx.y;
  const f4 act = load_action(S.pi.A, R.action, row, g);
  const float v = critic<MT, float>(S, k, R.obs, R.achieved, R.desired, row, act, g, lane);
  if (live && g == 0) q[(size_t)k * B + e] = v;
}

// target <- (float) fma(tau, (double) net, (1 - tau) * (double) target) on one pair of blobs, one lane per four floats: the product
// rounded to double, the fma rounded once, then the one rounding to float32.  A padding position, +0 in both, stays +0.  tau = 1
// (one_minus_tau == 0, the same for every lane) is the copy of the net's bits: the expression would turn a non-finite target element
// into NaN (0 * inf) and a net's -0 into +0.  THREADS: the block's size (a template: only the code objects that launch it hold it).
template <int THREADS>
__global__ __launch_bounds__(THREADS) void polyak_kernel(const float* __restrict__ net, float* __restrict__ target, int quads, double tau,
                                                     double one_minus_tau) {
  const int p = blockIdx.x * THREADS + threadIdx.x;
  if (p >= quads) return;
  const f4 c = reinterpret_cast<const f4*>(net)[p];
  f4 t = reinterpret_cast<f4*>(target)[p];
#pragma unroll
  for (int r = 0; r < 4; r++) t[r] = one_minus_tau == 0.0 ? c[r] : (float)fma(tau, (double)c[r], __dmul_rn(one_minus_tau, (double)t[r]));
  reinterpret_cast<f4*>(target)[p] = t;
}

// ------------------------------------------------------------------------------------------------------- host side
// The blobs' plan for a shape -> actor_floats + critic_floats; 0 and `why` for a refused shape.  The actor: the trunk, the head mu and,
// with log_std_head (SAC), the head log_std; the critic blob: n_critics critics.  S (where given): filled but for the blob pointers, N
// and act.
inline int64_t blob_plan(int obs_dim, int act_dim, int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, int n_critics,
                         bool log_std_head, Sac* S, int64_t* actor_floats, int64_t* critic_floats, const char** why) {
  if (n_critics != 1 && n_critics != 2) { *why = "n_critics must be 1 or 2"; return 0; }
  if (!checked_shape(obs_dim, act_dim, n_pi, pi_width, n_qf, qf_width, "qf", false, why)) return 0;
  const int kb0 = (obs_dim + 6 + 3) / 4;
  // the actor: the trunk, then the heads
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
  if (log_std_head) {
    ls.w[n_pi] = (int)at; at += head;
    ls.b[n_pi] = (int)at; at += 16;
  }
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
  at *= n_critics;                       // qf1: the same plan again
  if (S) {
    S->pi.net[1] = mu; S->pi.net[0] = ls; S->qf[0].net[0] = S->qf[1].net[0] = qf; S->qa = qa;
    S->pi.kb0 = S->qf[0].kb0 = S->qf[1].kb0 = kb0; S->pi.D = S->qf[0].D = S->qf[1].D = obs_dim; S->pi.A = S->qf[0].A = S->qf[1].A = act_dim;
  }
  if (actor_floats) *actor_floats = actor;
  if (critic_floats) *critic_floats = at;
  return actor + at;                     // < 2^21 floats at the largest shape
}

struct BlobArg { int bit; const void* p; const char* name; };

// What every entry checks of an mcg_sac or mcg_td3 `x` (not null; `what`: the struct's name) before it launches, `need` naming by
// their bits the ones of `blobs` that the entry touches -> true, and S filled but for the blob pointers and N; false after mcg_fail.
// named: an unaligned blob is refused by its name.
template <class T>
inline bool checked_blobs(const char* who, const char* what, const T* x, const BlobArg* blobs, int n, int need, int n_critics,
                          bool log_std_head, bool named, Sac* S) {
  for (int j = 0; j < n; j++)
    if ((need & blobs[j].bit) && !blobs[j].p) { mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is null", who, blobs[j].name); return false; }
  const char* why = nullptr;
  int64_t actor = 0, critic = 0;
  if (blob_plan(x->obs_dim, x->act_dim, x->n_pi, x->pi_width, x->n_qf, x->qf_width, n_critics, log_std_head, S, &actor, &critic, &why) == 0) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: %s", who, why); return false; }
  if (x->activation != MCG_POLICY_TANH && x->activation != MCG_POLICY_RELU) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: activation must be MCG_POLICY_TANH or MCG_POLICY_RELU", who); return false; }
  if (x->actor_floats != actor || x->critic_floats != critic) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: actor_floats / critic_floats are %lld / %lld, %s_blob_floats gives %lld / %lld for this shape", who,
                  (long long)x->actor_floats, (long long)x->critic_floats, what, (long long)actor, (long long)critic);
    return false;
  }
  for (int j = 0; j < n; j++)
    if ((need & blobs[j].bit) && ((uintptr_t)blobs[j].p & 15)) {
      if (named) mcg::mcg_fail(MCG_ERR_ARG, "%s: %s is not 16-byte aligned", who, blobs[j].name);
      else mcg::mcg_fail(MCG_ERR_ARG, "%s: a blob is not 16-byte aligned", who);
      return false;
    }
  S->pi.act = S->qf[0].act = S->qf[1].act = x->activation;
  return true;
}

enum { NEED_ACTOR = 1, NEED_CRITIC = 2, NEED_TARGET = 4 };

// checked_blobs of an mcg_sac's three blobs
inline bool checked_sac(const char* who, const mcg_sac* sac, int need, Sac* S) {
  if (!sac) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac", who); return false; }
  const BlobArg blobs[3] = {{NEED_ACTOR, sac->actor, "actor"}, {NEED_CRITIC, sac->critic, "critic"}, {NEED_TARGET, sac->critic_target, "critic_target"}};
  if (!checked_blobs(who, "mcg_sac", sac, blobs, 3, need, 2, true, false, S)) return false;
  S->pi.blob = sac->actor;
  return true;
}

// ---- an entry's other arguments, each refused in the entry's name (checked_rows: mcg_policy.hpp)
inline bool checked_envs(const char* who, long long n_envs) {
  if (n_envs < 1) { mcg::mcg_fail(MCG_ERR_ARG, "%s: n_envs must be >= 1", who); return false; }
  if (n_envs * MAX_ACT >= (1ll << 31)) { mcg::mcg_fail(MCG_ERR_ARG, "%s: n_envs must be below 2^27", who); return false; }
  return true;
}

inline bool checked_obs(const char* who, const mcg_step_out* obs) {
  if (!obs) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_step_out", who); return false; }
  if (!obs->obs || !obs->achieved_goal || !obs->desired_goal) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: obs, achieved_goal and desired_goal of the observation are required", who); return false; }
  return true;
}

// action: the rows' action is read too
inline bool checked_rows_arg(const char* who, const mcg_sac_rows* rows, bool action) {
  if (!rows) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_sac_rows", who); return false; }
  if (!rows->obs || !rows->achieved || !rows->desired || (action && !rows->action)) {
    if (action) mcg::mcg_fail(MCG_ERR_ARG, "%s: obs, achieved, desired and action of the rows are required", who);
    else mcg::mcg_fail(MCG_ERR_ARG, "%s: obs, achieved and desired of the rows are required", who);
    return false;
  }
  return true;
}

inline bool checked_batch(const char* who, const mcg_her_batch* batch) {
  if (!batch) { mcg::mcg_fail(MCG_ERR_ARG, "%s: null mcg_her_batch", who); return false; }
  if (!batch->next_obs || !batch->next_achieved || !batch->desired || !batch->reward || !batch->done) {
    mcg::mcg_fail(MCG_ERR_ARG, "%s: next_obs, next_achieved, desired, reward and done of the batch are required", who); return false; }
  return true;
}

inline int widest(int n_pi, const int32_t* pi_width, int n_qf, const int32_t* qf_width, bool pi, bool qf) {
  int w = 0;
  for (int L = 0; pi && L < n_pi; L++) w = pi_width[L] > w ? pi_width[L] : w;
  for (int L = 0; qf && L < n_qf; L++) w = qf_width[L] > w ? qf_width[L] : w;
  return w;
}
template <class T>
inline int widest(const T* x, bool pi, bool qf) { return widest(x->n_pi, x->pi_width, x->n_qf, x->qf_width, pi, qf); }

}  // namespace
