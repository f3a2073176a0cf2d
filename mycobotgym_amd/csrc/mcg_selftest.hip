// mcg_selftest.hip -- device self-tests: entries that run one device function of the step kernels on inputs a test hands in, where no
// state of the engine can bring those inputs about (include/mcg.h: mcg_selftest_bad_value).  No engine handle, nothing on the hot path.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives: the step kernels' code object stays as it is.
#include <hip/hip_runtime.h>

#include "mcg.h"
#include "mcg_engine.hpp"        // mcg_fail
#include "mcg_dynamics.hpp"      // bad_value, bad_value_any; build_H, ldl_factor, build_factor_H

using namespace mcg;

namespace {

constexpr int ST_LANES = 64;

// Lane = one case: a[12], r[12], qd_old[12], q_old[12], h.  The new velocities and positions come from robot_substep's own chain of
// fmas (bad_value_any's guarantee), the two predicates from the same registers.
__global__ __launch_bounds__(ST_LANES) void selftest_bad_value_kernel(const real* __restrict__ in, int n, real* __restrict__ state,
                                                                      uint8_t* __restrict__ each, uint8_t* __restrict__ any) {
  const int c = blockIdx.x * ST_LANES + threadIdx.x;
  if (c >= n) return;
  const real* p = in + (size_t)c * MCG_SELFTEST_BAD_VALUE_IN;
  const real h = p[4 * NB];
  real a[NB], qdn[NB], qn[NB];
  bool bad = false;
  static_for<NB>([&](auto I) { constexpr int i = I;
    a[i] = p[i];
    const real rhs = fma(-h, p[NB + i], a[i]);
    qdn[i] = fma(h, rhs, p[2 * NB + i]); qn[i] = fma(h, qdn[i], p[3 * NB + i]);
    bad = bad || bad_value(qn[i]) || bad_value(qdn[i]) || bad_value(a[i]); });
  const bool bad_any = bad_value_any(a, qdn, qn);
  static_for<NB>([&](auto I) { constexpr int i = I; state[(size_t)c * 2 * NB + i] = qdn[i]; state[(size_t)c * 2 * NB + NB + i] = qn[i]; });
  each[c] = bad ? 1 : 0; any[c] = bad_any ? 1 : 0;
}

// Lane = one case: H_eq[78], M[78], D[10], act[10], b[12].  H_eq and M go into the lane's LDS column, in the slots and with the slot
// stride the Reach kernels use; route 0 is build_H + ldl_factor<PAT_H> through the helper wave's window, route 1 build_factor_H through
// the RNE wave's windows (the two side waves' accessors; both serve these slots).  Each route solves H x = b with its own factor.
constexpr int TRI = NB * (NB + 1) / 2;
static_assert(MCG_SELFTEST_FACTOR_H_IN == 2 * TRI + 10 + 10 + NB && MCG_SELFTEST_FACTOR_H_OUT == 2 * (TRI + NB + NB), "mcg.h: the factor self-test's records");
static_assert(LDS_M + TRI <= LDS_SLOTS && LDS_HEQ + TRI <= LDS_SLOTS, "H_eq and M lie in the first LDS_SLOTS slots of the column");
__global__ __launch_bounds__(ST_LANES) void selftest_factor_h_kernel(const real* __restrict__ in, int n, real* __restrict__ out) {
  __shared__ real lds[LDS_SLOTS][ST_LANES];
  const int c = blockIdx.x * ST_LANES + threadIdx.x;
  const bool live = c < n;
  const real* p = in + (size_t)(live ? c : 0) * MCG_SELFTEST_FACTOR_H_IN;      // a lane past n recomputes case 0 and stores nothing
  const LaneScratch MS(&lds[0][threadIdx.x]);
  for (int k = 0; k < TRI; k++) { MS.st(LDS_HEQ + k, p[k]); MS.st(LDS_M + k, p[TRI + k]); }
  real Dl[10], b[NB];
  bool act[10];
  static_for<10>([&](auto I) { constexpr int j = I; Dl[j] = p[2 * TRI + j]; act[j] = p[2 * TRI + 10 + j] != 0; });
  static_for<NB>([&](auto I) { constexpr int i = I; b[i] = p[2 * TRI + 20 + i]; });
  __syncthreads();
  real* o = out + (size_t)(live ? c : 0) * MCG_SELFTEST_FACTOR_H_OUT;
  auto put = [&](int at, const real* L, const real* dinv, const real* x) {
    if (!live) return;
    static_for<NB>([&](auto I) { constexpr int i = I;
      static_for<i + 1>([&](auto Jj) { constexpr int j = Jj; o[at + tri(i, j)] = PAT_H.nz[i][j] ? L[tri(i, j)] : 0.0; });
      o[at + TRI + i] = dinv[i]; o[at + TRI + NB + i] = x[i]; });
  };
  {
    real L[TRI], dinv[NB], x[NB];
    const LowScratch MW(MS);
    build_H<SplitMainCols>(MW, L, act, Dl);
    ldl_factor<PAT_H>(L, dinv);
    static_for<NB>([&](auto I) { constexpr int i = I; x[i] = b[i]; });
    ldl_solve<PAT_H>(L, dinv, x);
    put(0, L, dinv, x);
  }
  {
    real L[TRI], dinv[NB], x[NB];
    const SideScratch MW(MS);
    build_factor_H<SplitMainCols>(MW, L, dinv, act, Dl);
    static_for<NB>([&](auto I) { constexpr int i = I; x[i] = b[i]; });
    ldl_solve<PAT_H>(L, dinv, x);
    put(TRI + 2 * NB, L, dinv, x);
  }
}

}  // namespace

int mcg_selftest_factor_h(const double* in, int n, double* out, void* stream) {
  const char* who = "mcg_selftest_factor_h";
  if (!in || !out) return mcg_fail(MCG_ERR_ARG, "%s: null pointer", who);
  if (n < 1 || n > (1 << 20)) return mcg_fail(MCG_ERR_ARG, "%s: n must be in [1, 2^20]", who);
  hipLaunchKernelGGL(selftest_factor_h_kernel, dim3((n + ST_LANES - 1) / ST_LANES), dim3(ST_LANES), 0, (hipStream_t)stream, in, n, out);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MCG_OK : mcg_fail(MCG_ERR_HIP, "%s kernel launch: %s", who, hipGetErrorString(e));
}

int mcg_selftest_bad_value(const double* in, int n, double* state, uint8_t* each, uint8_t* any, void* stream) {
  const char* who = "mcg_selftest_bad_value";
  if (!in || !state || !each || !any) return mcg_fail(MCG_ERR_ARG, "%s: null pointer", who);
  if (n < 1 || n > (1 << 20)) return mcg_fail(MCG_ERR_ARG, "%s: n must be in [1, 2^20]", who);
  hipLaunchKernelGGL(selftest_bad_value_kernel, dim3((n + ST_LANES - 1) / ST_LANES), dim3(ST_LANES), 0, (hipStream_t)stream, in, n, state, each, any);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MCG_OK : mcg_fail(MCG_ERR_HIP, "%s kernel launch: %s", who, hipGetErrorString(e));
}
