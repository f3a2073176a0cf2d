// mcg_selftest.hip -- device self-tests: entries that run one device function of the step kernels on inputs a test hands in, where no
// state of the engine can bring those inputs about (include/mcg.h: mcg_selftest_bad_value).  No engine handle, nothing on the hot path.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives: the step kernels' code object stays as it is.
#include <hip/hip_runtime.h>

#include "mcg.h"
#include "mcg_engine.hpp"        // mcg_fail
#include "mcg_dynamics.hpp"      // bad_value, bad_value_any

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

}  // namespace

int mcg_selftest_bad_value(const double* in, int n, double* state, uint8_t* each, uint8_t* any, void* stream) {
  const char* who = "mcg_selftest_bad_value";
  if (!in || !state || !each || !any) return mcg_fail(MCG_ERR_ARG, "%s: null pointer", who);
  if (n < 1 || n > (1 << 20)) return mcg_fail(MCG_ERR_ARG, "%s: n must be in [1, 2^20]", who);
  hipLaunchKernelGGL(selftest_bad_value_kernel, dim3((n + ST_LANES - 1) / ST_LANES), dim3(ST_LANES), 0, (hipStream_t)stream, in, n, state, each, any);
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MCG_OK : mcg_fail(MCG_ERR_HIP, "%s kernel launch: %s", who, hipGetErrorString(e));
}
