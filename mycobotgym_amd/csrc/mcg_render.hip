// mcg_render.hip -- the ray caster's translation unit (kernel: mcg_render.hpp; host entry mcg_render: mcg_hip.hip).
//
// A translation unit of its own, so a code object of its own: with the kernel in mcg_hip.hip's code object the step kernels, whose
// instructions did not change by one bit, moved by 16.5 KB inside it and the headline bench ran 0.6-0.8 % slower than the build without
// the ray caster, in every one of fifteen alternations.  Built this way mcg_hip.hip's code object is laid out as it
// is without the ray caster (it differs in the compilation unit's id alone).
#define MCG_RENDER_KERNELS
#include "mcg_render.hpp"

namespace mcg {

int launch_render(const RenderArgs& A, bool mounted, int body, float znear, int n, int nq, size_t lds_bytes, hipStream_t stream,
                  const double* qpos, const double* goal, const mcg_model* model) {
  if (mounted) hipLaunchKernelGGL(render_kernel<true>, dim3(n), dim3(RENDER_LANES), lds_bytes, stream, A, qpos, goal, n, nq, model, body, znear);
  else hipLaunchKernelGGL(render_kernel<false>, dim3(n), dim3(RENDER_LANES), lds_bytes, stream, A, qpos, goal, n, nq, model, body, znear);
  return (int)hipGetLastError();
}

}  // namespace mcg
