// mcg_render.hip -- the ray caster's translation unit (kernel: mcg_render.hpp; host entries mcg_render, mcg_render_mounted,
// mcg_render_scenes, mcg_scene_randomize: mcg_hip.hip), and the kernel that draws the per-environment scene tables.
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
  if (mounted) hipLaunchKernelGGL((render_kernel<true, false>), dim3(n), dim3(RENDER_LANES), lds_bytes, stream, A, qpos, goal, n, nq, model, body, znear, nullptr);
  else hipLaunchKernelGGL((render_kernel<false, false>), dim3(n), dim3(RENDER_LANES), lds_bytes, stream, A, qpos, goal, n, nq, model, body, znear, nullptr);
  return (int)hipGetLastError();
}

int launch_render_scenes(const RenderArgs& A, const double* scenes, int body, float znear, int n, int nq, size_t lds_bytes, hipStream_t stream,
                         const double* qpos, const double* goal, const mcg_model* model) {
  hipLaunchKernelGGL((render_kernel<true, true>), dim3(n), dim3(RENDER_LANES), lds_bytes, stream, A, qpos, goal, n, nq, model, body, znear, scenes);
  return (int)hipGetLastError();
}

// ---- mcg_scene_randomize (include/mcg.h): one lane per environment, one row of the table each
namespace {

// the reset draws' keying (mcg_hip.hip: rng_pair) and 53-bit mapping, on the pictures' stream
constexpr uint32_t SCENE_STREAM = 2, SCENE_CAM_DRAW0 = 32, SCENE_CAM_DRAWS = 4;

MCG_DEV void scene_pair(const SceneRandArgs& P, int i, int32_t episode, uint32_t draw, real& u0, real& u1) {
  const unsigned long long gid = (unsigned long long)(P.env_id_offset + i);
  uint32_t r[4];
  philox4x32_10((uint32_t)gid, (uint32_t)episode, draw, SCENE_STREAM ^ ((uint32_t)(gid >> 32) << 8), (uint32_t)P.seed, (uint32_t)(P.seed >> 32), r);
  u0 = (real)((((unsigned long long)r[0] << 32) | r[1]) >> 11) * (1.0 / 9007199254740992.0);
  u1 = (real)((((unsigned long long)r[2] << 32) | r[3]) >> 11) * (1.0 / 9007199254740992.0);
}

// a + (b - a) * u as one explicit fma, as sample_goal maps its uniforms
MCG_DEV real scene_map(real lo, real hi, real u) { return fma(hi - lo, u, lo); }
// a zero offset leaves the base's value as it is, a signed zero included
MCG_DEV real scene_add(real x, real d) { return d == 0.0 ? x : x + d; }

__global__ __launch_bounds__(64) void scene_randomize_kernel(SceneRandArgs P, const int32_t* __restrict__ episode, const uint8_t* __restrict__ mask,
                                                             double* __restrict__ scenes) {
  const int i = blockIdx.x * 64 + threadIdx.x;
  if (i >= P.n) return;
  if (mask && mask[i] == 0) return;
  const int32_t ep = episode[i];
  const real* B = P.base;
  real out[MCG_SCENE_ENV_DOUBLES];
  real u0, u1;
  // ---- the world block: light and colours
  scene_pair(P, i, ep, 0, u0, u1);
  {
    const real th = P.r.light_tilt * sqrt(u0), ph = 6.283185307179586476925 * u1;
    const real* d0 = B + MCG_SCENE_LIGHT_DIR;
    const bool usey = fabs(d0[0]) > 0.9;
    const real ax[3] = {usey ? 0.0 : 1.0, usey ? 1.0 : 0.0, 0.0};
    real e1[3] = {ax[1] * d0[2] - ax[2] * d0[1], ax[2] * d0[0] - ax[0] * d0[2], ax[0] * d0[1] - ax[1] * d0[0]};
    const real inv = 1.0 / sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]);
    for (int k = 0; k < 3; k++) e1[k] *= inv;
    const real e2[3] = {d0[1] * e1[2] - d0[2] * e1[1], d0[2] * e1[0] - d0[0] * e1[2], d0[0] * e1[1] - d0[1] * e1[0]};
    real st, ct, sp, cp;
    sincos(th, &st, &ct); sincos(ph, &sp, &cp);
    for (int k = 0; k < 3; k++) out[MCG_SCENE_LIGHT_DIR + k] = th == 0.0 ? d0[k] : ct * d0[k] + st * (cp * e1[k] + sp * e2[k]);
  }
  scene_pair(P, i, ep, 1, u0, u1);
  out[MCG_SCENE_LIGHT_AMBIENT] = B[MCG_SCENE_LIGHT_AMBIENT] * scene_map(P.r.light_ambient_scale[0], P.r.light_ambient_scale[1], u0);
  out[MCG_SCENE_LIGHT_DIFFUSE] = B[MCG_SCENE_LIGHT_DIFFUSE] * scene_map(P.r.light_diffuse_scale[0], P.r.light_diffuse_scale[1], u1);
  scene_pair(P, i, ep, 2, u0, u1);
  {
    const real s = scene_map(P.r.head_scale[0], P.r.head_scale[1], u0);
    out[MCG_SCENE_HEAD_AMBIENT] = B[MCG_SCENE_HEAD_AMBIENT] * s; out[MCG_SCENE_HEAD_DIFFUSE] = B[MCG_SCENE_HEAD_DIFFUSE] * s;
  }
  _Pragma("unroll") for (int k = 0; k < 9; k++) {
    scene_pair(P, i, ep, 3 + k, u0, u1);
    _Pragma("unroll") for (int j = 0; j < 2; j++) {
      const int ch = 2 * k + j;
      const real h = P.r.rgb[ch / 3];
      const real c = scene_add(B[MCG_SCENE_RGB + ch], scene_map(-h, h, j ? u1 : u0));
      out[MCG_SCENE_RGB + ch] = c < 0.0 ? 0.0 : (c > 1.0 ? 1.0 : c);
    }
  }
  // ---- the camera block of this slot
  const uint32_t cd = SCENE_CAM_DRAW0 + SCENE_CAM_DRAWS * (uint32_t)P.cam_slot;
  real dpos[3], w[3], uf, unused;
  scene_pair(P, i, ep, cd, u0, u1);
  dpos[0] = scene_map(-P.r.cam_pos[0], P.r.cam_pos[0], u0); dpos[1] = scene_map(-P.r.cam_pos[1], P.r.cam_pos[1], u1);
  scene_pair(P, i, ep, cd + 1, u0, uf);
  dpos[2] = scene_map(-P.r.cam_pos[2], P.r.cam_pos[2], u0);
  scene_pair(P, i, ep, cd + 2, u0, u1);
  w[0] = scene_map(-P.r.cam_rot[0], P.r.cam_rot[0], u0); w[1] = scene_map(-P.r.cam_rot[1], P.r.cam_rot[1], u1);
  scene_pair(P, i, ep, cd + 3, u0, unused);
  w[2] = scene_map(-P.r.cam_rot[2], P.r.cam_rot[2], u0);
  for (int k = 0; k < 3; k++) out[MCG_SCENE_CAM_POS + k] = scene_add(B[MCG_SCENE_CAM_POS + k], dpos[k]);
  out[MCG_SCENE_FOVY] = B[MCG_SCENE_FOVY] * scene_map(P.r.fovy_scale[0], P.r.fovy_scale[1], uf);
  {
    const real th = sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2]);
    const bool tiny = th < 1e-12;
    real sn_, cs_; sincos(th, &sn_, &cs_);
    const real a = tiny ? 1.0 : sn_ / th, b = tiny ? 0.5 : (1.0 - cs_) / (th * th);
    const real K[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    real R[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) {
        const real k2 = K[3*r] * K[c] + K[3*r+1] * K[3 + c] + K[3*r+2] * K[6 + c];
        R[3*r + c] = (r == c ? 1.0 : 0.0) + a * K[3*r + c] + b * k2;
      }
    const real* M = B + MCG_SCENE_CAM_MAT;
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++)
        out[MCG_SCENE_CAM_MAT + 3*r + c] = th == 0.0 ? M[3*r + c] : R[3*r] * M[c] + R[3*r+1] * M[3 + c] + R[3*r+2] * M[6 + c];
  }
  out[MCG_SCENE_PAD] = 0.0; out[MCG_SCENE_PAD + 1] = 0.0;
  double* dst = scenes + (size_t)i * MCG_SCENE_ENV_DOUBLES;
  _Pragma("unroll") for (int k = 0; k < MCG_SCENE_ENV_DOUBLES; k++) dst[k] = out[k];
}

}  // namespace

int launch_scene_randomize(const SceneRandArgs& P, const int32_t* episode, const uint8_t* mask, double* scenes, hipStream_t stream) {
  hipLaunchKernelGGL(scene_randomize_kernel, dim3((P.n + 63) / 64), dim3(64), 0, stream, P, episode, mask, scenes);
  return (int)hipGetLastError();
}

}  // namespace mcg
