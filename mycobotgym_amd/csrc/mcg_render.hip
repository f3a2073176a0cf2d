// mcg_render.hip -- the ray caster: its kernel (mcg_render.hpp), the kernel that draws the per-environment scene tables, and the host
// entries of both (include/mcg.h: mcg_render, mcg_render_mounted, mcg_render_scenes, mcg_scene_randomize), with the face table that
// mcg_create has this unit build.  The engine behind the handle -- mcg_env, the state's layout, error reporting -- is mcg_engine.hpp's.
//
// A translation unit of its own, so a code object of its own: with the kernel in mcg_hip.hip's code object the step kernels, whose
// instructions did not change by one bit, moved by 16.5 KB inside it and the headline bench ran 0.6-0.8 % slower than the build without
// the ray caster, in every one of fifteen alternations.  Built this way mcg_hip.hip's code object is laid out as it
// is without the ray caster (it differs in the compilation unit's id alone).
#include <cstring>

#include "mcg_engine.hpp"
#include "mcg_render.hpp"

using namespace mcg;

// the face planes of a polytope block (checked by mcg_create) as float32 (n, d), mesh by mesh, each range padded to a multiple of four
void mcg::render_face_table(mcg_env* e, const double* pb) {
  std::vector<float>& tab = e->faces_host;
  for (int mm = 0; mm < MCG_NMESH; mm++) {
    const double* meta = pb + 8 * mm;
    const long long nf = (long long)meta[1], off = (long long)meta[3], vp = (long long)meta[4], fp = (long long)meta[5];
    const double* f = pb + off + 3 * vp;                    // [4, Fpad]: nx ny nz d
    e->foff[mm] = (int)(tab.size() / 4);
    for (long long k = 0; k < nf; k++) for (int a = 0; a < 4; a++) tab.push_back((float)f[a * fp + k]);
    while ((tab.size() / 4) % 4) { tab.insert(tab.end(), {0.0f, 0.0f, 0.0f, 1e30f}); }
  }
  e->foff[MCG_NMESH] = (int)(tab.size() / 4);
  if (tab.empty()) tab.assign(4, 0.0f);
}

// ---- the three picture entries' shared pieces (host only)
// the checks of what is per call, in the order and with the texts mcg_render has always had; nothing here touches HIP
static int render_call_checks(const char* fn, const mcg_render_out* out, int width, int height, int samples, int body, double znear) {
  if (!out->rgb && !out->gray && !out->depth && !out->geom) return mcg_fail(MCG_ERR_ARG, "%s: all four outputs are null", fn);
  if (width < 1 || width > 512 || height < 1 || height > 512) return mcg_fail(MCG_ERR_ARG, "%s: width and height must be in 1..512", fn);
  if (samples < 1 || samples > 4) return mcg_fail(MCG_ERR_ARG, "%s: samples must be in 1..4", fn);
  if (body < -1 || body >= NB) return mcg_fail(MCG_ERR_ARG, "%s: body must be -1 (the world) or an engine body 0..11", fn);
  if (!(std::isfinite(znear) && znear >= 0.0)) return mcg_fail(MCG_ERR_ARG, "%s: znear must be finite and not negative", fn);
  return MCG_OK;
}

// the checks of a scene's own values
static int scene_value_checks(const char* fn, const mcg_scene* sc) {
  if (!(sc->fovy > 0.0 && sc->fovy < 180.0)) return mcg_fail(MCG_ERR_ARG, "%s: fovy must be in (0, 180) degrees", fn);
  for (int a = 0; a < 3; a++)
    for (int b = 0; b < 3; b++) {
      double s = 0;
      for (int k = 0; k < 3; k++) s += sc->cam_mat[3 * k + a] * sc->cam_mat[3 * k + b];
      if (!(std::fabs(s - (a == b ? 1.0 : 0.0)) <= 1e-9)) return mcg_fail(MCG_ERR_ARG, "%s: cam_mat is not orthonormal to 1e-9", fn);
    }
  if (!(std::fabs(norm3(sc->light_dir) - 1.0) <= 1e-9)) return mcg_fail(MCG_ERR_ARG, "%s: light_dir is not a unit vector to 1e-9", fn);
  return MCG_OK;
}

// after the host checks of a call: the engine can be drawn, and its face table is on the device (the first picture's blocking copy)
static int render_ready(const char* fn, mcg_env* e) {
  if (!e) return mcg_fail(MCG_ERR_ARG, "%s: null handle", fn);
  if (!e->render_ok) return mcg_fail(MCG_ERR_UNSUPPORTED, "mcg_render: this engine's model came without the polytope block specialised with it: %s", e->render_why);
  if (e->d_faces) return MCG_OK;
  HIP_OK(hipSetDevice(e->device));
  float4* d = nullptr;
  HIP_OK(hipMalloc(&d, e->faces_host.size() * sizeof(float)));
  const hipError_t err = hipMemcpy(d, e->faces_host.data(), e->faces_host.size() * sizeof(float), hipMemcpyHostToDevice);
  if (err != hipSuccess) { (void)hipFree(d); return mcg_fail(MCG_ERR_HIP, "mcg_render: %s", hipGetErrorString(err)); }
  e->d_faces = d;
  return MCG_OK;
}

// what of RenderArgs is per call: the target box, the picture, the face table, mask and outputs; the rest is zero
static RenderArgs render_call_args(const mcg_env* e, const double* target_half, int width, int height, int samples, int target_at_goal,
                                   const uint8_t* mask, const mcg_render_out* out) {
  RenderArgs A;
  memset(&A, 0, sizeof(A));
  for (int k = 0; k < 3; k++) A.target_half[k] = (float)target_half[k];
  A.W = width; A.H = height; A.S = samples; A.target_at_goal = target_at_goal ? 1 : 0;
  A.draw_cube = (e->cfg.has_object && !e->cfg.hidden) ? 1 : 0;       // the reference hides the cube in Reach (mycobot.py:475-481)
  A.dwords = (width % 4 == 0) && ((uintptr_t)out->rgb % 4 == 0) && ((uintptr_t)out->gray % 4 == 0) && ((uintptr_t)out->depth % 16 == 0)
             && ((uintptr_t)out->geom % 4 == 0);
  memcpy(A.foff, e->foff, sizeof(A.foff));
  A.faces = e->d_faces; A.mask = mask; A.out = *out;
  return A;
}

// the launch of one instantiation (`who` names it in the message): a workgroup per environment, over the qpos and goal rows of the state
template <bool MOUNTED, bool SCENES>
static int render_launch(const char* who, const mcg_env* e, const RenderArgs& A, void* stream, int body, double znear, const double* scenes) {
  const View& V = e->view;
  const size_t lds_bytes = (size_t)render_head_floats(MOUNTED, SCENES) * sizeof(float) + (size_t)e->foff[MCG_NMESH] * sizeof(float4) + RENDER_TILE_BYTES;     // built-in tables: 35 KB
  if (lds_bytes > 64 * 1024) return mcg_fail(MCG_ERR_UNSUPPORTED, "mcg_render: the face tables do not fit the 64 KB of LDS a workgroup asks for (about 3 200 faces)");
  hipLaunchKernelGGL((render_kernel<MOUNTED, SCENES>), dim3(V.n), dim3(RENDER_LANES), lds_bytes, (hipStream_t)stream, A, V.row(V.rows().qpos),
                     V.row(V.rows().goal), V.n, V.nq, e->d_model, body, (float)znear, scenes);
  const hipError_t lerr = hipGetLastError();
  return lerr == hipSuccess ? MCG_OK : mcg_fail(MCG_ERR_HIP, "%s: launch: %s", who, hipGetErrorString(lerr));
}

extern "C" {

int mcg_render_mounted(mcg_env* e, const mcg_scene* sc, int body, double znear, int width, int height, int samples, int target_at_goal,
                       const uint8_t* mask, const mcg_render_out* out, void* stream) {
  // host checks first: nothing below them touches HIP.  (mcg_render is this entry with body = -1, znear = 0: it keeps its kernel and its texts)
  const bool mounted = !(body == -1 && znear == 0.0);
  const char* fn = mounted ? "mcg_render_mounted" : "mcg_render";
  if (!sc || !out) return mcg_fail(MCG_ERR_ARG, "%s: null scene or output block", fn);
  if (int rc = render_call_checks(fn, out, width, height, samples, body, znear)) return rc;
  if (int rc = scene_value_checks(fn, sc)) return rc;
  if (int rc = render_ready(fn, e)) return rc;
  RenderArgs A = render_call_args(e, sc->target_half, width, height, samples, target_at_goal, mask, out);
  for (int k = 0; k < 3; k++) { A.cam_pos[k] = sc->cam_pos[k]; A.light[k] = sc->light_dir[k]; }
  for (int k = 0; k < 9; k++) { A.cam_mat[k] = sc->cam_mat[k]; A.cam_matf[k] = (float)sc->cam_mat[k]; }
  A.focal = (float)(0.5 * height / std::tan(0.5 * sc->fovy * 3.14159265358979323846 / 180.0));
  A.la = (float)sc->light_ambient; A.ld = (float)sc->light_diffuse; A.ha = (float)sc->head_ambient; A.hd = (float)sc->head_diffuse;
  const double* rgb[6] = {sc->rgb_ground, sc->rgb_table, sc->rgb_cube, sc->rgb_target, sc->rgb_mesh, sc->rgb_sky};
  for (int c = 0; c < 6; c++) for (int k = 0; k < 3; k++) A.rgb[c][k] = (float)(255.0 * rgb[c][k]);
  return mounted ? render_launch<true, false>("mcg_render", e, A, stream, body, znear, nullptr)
                 : render_launch<false, false>("mcg_render", e, A, stream, body, znear, nullptr);
}

int mcg_render_scenes(mcg_env* e, const double* scenes, const double* target_half, int body, double znear, int width, int height, int samples,
                      int target_at_goal, const uint8_t* mask, const mcg_render_out* out, void* stream) {
  const char* fn = "mcg_render_scenes";
  if (!scenes) return mcg_fail(MCG_ERR_ARG, "%s: null scene table", fn);
  if (!target_half || !out) return mcg_fail(MCG_ERR_ARG, "%s: null target_half or output block", fn);
  if (int rc = render_call_checks(fn, out, width, height, samples, body, znear)) return rc;
  if (int rc = render_ready(fn, e)) return rc;
  const RenderArgs A = render_call_args(e, target_half, width, height, samples, target_at_goal, mask, out);      // camera, light and colours stay zero: the kernel takes them from the table
  return render_launch<true, true>("mcg_render_scenes", e, A, stream, body, znear, scenes);
}

int mcg_render(mcg_env* e, const mcg_scene* sc, int width, int height, int samples, int target_at_goal, const uint8_t* mask,
               const mcg_render_out* out, void* stream) {
  return mcg_render_mounted(e, sc, -1, 0.0, width, height, samples, target_at_goal, mask, out, stream);
}

}  // extern "C"

// ---- mcg_scene_randomize (include/mcg.h): one lane per environment, one row of the table each
namespace mcg {
struct SceneRandArgs {
  double base[MCG_SCENE_PAD];                         // the base scene as a row
  mcg_scene_rand r;
  unsigned long long seed;
  long long env_id_offset;
  int cam_slot, n;
};

namespace {

// the reset draws' keying (mcg_hip.hip: rng_pair), on the pictures' stream
constexpr uint32_t SCENE_CAM_DRAW0 = 32, SCENE_CAM_DRAWS = 4;

MCG_DEV void scene_pair(const SceneRandArgs& P, int i, int32_t episode, uint32_t draw, real& u0, real& u1) {
  const unsigned long long gid = (unsigned long long)(P.env_id_offset + i);
  philox_pair((uint32_t)gid, (uint32_t)episode, draw, DOMAIN_SCENE ^ ((uint32_t)(gid >> 32) << 8), P.seed, u0, u1);
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
}  // namespace mcg

extern "C" int mcg_scene_randomize(mcg_env* e, const mcg_scene* base, const mcg_scene_rand* r, int cam_slot, const uint8_t* mask, double* scenes, void* stream) {
  const char* fn = "mcg_scene_randomize";
  if (!base || !r || !scenes) return mcg_fail(MCG_ERR_ARG, "%s: null base scene, ranges or scene table", fn);
  if (cam_slot < 0 || cam_slot >= MCG_SCENE_RAND_CAM_SLOTS) return mcg_fail(MCG_ERR_ARG, "%s: cam_slot must be in 0..7", fn);
  {
    bool ok = std::isfinite(r->light_tilt) && r->light_tilt >= 0.0;
    for (int k = 0; k < 3; k++) ok = ok && std::isfinite(r->cam_pos[k]) && r->cam_pos[k] >= 0.0 && std::isfinite(r->cam_rot[k]) && r->cam_rot[k] >= 0.0;
    for (int k = 0; k < 6; k++) ok = ok && std::isfinite(r->rgb[k]) && r->rgb[k] >= 0.0;
    if (!ok) return mcg_fail(MCG_ERR_ARG, "%s: a range is negative or not finite", fn);
  }
  if (!(r->light_tilt <= 3.14159265358979323846)) return mcg_fail(MCG_ERR_ARG, "%s: light_tilt must be in [0, pi]", fn);
  const double* pairs[4] = {r->fovy_scale, r->light_ambient_scale, r->light_diffuse_scale, r->head_scale};
  for (int k = 0; k < 4; k++)
    if (!(std::isfinite(pairs[k][0]) && std::isfinite(pairs[k][1]) && pairs[k][0] > 0.0 && pairs[k][0] <= pairs[k][1]))
      return mcg_fail(MCG_ERR_ARG, "%s: a scale pair needs 0 < lo <= hi, both finite", fn);
  if (int rc = scene_value_checks(fn, base)) return rc;
  if (!(base->fovy * r->fovy_scale[1] < 180.0)) return mcg_fail(MCG_ERR_ARG, "%s: fovy * fovy_scale[1] must stay below 180 degrees", fn);
  if (!e) return mcg_fail(MCG_ERR_ARG, "%s: null handle", fn);
  SceneRandArgs P;
  static_assert(offsetof(mcg_scene, target_half) == MCG_SCENE_PAD * sizeof(double), "a row is the head of mcg_scene");
  memcpy(P.base, base, sizeof(P.base));
  P.r = *r; P.seed = e->cfg.seed; P.env_id_offset = e->cfg.env_id_offset; P.cam_slot = cam_slot; P.n = e->cfg.n;
  hipLaunchKernelGGL(scene_randomize_kernel, dim3((P.n + 63) / 64), dim3(64), 0, (hipStream_t)stream, P, e->view.i32 + e->cfg.n, mask, scenes);
  const hipError_t lerr = hipGetLastError();
  if (lerr != hipSuccess) return mcg_fail(MCG_ERR_HIP, "mcg_scene_randomize: launch: %s", hipGetErrorString(lerr));
  return MCG_OK;
}
