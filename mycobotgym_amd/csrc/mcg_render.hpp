// mcg_render.hpp -- the picture of an environment: a ray caster over the engine's own state (mcg_render; MyCobotImgEnv / render(),
// mycobot.py:308-311, 517-545).  The kernel; mcg_render.hip, which alone includes this file, holds the entries that launch it.
//
// The scene is the ground plane, three boxes (table, cube, target site) and the fourteen mesh geoms as their collision polytopes (face
// planes n.x <= d in the frame of the body a mesh rides on: the tables the mesh collision uses, within 1 mm of the convex hulls).  A ray
// against a convex polytope is a clip of the ray's parameter interval by the face planes; a ray against a box is a slab test.
//
// One workgroup of 256 lanes per environment:
//   1. lane 0 runs the kinematic chain of the twelve robot bodies (and places the cube) in float64 from the environment's qpos, with the
//      joint conventions and the sine / cosine of the step kernels (mcg_dynamics.hpp), and parks per body, as float32: the rotation, the
//      camera's position and the light's direction in the body's frame.  All per-ray arithmetic is float32.
//   2. the face tables (float32 n, d; a device copy made at mcg_create) are staged into LDS once, as (n, d - n.o) with o the camera's
//      position in the face's frame: every ray of the picture starts there, so the numerator of the clip is per face, not per ray.
//      A face then costs a wave one broadcast ds_read_b128, three FMAs, one reciprocal and a handful of selects.
//   3. a wave walks 16 x 16 pixel tiles, each as four compact 8 x 8 blocks of rays (lane = pixel).  Per ray: ground, table, cube, target,
//      then the meshes in a wave-uniform loop: the ray in the body's frame, slab test against mesh_box, and only where some lane's ray
//      enters the box in front of what it has already hit, the walk over the faces.  Nearest hit wins, ties go to the lower geom id
//      (strict `<` in ascending id order).  The tile's pixels pass through LDS so that a lane stores four consecutive pixels of a row:
//      its bytes leave as whole dwords.
// Nothing is written but the four output images (plain vector stores); the engine's state is only read.
//
// A camera mounted on a body (mcg_render_mounted; the reference's gripper_camera_rgb under `flange`) is the second instantiation of the
// kernel, render_kernel<true>: lane 0 finishes the chain first, composes the camera's world pose in float64 from the carrier body's R, p
// and parks it in the LDS head, and only then parks the per-body camera origins; the rays take the camera's matrix and position from
// there, lifted into uniform registers once per wave.  It also carries the near plane.  render_kernel<false> is the world camera's
// kernel as it was: the switch is a template parameter, so its instruction stream does not change.
//
// Per-environment scenes (mcg_render_scenes) are the third instantiation, render_kernel<true, true>: lane 0 reads the environment's row
// of the scene table (40 doubles), composes the camera's world pose from it as the mounted kernel does from the call's scene, and parks
// in the LDS head, as float32, what the rays need: the focal length in pixels, the four shading coefficients, the light's direction
// and the six colours x 255; the waves lift the scalars into uniform registers once.  Of RenderArgs it reads what is per call.
//
// Visibility.  Surfaces are one-sided: a convex geom whose entry point lies behind the camera or before the near plane (depth along the
// camera's -z below znear) is invisible along that ray, and the ray goes on to the other geoms.  So a camera inside a polytope does not
// see it (OpenGL's back-face culling on closed convex solids): the gripper camera sits inside the flange's polytope and looks out of it.
#pragma once

#include <hip/hip_runtime.h>
#include "mcg.h"
#include "mcg_dynamics.hpp"
#include "mcg_cube.hpp"

namespace mcg {

constexpr int RENDER_LANES = 256;
constexpr int RENDER_FRAMES = NB + 1;                 // twelve robot bodies, the cube
constexpr int RF_STRIDE = 16;                         // floats per parked frame: R[9] (row-major world <- body), camera o[3], light l[3], pad
constexpr int RF_O = 9, RF_L = 12;
constexpr int RENDER_BOX_FLOATS = 8;                  // per mesh: box centre [3], half [3], pad
constexpr int RENDER_RGB = RENDER_FRAMES * RF_STRIDE + NMESH * RENDER_BOX_FLOATS;       // six colours x 4 floats (a lane picks its own: an LDS read, not a kernel-argument index)
constexpr int RENDER_HEAD_FLOATS = RENDER_RGB + 6 * 4;                                  // 344: the faces follow, 16-byte aligned
static_assert((RENDER_HEAD_FLOATS * 4) % 16 == 0, "the face table is read as b128");
constexpr int RENDER_CAM = RENDER_HEAD_FLOATS;        // a mounted camera's head is longer: its world position [3], pad, rotation [9] (row-major world <- camera), pad
constexpr int RENDER_CAM_MAT = RENDER_CAM + 4;
constexpr int RENDER_HEAD_FLOATS_MOUNTED = RENDER_HEAD_FLOATS + 16;
static_assert((RENDER_HEAD_FLOATS_MOUNTED * 4) % 16 == 0, "the face table is read as b128");
// per-environment scenes (mcg_render_scenes): the mounted head and, converted by lane 0 from the environment's row, the focal length in
// pixels, the four shading coefficients, the light's direction in the world; the six colours take the place of the call's in RENDER_RGB
constexpr int RENDER_SCN = RENDER_HEAD_FLOATS_MOUNTED;
constexpr int RENDER_SCN_FOCAL = RENDER_SCN, RENDER_SCN_SHADE = RENDER_SCN + 1, RENDER_SCN_LIGHT = RENDER_SCN + 5;
constexpr int RENDER_HEAD_FLOATS_SCENES = RENDER_HEAD_FLOATS_MOUNTED + 8;
static_assert((RENDER_HEAD_FLOATS_SCENES * 4) % 16 == 0, "the face table is read as b128");
constexpr int render_head_floats(bool mounted, bool scenes) { return scenes ? RENDER_HEAD_FLOATS_SCENES : (mounted ? RENDER_HEAD_FLOATS_MOUNTED : RENDER_HEAD_FLOATS); }
constexpr int RENDER_TILE_BYTES = (RENDER_LANES / 64) * 3 * 256 * 4;                    // per wave: 256 pixels x (packed r g b gray, depth, geom); after the faces
constexpr float RENDER_BOX_SLACK = 1e-6f;             // the slab test is a filter: the faces decide

struct RenderArgs {
  double cam_pos[3], cam_mat[9], light[3];            // float64 for the change of frame (lane 0)
  float cam_matf[9], focal;                           // focal length in pixels: 0.5 H / tan(fovy / 2)
  float la, ld, ha, hd;
  float rgb[6][3];                                    // ground table cube target mesh sky, times 255
  float target_half[3];
  int W, H, S, target_at_goal, draw_cube;
  int dwords;                                         // W % 4 == 0 and the output pointers aligned: a lane's four pixels leave as whole dwords
  int foff[NMESH + 1];                                // face ranges in the device table (each padded to a multiple of four)
  const float4* faces;
  const uint8_t* mask;
  mcg_render_out out;
};

struct RayHit { float t; int id; float nl, nd; };      // distance along the (unit) ray, geom id, n.(-light), n.(-ray) of the face hit

// slab test of the ray o + t d against the box |x - c| <= h; on a hit (the ray enters from outside, in front of the camera): tin and the
// entry face's axis.  MOUNTED: a hit is a ray that is inside the box somewhere beyond tnear (the camera may be inside a mesh's box and
// outside its polytope); the caller asks for tin > tnear where the box is the solid itself
template <bool MOUNTED>
MCG_DEV bool ray_box(const float* o, const float* d, const float* c, const float* h, float tnear, float& tin, float& tout, int& axis) {
  tin = -INFINITY; tout = INFINITY; axis = 0;
  _Pragma("unroll") for (int k = 0; k < 3; k++) {
    const float inv = __builtin_amdgcn_rcpf(d[k]);
    const float a = (c[k] - h[k] - o[k]) * inv, b = (c[k] + h[k] - o[k]) * inv;
    const float lo = fminf(a, b), hi = fmaxf(a, b);               // (a NaN of 0 * inf drops out: fminf / fmaxf return the other operand)
    if (lo > tin) { tin = lo; axis = k; }
    tout = fminf(tout, hi);
  }
  if constexpr (MOUNTED) return tin <= tout && tout > tnear;
  else return tin <= tout && tin > 0.0f;
}

MCG_DEV void to_frame(const float* F, const float* dw, float* db) {      // db = R^T dw
  _Pragma("unroll") for (int j = 0; j < 3; j++) db[j] = F[j] * dw[0] + F[3 + j] * dw[1] + F[6 + j] * dw[2];
}

// a box with its own frame (F: parked frame, or null = world with the camera at ow and the light lw)
template <bool MOUNTED>
MCG_DEV void hit_box(RayHit& best, int id, const float* o, const float* d, const float* l, const float* c, const float* h, float tnear) {
  float tin, tout; int ax;
  bool hit = ray_box<MOUNTED>(o, d, c, h, tnear, tin, tout, ax) && h[0] > 0.0f && h[1] > 0.0f && h[2] > 0.0f;
  if constexpr (MOUNTED) hit = hit && tin > tnear;
  if (hit && tin < best.t) {
    const float dk = sel3(ax, d[0], d[1], d[2]), lk = sel3(ax, l[0], l[1], l[2]);
    const float sg = dk > 0.0f ? -1.0f : 1.0f;                    // the entry face looks against the ray
    best.t = tin; best.id = id; best.nl = -sg * lk; best.nd = -sg * dk;
  }
}

// tnear: the near plane as a distance along this ray (MOUNTED alone; the world camera's entry tests stay `> 0`)
template <bool MOUNTED, bool SCENES>
MCG_DEV RayHit trace(const RenderArgs& A, const float* __restrict__ lds, const float* camw, const float* lightw, const float* tpos,
                     const float* table_c, const float* table_h, const float* cube_h, const float* dw, float tnear) {
  RayHit best{INFINITY, -1, 0.0f, 0.0f};
  // 0: the ground plane z = 0, seen from above (infinite: the collision rule's plane)
  if constexpr (MOUNTED) {
    const float t = -camw[2] * __builtin_amdgcn_rcpf(dw[2]);
    if (dw[2] < 0.0f && camw[2] > 0.0f && t > tnear) { best.t = t; best.id = 0; best.nl = -lightw[2]; best.nd = -dw[2]; }
  } else {
    if (dw[2] < 0.0f && camw[2] > 0.0f) { best.t = -camw[2] * __builtin_amdgcn_rcpf(dw[2]); best.id = 0; best.nl = -lightw[2]; best.nd = -dw[2]; }
  }
  hit_box<MOUNTED>(best, 1, camw, dw, lightw, table_c, table_h, tnear);
  if (A.draw_cube) {                                               // wave-uniform
    const float* F = lds + NB * RF_STRIDE;
    float db[3]; to_frame(F, dw, db);
    const float zero[3] = {0.0f, 0.0f, 0.0f};
    hit_box<MOUNTED>(best, 2, F + RF_O, db, F + RF_L, zero, cube_h, tnear);
  }
  hit_box<MOUNTED>(best, 3, camw, dw, lightw, tpos, A.target_half, tnear);
  const float4* __restrict__ faces = (const float4*)(lds + render_head_floats(MOUNTED, SCENES));
  int body_at = -1;
  float db[3];
  const float* F = lds;
  for (int m = 0; m < NMESH; m++) {                                // wave-uniform
    const int body = mesh_body(m);
    if (body != body_at) { body_at = body; F = lds + body * RF_STRIDE; to_frame(F, dw, db); }      // meshes 5, 6, 7 share body 5
    const float* B = lds + RENDER_FRAMES * RF_STRIDE + m * RENDER_BOX_FLOATS;
    float bin, bout; int ax;
    const bool inbox = ray_box<MOUNTED>(F + RF_O, db, B, B + 3, tnear, bin, bout, ax) && bin < best.t;
    if (!__any(inbox)) continue;
    float tin = 0.0f, tout = INFINITY, nx = 0.0f, ny = 0.0f, nz = 0.0f;
    bool miss = false;
    const int f1 = A.foff[m + 1];
    for (int k = A.foff[m]; k < f1; k += 4) {                      // (ranges are padded to four with null faces: n = 0, d huge)
      _Pragma("unroll") for (int u = 0; u < 4; u++) {
        const float4 f = faces[k + u];                             // one address for the wave: a broadcast read
        const float den = f.x * db[0] + f.y * db[1] + f.z * db[2];
        const float t = f.w * __builtin_amdgcn_rcpf(den);          // f.w = d - n.o
        const bool enter = den < 0.0f && t > tin;
        tin = enter ? t : tin; nx = enter ? f.x : nx; ny = enter ? f.y : ny; nz = enter ? f.z : nz;
        tout = den > 0.0f ? fminf(tout, t) : tout;
        miss = miss || (den == 0.0f && f.w < 0.0f);
      }
    }
    if (!miss && tin <= tout && (MOUNTED ? tin > tnear : tin > 0.0f) && tin < best.t) {
      best.t = tin; best.id = 4 + m;
      best.nl = -(nx * F[RF_L] + ny * F[RF_L + 1] + nz * F[RF_L + 2]);
      best.nd = -(nx * db[0] + ny * db[1] + nz * db[2]);
    }
  }
  return best;
}

// one joint of the chain: the child's origin, then its rotation about axis K by sg * angle (as mcg_cube.hpp: collide_primitives)
template <int K>
MCG_DEV void render_joint(const TrigC& T, int sg, const real* r, real ang, real* R, real* p) {
  constexpr int A = (K + 1) % 3, B = (K + 2) % 3;
  for (int k = 0; k < 3; k++) p[k] += R[3*k]*r[0] + R[3*k+1]*r[1] + R[3*k+2]*r[2];
  real sn_, cs_; sincos_cw(T, sg * ang, sn_, cs_);
  for (int k = 0; k < 3; k++) {
    const real ca = R[3*k + A], cb = R[3*k + B];
    R[3*k + A] = cs_ * ca + sn_ * cb; R[3*k + B] = -sn_ * ca + cs_ * cb;
  }
}

// cam: the camera's world position, light: the light's direction in the world
MCG_DEV void render_park(const real* light, const real* cam, float* lds, int slot, const real* R, const real* p) {
  float* F = lds + slot * RF_STRIDE;
  const real c[3] = {cam[0] - p[0], cam[1] - p[1], cam[2] - p[2]};
  for (int k = 0; k < 9; k++) F[k] = (float)R[k];
  for (int j = 0; j < 3; j++) {
    F[RF_O + j] = (float)(R[j] * c[0] + R[3 + j] * c[1] + R[6 + j] * c[2]);
    F[RF_L + j] = (float)(R[j] * light[0] + R[3 + j] * light[1] + R[6 + j] * light[2]);
  }
  F[15] = 0.0f;
}

MCG_DEV float render_uniform(float x) { return __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(x))); }

namespace {       // (internal linkage, like the other kernels: a text section of its own, placed in definition order)
// qpos: [nq, N] (the engine's state), goal: [3, N].  MOUNTED: the camera rides on body cam_body (see the head of this file).  SCENES (with
// MOUNTED): camera, fovy, light, shading coefficients and colours are environment env's row of `scenes`, not A's; the row's address
// depends on env alone and nothing read from it reaches an address or a loop bound, so any bit pattern in a row gives a bad picture of
// that environment and nothing else.  Arguments an instantiation does not read trail the others, so that each finds its own where they
// were.  (One kernel template, not a shared body behind three kernels: through such a wrapper the two older instantiations came out
// with other instruction streams.)
template <bool MOUNTED, bool SCENES>
__global__ __launch_bounds__(RENDER_LANES) void render_kernel(RenderArgs A, const double* __restrict__ qpos, const double* __restrict__ goal,
                                                              int n, int nq, const mcg_model* __restrict__ Pg, int cam_body, float cam_znear,
                                                              const double* __restrict__ scenes) {
  static_assert(MOUNTED || !SCENES, "per-environment scenes are built on the mounted path");
  extern __shared__ __attribute__((aligned(16))) float lds[];
  const int env = blockIdx.x;
  if (env >= n) return;
  if (A.mask && A.mask[env] == 0) return;                          // workgroup-uniform
  const int tid = threadIdx.x;
  constexpr int HEAD = render_head_floats(MOUNTED, SCENES);

  if (tid == 0) {
    const TrigC T = load_trig();
    real srow[SCENES ? MCG_SCENE_RGB : 1];                         // SCENES: the row's camera, fovy, light and shading coefficients
    const real* cam_pos = A.cam_pos; const real* cam_mat = A.cam_mat; const real* light = A.light;
    if constexpr (SCENES) {
      const double* __restrict__ row = scenes + (size_t)env * MCG_SCENE_ENV_DOUBLES;
      for (int k = 0; k < MCG_SCENE_RGB; k++) srow[k] = row[k];
      cam_pos = srow + MCG_SCENE_CAM_POS; cam_mat = srow + MCG_SCENE_CAM_MAT; light = srow + MCG_SCENE_LIGHT_DIR;
      lds[RENDER_SCN_FOCAL] = (float)(0.5 * A.H / tan(0.5 * srow[MCG_SCENE_FOVY] * 3.14159265358979323846 / 180.0));
      for (int k = 0; k < 4; k++) lds[RENDER_SCN_SHADE + k] = (float)srow[MCG_SCENE_LIGHT_AMBIENT + k];
      for (int k = 0; k < 3; k++) lds[RENDER_SCN_LIGHT + k] = (float)light[k];
      for (int c = 0; c < 6; c++)
        for (int k = 0; k < 4; k++) lds[RENDER_RGB + 4 * c + k] = k < 3 ? (float)(255.0 * row[MCG_SCENE_RGB + 3 * c + k]) : 0.0f;
    }
    real R[9], p[3], R5[9], p5[3];
    // MOUNTED: the bodies' R, p wait as float64 where the faces will lie (lane 0 alone reads them back, before the barrier), the
    // carrier's are kept: the camera's world pose has to be known before any body's camera origin can be parked
    real* const chain = (real*)(lds + HEAD);
    real Rb[9] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0}, pb[3] = {0.0, 0.0, 0.0};
    for (int k = 0; k < 9; k++) R[k] = Pg->base_mat[k];
    for (int k = 0; k < 3; k++) p[k] = Pg->base_pos[k];
    static_for<NB>([&](auto I) { constexpr int i = I;
      if constexpr (PAR[i] != i - 1) {                             // a branch of the gripper: back to link6
        for (int k = 0; k < 9; k++) R[k] = R5[k];
        for (int k = 0; k < 3; k++) p[k] = p5[k];
      }
      real r[3] = {Pg->body[i].r[0], Pg->body[i].r[1], Pg->body[i].r[2]};
      render_joint<AXK[i]>(T, AXS[i], r, qpos[(size_t)i * n + env], R, p);
      if constexpr (i == 5) {
        for (int k = 0; k < 9; k++) R5[k] = R[k];
        for (int k = 0; k < 3; k++) p5[k] = p[k];
      }
      if constexpr (MOUNTED) {
        for (int k = 0; k < 9; k++) chain[12 * i + k] = R[k];
        for (int k = 0; k < 3; k++) chain[12 * i + 9 + k] = p[k];
        if (i == cam_body) {
          for (int k = 0; k < 9; k++) Rb[k] = R[k];
          for (int k = 0; k < 3; k++) pb[k] = p[k];
        }
      } else {
        render_park(A.light, A.cam_pos, lds, i, R, p);
      } });
    static_assert(PAR[6] == 5 && PAR[7] == 6 && PAR[8] == 5 && PAR[9] == 8 && PAR[10] == 5 && PAR[11] == 5, "the chain above");
    real camd[3];                                                  // MOUNTED: the camera's world position
    if constexpr (MOUNTED) {                                       // world <- camera = (world <- body) (body <- camera); cam_body == -1: Rb, pb are the identity
      for (int k = 0; k < 3; k++) {
        camd[k] = pb[k] + Rb[3*k] * cam_pos[0] + Rb[3*k+1] * cam_pos[1] + Rb[3*k+2] * cam_pos[2];
        lds[RENDER_CAM + k] = (float)camd[k];
        for (int j = 0; j < 3; j++)
          lds[RENDER_CAM_MAT + 3*k + j] = (float)(Rb[3*k] * cam_mat[j] + Rb[3*k+1] * cam_mat[3 + j] + Rb[3*k+2] * cam_mat[6 + j]);
      }
      lds[RENDER_CAM + 3] = 0.0f;
      for (int k = 9; k < 12; k++) lds[RENDER_CAM_MAT + k] = 0.0f;
      for (int i = 0; i < NB; i++) render_park(light, camd, lds, i, chain + 12 * i, chain + 12 * i + 9);
    }
    if (A.draw_cube) {                                             // nq == 19: the free joint's position and quaternion (normalised as mj_kinematics does)
      real q[4], Rc[9], pc[3];
      for (int k = 0; k < 3; k++) pc[k] = qpos[(size_t)(NB + k) * n + env];
      for (int k = 0; k < 4; k++) q[k] = qpos[(size_t)(NB + 3 + k) * n + env];
      const real nn = sqrt(q[0]*q[0] + q[1]*q[1] + q[2]*q[2] + q[3]*q[3]);
      const bool tiny = nn < MINVAL;
      for (int k = 0; k < 4; k++) q[k] = tiny ? (k == 0 ? 1.0 : 0.0) : q[k] / nn;
      quat_to_mat(q, Rc);
      render_park(light, MOUNTED ? camd : A.cam_pos, lds, NB, Rc, pc);
    } else {
      for (int k = 0; k < RF_STRIDE; k++) lds[NB * RF_STRIDE + k] = 0.0f;
    }
  }
  if (tid >= 64 && tid < 64 + NMESH * RENDER_BOX_FLOATS) {          // the meshes' bounding boxes, a little wider
    const int m = (tid - 64) / RENDER_BOX_FLOATS, k = (tid - 64) % RENDER_BOX_FLOATS;
    lds[RENDER_FRAMES * RF_STRIDE + m * RENDER_BOX_FLOATS + k] = k < 6 ? (float)Pg->mesh_box[m][k] + (k >= 3 ? RENDER_BOX_SLACK : 0.0f) : 0.0f;
  }
  if constexpr (!SCENES)
    if (tid >= 192 && tid < 192 + 24) lds[RENDER_RGB + tid - 192] = ((tid - 192) & 3) < 3 ? A.rgb[(tid - 192) >> 2][(tid - 192) & 3] : 0.0f;
  __syncthreads();
  {   // the faces, with the camera folded in
    float4* lf = (float4*)(lds + HEAD);
    const int total = A.foff[NMESH];
    for (int k = tid; k < total; k += RENDER_LANES) {
      int m = 0;
      _Pragma("unroll") for (int j = 1; j < NMESH; j++) m += (k >= A.foff[j]) ? 1 : 0;
      const float* F = lds + mesh_body(m) * RF_STRIDE;
      float4 f = A.faces[k];
      f.w = f.w - (f.x * F[RF_O] + f.y * F[RF_O + 1] + f.z * F[RF_O + 2]);
      lf[k] = f;
    }
  }
  __syncthreads();

  // MOUNTED: the camera from the LDS head, once per wave, into uniform registers
  float camm[3] = {0.0f, 0.0f, 0.0f}, cmat[9] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (MOUNTED) {
    for (int k = 0; k < 3; k++) camm[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lds[RENDER_CAM + k])));
    for (int k = 0; k < 9; k++) cmat[k] = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(lds[RENDER_CAM_MAT + k])));
  }
  const float* const cm = MOUNTED ? cmat : A.cam_matf;
  const float camw[3] = {MOUNTED ? camm[0] : (float)A.cam_pos[0], MOUNTED ? camm[1] : (float)A.cam_pos[1], MOUNTED ? camm[2] : (float)A.cam_pos[2]};
  // SCENES: the focal length, the shading coefficients and the light from the head as well
  // (read through accessors at the places of use: the two other instantiations then read A where they always did)
  float scn[5] = {0.0f, 0.0f, 0.0f, 0.0f, 0.0f};
  if constexpr (SCENES) for (int k = 0; k < 5; k++) scn[k] = render_uniform(lds[RENDER_SCN + k]);
  static_assert(RENDER_SCN_FOCAL == RENDER_SCN && RENDER_SCN_SHADE == RENDER_SCN + 1, "scn[]: focal, la, ld, ha, hd");
  auto focal = [&]() -> float { if constexpr (SCENES) return scn[0]; else return A.focal; };
  auto la = [&]() -> float { if constexpr (SCENES) return scn[1]; else return A.la; };
  auto ld = [&]() -> float { if constexpr (SCENES) return scn[2]; else return A.ld; };
  auto ha = [&]() -> float { if constexpr (SCENES) return scn[3]; else return A.ha; };
  auto hd = [&]() -> float { if constexpr (SCENES) return scn[4]; else return A.hd; };
  const float lightw[3] = {SCENES ? render_uniform(lds[RENDER_SCN_LIGHT]) : (float)A.light[0], SCENES ? render_uniform(lds[RENDER_SCN_LIGHT + 1]) : (float)A.light[1],
                           SCENES ? render_uniform(lds[RENDER_SCN_LIGHT + 2]) : (float)A.light[2]};
  float tpos[3], table_c[3], table_h[3], cube_h[3];
  for (int k = 0; k < 3; k++) {
    tpos[k] = (float)(A.target_at_goal ? goal[(size_t)k * n + env] : Pg->target0[k]);
    table_c[k] = (float)Pg->table_pos[k]; table_h[k] = (float)Pg->table_half[k]; cube_h[k] = (float)Pg->cube_half[k];
  }

  const int W = A.W, H = A.H, S = A.S;
  const int wave = tid >> 6, lane = tid & 63;
  const int tiles_x = (W + 15) >> 4, tiles_y = (H + 15) >> 4;
  const float inv_s = 1.0f / (float)S, inv_ss = inv_s * inv_s;
  const bool want_centre = (A.out.depth || A.out.geom);
  const bool dwords = A.dwords != 0;
  const size_t img = (size_t)env * H * W;
  // a wave's tile passes through LDS: rays are traced in four compact 8 x 8 blocks (what a wave-wide ballot culls is a mesh that no ray
  // of 64 NEIGHBOURING pixels meets: an 8 x 8 block does that four times as finely as every fourth pixel of 16 x 16), the stores want four
  // consecutive pixels of a row per lane
  uint32_t* tile_px = (uint32_t*)(lds + HEAD + 4 * A.foff[NMESH]) + wave * (3 * 256);      // per pixel: r g b gray | depth | geom
  const int ntiles = tiles_x * tiles_y;
  for (int tile0 = 0; tile0 < ntiles; tile0 += RENDER_LANES / 64) {        // the same trip count for the four waves: barriers inside
    const int tile = tile0 + wave;
    const bool live = tile < ntiles;                                          // wave-uniform
    const int tx = (tile % tiles_x) * 16, ty = (tile / tiles_x) * 16;
    if (live) for (int j = 0; j < 4; j++) {
      const int px_t = ((j >> 1) * 8 + (lane >> 3)) * 16 + (j & 1) * 8 + (lane & 7);      // this lane's pixel of block j, in the tile
      const int x = tx + (px_t & 15), y = ty + (px_t >> 4);
      float sr = 0.0f, sg = 0.0f, sb = 0.0f, sy = 0.0f, dep1 = INFINITY; int gid1 = -1;
      const int nray = S * S + ((S > 1 && want_centre) ? 1 : 0);   // wave-uniform; the last ray of S > 1 is the pixel's centre
      for (int s = 0; s < nray; s++) {
        const bool centre_only = s == S * S;
        const float fx = centre_only ? 0.5f : ((float)(s % S) + 0.5f) * inv_s, fy = centre_only ? 0.5f : ((float)(s / S) + 0.5f) * inv_s;
        const float u = (float)x + fx - 0.5f * (float)W, v = -((float)y + fy - 0.5f * (float)H);
        const float rn = __frsqrt_rn(u * u + v * v + focal() * focal());
        const float dc[3] = {u * rn, v * rn, -focal() * rn};
        float dw[3];
        for (int k = 0; k < 3; k++) dw[k] = cm[3*k] * dc[0] + cm[3*k+1] * dc[1] + cm[3*k+2] * dc[2];
        // depth along the camera's -z = t * focal * rn: the near plane as a distance along this ray
        const float tnear = MOUNTED ? cam_znear * __builtin_amdgcn_rcpf(focal() * rn) : 0.0f;
        const RayHit h = trace<MOUNTED, SCENES>(A, lds, camw, lightw, tpos, table_c, table_h, cube_h, dw, tnear);
        if (centre_only || S == 1) { dep1 = h.id < 0 ? INFINITY : h.t * focal() * rn; gid1 = h.id; }
        if (!centre_only) {
          const int ci = h.id < 0 ? 5 : (h.id < 4 ? h.id : 4);
          const float shade = h.id < 0 ? 1.0f : la() + ld() * fmaxf(0.0f, h.nl) + ha() + hd() * fmaxf(0.0f, h.nd);
          const float* col = lds + RENDER_RGB + 4 * ci;
          const float r = fminf(col[0] * shade, 255.0f), g = fminf(col[1] * shade, 255.0f), b = fminf(col[2] * shade, 255.0f);
          sr += r; sg += g; sb += b;
          sy += 0.114f * r + 0.587f * g + 0.299f * b;               // cv2.COLOR_BGR2GRAY applied to an RGB frame (utils.py:591)
        }
      }
      const uint32_t r8 = (uint32_t)floorf(sr * inv_ss + 0.5f), g8 = (uint32_t)floorf(sg * inv_ss + 0.5f), b8 = (uint32_t)floorf(sb * inv_ss + 0.5f);
      const uint32_t y8 = (uint32_t)fminf(floorf(sy * inv_ss + 0.5f), 255.0f);
      tile_px[px_t] = r8 | (g8 << 8) | (b8 << 16) | (y8 << 24);
      tile_px[256 + px_t] = __float_as_uint(dep1);
      tile_px[512 + px_t] = (uint32_t)gid1;
    }
    __syncthreads();
    const int x0 = tx + (lane & 3) * 4, y = ty + (lane >> 2);
    float cr[4], cg[4], cb[4], gy[4], dep[4]; int gid[4];
    for (int j = 0; j < 4; j++) {
      const int px_t = (lane >> 2) * 16 + (lane & 3) * 4 + j;
      const uint32_t c = tile_px[px_t];
      cr[j] = (float)(c & 255u); cg[j] = (float)((c >> 8) & 255u); cb[j] = (float)((c >> 16) & 255u); gy[j] = (float)(c >> 24);
      dep[j] = __uint_as_float(tile_px[256 + px_t]); gid[j] = (int)tile_px[512 + px_t];
    }
    __syncthreads();                                                          // the next pass overwrites the tile
    if (!live) continue;
    if (y >= H || x0 >= W) continue;
    const size_t px = img + (size_t)y * W + x0;
    if (dwords) {                                                   // x0 + 3 < W, and every row starts on a dword: whole dwords leave
      if (A.out.rgb) {
        const uint32_t b[12] = {(uint32_t)cr[0], (uint32_t)cg[0], (uint32_t)cb[0], (uint32_t)cr[1], (uint32_t)cg[1], (uint32_t)cb[1],
                                (uint32_t)cr[2], (uint32_t)cg[2], (uint32_t)cb[2], (uint32_t)cr[3], (uint32_t)cg[3], (uint32_t)cb[3]};
        uint32_t* dst = (uint32_t*)(A.out.rgb + 3 * px);
        for (int k = 0; k < 3; k++) dst[k] = b[4*k] | (b[4*k+1] << 8) | (b[4*k+2] << 16) | (b[4*k+3] << 24);
      }
      if (A.out.gray) *(uint32_t*)(A.out.gray + px) = (uint32_t)gy[0] | ((uint32_t)gy[1] << 8) | ((uint32_t)gy[2] << 16) | ((uint32_t)gy[3] << 24);
      if (A.out.depth) *(float4*)(A.out.depth + px) = make_float4(dep[0], dep[1], dep[2], dep[3]);
      if (A.out.geom) *(uint32_t*)(A.out.geom + px) = (uint32_t)(gid[0] & 255) | ((uint32_t)(gid[1] & 255) << 8) | ((uint32_t)(gid[2] & 255) << 16) | ((uint32_t)(gid[3] & 255) << 24);
    } else {
      for (int j = 0; j < 4; j++) {
        if (x0 + j >= W) break;
        if (A.out.rgb) { uint8_t* d = A.out.rgb + 3 * (px + j); d[0] = (uint8_t)cr[j]; d[1] = (uint8_t)cg[j]; d[2] = (uint8_t)cb[j]; }
        if (A.out.gray) A.out.gray[px + j] = (uint8_t)gy[j];
        if (A.out.depth) A.out.depth[px + j] = dep[j];
        if (A.out.geom) A.out.geom[px + j] = (int8_t)gid[j];
      }
    }
  }
}

}  // namespace
}  // namespace mcg
