// mcg_replay_img.hip -- the off-policy replay buffer of pictures (include/mcg.h: mcg_replay_img_*): a ring that stores every picture
// once, insertion that keeps a time-limit end's last picture apart, and uniform sampling of (picture, action, reward, next picture,
// done) on the device.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  Kernels and C entries are both here.  The
// C side is stateless: every call gets the caller's device pointers in an mcg_replay_img_buf; of mcg_engine.hpp it uses the error
// reporting alone.  This is data movement, and every kernel here is judged by bytes per second; the pixel paths are mcg_pixels.hpp's,
// the ones mcg_rollout.hip's picture kernels run on.
#include <hip/hip_runtime.h>

#include "mcg.h"
#include "mcg_buffer.hpp"        // launched, padded_words, blocks; philox_pair
#include "mcg_pixels.hpp"        // Pix, Src, load_chunk, each_unit, store_u8, quotient_255; check_src, load_width, store_align

using namespace mcg;

namespace {

constexpr int MAX_DRAWS = 256;          // rejection draws per sample
constexpr int ADD_LANES = 256;
constexpr uint32_t TERMINATED = 1u, TIMEOUT = 2u, NO_NEXT = 4u;      // a record's flags

struct Ring {                            // mcg_replay_img_buf as the kernels see it (the pixel plane and the record's shape: Pix)
  uint8_t* fin; long long* ftime; uint32_t* rec; unsigned long long* cnt;
  int n, R, Tm, F;                       // environments, rows (capacity + 1), time limit, rows of finals
};

MCG_DEV uint4* pixel_row(const Pix& X, const Ring& B, uint8_t* plane, int row, int e) {
  return reinterpret_cast<uint4*>(plane + ((size_t)row * B.n + e) * X.P);
}

// ------------------------------------------------------------------------------------------------------------ start
// Lane = 16 bytes of row `row` of pixels, environments neighbours: the grid writes one contiguous run.  One more lane per environment,
// after the pixels, marks the record of the transition before (row `prev`; < 0: there is none) as having lost its next picture.
template <int W>
__global__ __launch_bounds__(ADD_LANES) void replay_img_start_kernel(Ring B, Pix X, int row, int prev, Src S, const uint8_t* __restrict__ mask) {
  const int c16 = X.P >> 4;
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, npix = (long long)B.n * c16;
  if (x >= npix + B.n) return;
  const int e = x < npix ? (int)(x / c16) : (int)(x - npix);
  if (mask && mask[e] == 0) return;
  if (x < npix) {
    const int q = (int)(x % c16);
    pixel_row(X, B, X.px, row, e)[q] = load_chunk<W>(X, S, e, q * 16);
  } else if (prev >= 0) {
    uint32_t* flags = B.rec + ((size_t)prev * B.n + e) * X.rw + X.A + 1;
    const uint32_t f = *flags;
    if ((f & (TERMINATED | TIMEOUT)) == 0) *flags = f | NO_NEXT;
  }
}

// -------------------------------------------------------------------------------------------------------------- add
// Lane = 16 bytes of row `next` of pixels, as above; where the time limit alone ended environment e's episode the same lane copies
// the same 16 bytes of the finished episode's last picture into row `frow` of finals, so every pixel is read and written once.  After
// the pixels, per environment, one lane per 16 bytes of its record (row `row`) and one for the stamp of its finals row.
template <int W>
__global__ __launch_bounds__(ADD_LANES) void replay_img_add_kernel(Ring B, Pix X, long long a, int row, int next, int frow, Src S, Src Fs,
                                                                   const float* __restrict__ actions, const double* __restrict__ reward,
                                                                   const uint8_t* __restrict__ terminated,
                                                                   const uint8_t* __restrict__ truncated) {
  const int c16 = X.P >> 4, r16 = X.rw >> 2;
  const long long x = (long long)blockIdx.x * ADD_LANES + threadIdx.x, npix = (long long)B.n * c16;
  if (x < npix) {
    const int e = (int)(x / c16), q = (int)(x % c16);
    const bool timeout = truncated[e] != 0 && terminated[e] == 0;
    pixel_row(X, B, X.px, next, e)[q] = load_chunk<W>(X, S, e, q * 16);
    if (timeout) pixel_row(X, B, B.fin, frow, e)[q] = load_chunk<W>(X, Fs, e, q * 16);
    return;
  }
  const long long y = x - npix;
  if (y >= (long long)B.n * (r16 + 1)) return;
  const int e = (int)(y / (r16 + 1)), q = (int)(y % (r16 + 1));
  const bool term = terminated[e] != 0, timeout = truncated[e] != 0 && !term;
  if (q == r16) {
    if (timeout) B.ftime[(size_t)frow * B.n + e] = a;
    return;
  }
  uint32_t w[4];
#pragma unroll
  for (int k = 0; k < 4; k++) {          // action[A], reward, flags, zeros
    const int i = 4 * q + k;
    w[k] = i < X.A ? __float_as_uint(actions[(size_t)e * X.A + i])
         : i == X.A ? __float_as_uint((float)reward[e])
         : i == X.A + 1 ? (term ? TERMINATED : 0u) | (timeout ? TIMEOUT : 0u) : 0u;
  }
  reinterpret_cast<uint4*>(B.rec)[((size_t)row * B.n + e) * r16 + q] = make_uint4(w[0], w[1], w[2], w[3]);
}

// ----------------------------------------------------------------------------------------------------------- sample
struct Batch { uint8_t *pix, *npix; float *pix_f32, *npix_f32, *act, *rew, *done; int32_t* index; };

// One sample per wave, four per block, as mcg_rollout.hip's img_gather_kernel and for its reason.  The index phase is wave-uniform:
// every lane makes the wave's draws and reads the drawn record's flags, so neither the rows nor the flags need a broadcast.  The two
// pictures of the sample then go through one copy loop as 2 * per units, the first picture's units before the next picture's: with
// IMG_FLIGHT loads in flight per lane, a 4 KB picture and its successor are both in flight before the first store.
// ALIGN: as img_gather_kernel's, over the rows of both uint8 and of both float32 outputs.
template <int ALIGN>
__global__ __launch_bounds__(SAMPLE_LANES) void replay_img_sample_kernel(Ring B, Pix X, long long n_written, int Wn, uint32_t base,
                                                                         unsigned long long seed, unsigned long long call, int batch,
                                                                         Batch O) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * (SAMPLE_LANES / 64) + (threadIdx.x >> 6);   // wave-uniform; the output row of this wave
  if (k >= batch) return;
  // ---- index phase: the first draw whose record still has its next picture
  const uint32_t c1 = (uint32_t)call, c3 = DOMAIN_REPLAY_IMG ^ ((uint32_t)(call >> 32) << 8);
  int j = 0, e = 0, row = 0;
  uint32_t flags = NO_NEXT;
  for (int d = 0; d < MAX_DRAWS && (flags & NO_NEXT) != 0; d++) {
    double u0, u1;
    philox_pair((uint32_t)k, c1, (uint32_t)d, c3, seed, u0, u1);
    j = (int)floor(u0 * (double)Wn); j = j > Wn - 1 ? Wn - 1 : j;
    e = (int)floor(u1 * (double)B.n); e = e > B.n - 1 ? B.n - 1 : e;
    row = (int)((base + (uint32_t)j) % (uint32_t)B.R);                  // (n_written - Wn + j) % R; base < R, j < R: no overflow
    flags = B.rec[((size_t)row * B.n + e) * X.rw + X.A + 1];
  }
  const bool ok = (flags & NO_NEXT) == 0;
  const long long a = n_written - Wn + j;                               // the transition's absolute time
  int nrow = row + 1 == B.R ? 0 : row + 1, from_finals = 0;
  float done = (flags & TERMINATED) != 0 ? 1.0f : 0.0f;
  bool lost = false;
  if (ok && (flags & TIMEOUT) != 0) {
    const int frow = (int)((a / B.Tm) % B.F);
    if (B.ftime[(size_t)frow * B.n + e] == a) { nrow = frow; from_finals = 1; }
    else { done = 1.0f; lost = true; }   // the final picture was overwritten: a terminal transition, never another episode's picture
  }
  const uint32_t* rec = B.rec + ((size_t)row * B.n + e) * X.rw;
  if (O.act)
    for (int w = lane; w < X.A; w += 64) O.act[(size_t)k * X.A + w] = ok ? __uint_as_float(rec[w]) : 0.0f;
  if (lane == 0) {
    if (O.rew) O.rew[k] = ok ? __uint_as_float(rec[X.A]) : 0.0f;
    if (O.done) O.done[k] = ok ? done : 0.0f;
    if (O.index) {
      O.index[(size_t)k * 3] = ok ? row : -1; O.index[(size_t)k * 3 + 1] = ok ? e : -1; O.index[(size_t)k * 3 + 2] = ok ? from_finals : -1;
    }
    if (!ok) atomicAdd(B.cnt, 1ull);
    if (lost) atomicAdd(B.cnt + 1, 1ull);
  }
  // ---- copy phase
  const uint8_t* from = X.px + ((size_t)row * B.n + e) * X.P;
  const uint8_t* succ = (from_finals ? B.fin : X.px) + ((size_t)nrow * B.n + e) * X.P;
  if (O.pix || O.npix) {
    uint8_t* r0 = O.pix ? O.pix + (size_t)k * X.Pu : nullptr;
    uint8_t* r1 = O.npix ? O.npix + (size_t)k * X.Pu : nullptr;
    const int per = X.P >> 4;
    each_unit<uint4>(lane, 2 * per,
      [&](int q) {
        const bool second = q >= per;
        if (!ok || !(second ? r1 : r0)) return make_uint4(0u, 0u, 0u, 0u);
        return reinterpret_cast<const uint4*>(second ? succ : from)[second ? q - per : q];
      },
      [&](int q, uint4 v) {
        const bool second = q >= per;
        uint8_t* to = second ? r1 : r0;
        if (to) store_u8<ALIGN>(to, X.Pu, second ? q - per : q, v);
      });
  }
  if (O.pix_f32 || O.npix_f32) {
    float* r0 = O.pix_f32 ? O.pix_f32 + (size_t)k * X.Pu : nullptr;
    float* r1 = O.npix_f32 ? O.npix_f32 + (size_t)k * X.Pu : nullptr;
    if constexpr (ALIGN >= 4) {
      const int per = X.Pu >> 2;
      each_unit<uint32_t>(lane, 2 * per,
        [&](int q) {
          const bool second = q >= per;
          if (!ok || !(second ? r1 : r0)) return 0u;
          return reinterpret_cast<const uint32_t*>(second ? succ : from)[second ? q - per : q];
        },
        [&](int q, uint32_t v) {
          const bool second = q >= per;
          float* to = second ? r1 : r0;
          if (to) reinterpret_cast<float4*>(to)[second ? q - per : q] = quotient_255(v);
        });
    } else {
      const int per = X.Pu;
      each_unit<uint8_t>(lane, 2 * per,
        [&](int q) {
          const bool second = q >= per;
          if (!ok || !(second ? r1 : r0)) return (uint8_t)0;
          return (second ? succ : from)[second ? q - per : q];
        },
        [&](int q, uint8_t v) {
          const bool second = q >= per;
          float* to = second ? r1 : r0;
          if (to) to[second ? q - per : q] = (float)v / 255.0f;
        });
    }
  }
}

// --------------------------------------------------------------------------------------------------- sample, stacked
// Unit q of a sample of `per` units per picture -> the picture j = q / per it belongs to and its place p = q - j * per in it.  `inv`
// is 1.0f / per; q / per <= 9, so the float quotient is off by one at the most, and the two compares settle it.
MCG_DEV void picture_of(int q, int per, float inv, int& j, int& p) {
  j = (int)((float)q * inv);
  if (j * per > q) j--;
  else if ((j + 1) * per <= q) j++;
  p = q - j * per;
}

// replay_img_sample_kernel on stacks of ks frames: one sample per wave, the same draws (over Wn = min(n_written, K - (ks - 1))), then
// the depth of the stack: the flags of the ks - 1 <= 7 records before the sample's, walked back to the first episode start.  Every
// lane reads them, so the index phase stays wave-uniform.  The copy phase has ks + 1 source pictures: j = 0 .. ks - 1 is time
// a - (ks - 1 - j), the picture of slot j of the stack, a zero picture where it lies before the episode's start; j = ks is the
// successor or the final picture.  Each is loaded once and stored twice: into slot j of `observations` (j < ks) and into slot j - 1 of
// `next_observations` (j >= 1), which takes zeros from j < ks where the next stack starts an episode.  They go through one copy loop
// as (ks + 1) * per units with IMG_FLIGHT loads in flight per lane; every byte of both outputs is written.
template <int ALIGN>
__global__ __launch_bounds__(SAMPLE_LANES) void replay_img_sample_stacked_kernel(Ring B, Pix X, long long n_written, int Wn, uint32_t base,
                                                                                 unsigned long long seed, unsigned long long call,
                                                                                 int batch, int ks, Batch O) {
  const int lane = threadIdx.x & 63;
  const int k = blockIdx.x * (SAMPLE_LANES / 64) + (threadIdx.x >> 6);   // wave-uniform; the output row of this wave
  if (k >= batch) return;
  // ---- index phase: the first draw whose record still has its next picture
  const uint32_t c1 = (uint32_t)call, c3 = DOMAIN_REPLAY_IMG ^ ((uint32_t)(call >> 32) << 8);
  int j = 0, e = 0, row = 0;
  uint32_t flags = NO_NEXT;
  for (int d = 0; d < MAX_DRAWS && (flags & NO_NEXT) != 0; d++) {
    double u0, u1;
    philox_pair((uint32_t)k, c1, (uint32_t)d, c3, seed, u0, u1);
    j = (int)floor(u0 * (double)Wn); j = j > Wn - 1 ? Wn - 1 : j;
    e = (int)floor(u1 * (double)B.n); e = e > B.n - 1 ? B.n - 1 : e;
    row = (int)((base + (uint32_t)j) % (uint32_t)B.R);                  // (n_written - Wn + j) % R; base < R, j < R: no overflow
    flags = B.rec[((size_t)row * B.n + e) * X.rw + X.A + 1];
  }
  const bool ok = (flags & NO_NEXT) == 0;
  const long long a = n_written - Wn + j;                               // the transition's absolute time
  // the depth: pictures a - depth + 1 .. a belong to the sample's episode.  The ks - 1 records before the sample's and the stamp are
  // loaded together, before any is tested (their rows do not depend on stored content; a - i >= n_written - R + 1 for i < ks: the rows
  // are live, and a row of a time before 0 is read and not used), so the index phase waits for memory twice, not ks + 1 times.
  uint32_t before[7];
#pragma unroll
  for (int i = 0; i < 7; i++) {
    const int r = row - (i + 1) < 0 ? row - (i + 1) + B.R : row - (i + 1);                  // i + 1 < ks <= R - 1
    before[i] = i + 1 < ks ? B.rec[((size_t)r * B.n + e) * X.rw + X.A + 1] : NO_NEXT;
  }
  const int frow = (int)((a / B.Tm) % B.F);
  const long long stamp = B.ftime[(size_t)frow * B.n + e];
  int depth = 1;
#pragma unroll
  for (int i = 0; i < 7; i++)           // picture a - i is no episode start: a - i > 0 and the record of transition a - i - 1 ended nothing
    if (depth == i + 1 && i + 1 < ks && a - i > 0 && (before[i] & (TERMINATED | TIMEOUT | NO_NEXT)) == 0) depth = i + 2;
  int nrow = row + 1 == B.R ? 0 : row + 1, from_finals = 0;
  float done = (flags & TERMINATED) != 0 ? 1.0f : 0.0f;
  bool lost = false;
  if (ok && (flags & TIMEOUT) != 0) {
    if (stamp == a) { nrow = frow; from_finals = 1; }
    else { done = 1.0f; lost = true; }   // the final picture was overwritten: a terminal transition, never another episode's picture
  }
  // the next stack keeps the older frames unless picture a + 1 starts an episode: the final picture belongs to the sample's own
  const bool keep = ok && ((flags & (TERMINATED | TIMEOUT)) == 0 || from_finals != 0);
  const uint32_t* rec = B.rec + ((size_t)row * B.n + e) * X.rw;
  if (O.act)
    for (int w = lane; w < X.A; w += 64) O.act[(size_t)k * X.A + w] = ok ? __uint_as_float(rec[w]) : 0.0f;
  if (lane == 0) {
    if (O.rew) O.rew[k] = ok ? __uint_as_float(rec[X.A]) : 0.0f;
    if (O.done) O.done[k] = ok ? done : 0.0f;
    if (O.index) {
      O.index[(size_t)k * 3] = ok ? row : -1; O.index[(size_t)k * 3 + 1] = ok ? e : -1; O.index[(size_t)k * 3 + 2] = ok ? from_finals : -1;
    }
    if (!ok) atomicAdd(B.cnt, 1ull);
    if (lost) atomicAdd(B.cnt + 1, 1ull);
  }
  // ---- copy phase
  const uint8_t* succ = (from_finals ? B.fin : X.px) + ((size_t)nrow * B.n + e) * X.P;
  // source picture s (nullptr: zeros).  ks - 1 - s < R: capacity >= ks, the host's check
  auto source = [&](int s) -> const uint8_t* {
    if (!ok) return nullptr;
    if (s == ks) return succ;
    const int back = ks - 1 - s;
    if (back >= depth) return nullptr;
    const int r = row - back < 0 ? row - back + B.R : row - back;
    return X.px + ((size_t)r * B.n + e) * X.P;
  };
  const size_t out_row = (size_t)k * ks * X.Pu;                        // a row of an output: ks pictures
  if (O.pix || O.npix) {
    const int per = X.P >> 4;
    const float inv = 1.0f / (float)per;
    each_unit<uint4>(lane, (ks + 1) * per,
      [&](int q) {
        int s, p;
        picture_of(q, per, inv, s, p);
        const uint8_t* from = source(s);
        if (!from || !(s < ks ? (O.pix || (O.npix && s >= 1 && keep)) : O.npix != nullptr)) return make_uint4(0u, 0u, 0u, 0u);
        return reinterpret_cast<const uint4*>(from)[p];
      },
      [&](int q, uint4 v) {
        int s, p;
        picture_of(q, per, inv, s, p);
        if (O.pix && s < ks) store_u8<ALIGN>(O.pix + out_row + (size_t)s * X.Pu, X.Pu, p, v);
        if (O.npix && s >= 1)
          store_u8<ALIGN>(O.npix + out_row + (size_t)(s - 1) * X.Pu, X.Pu, p, s == ks || keep ? v : make_uint4(0u, 0u, 0u, 0u));
      });
  }
  if (O.pix_f32 || O.npix_f32) {
    if constexpr (ALIGN >= 4) {
      const int per = X.Pu >> 2;
      const float inv = 1.0f / (float)per;
      each_unit<uint32_t>(lane, (ks + 1) * per,
        [&](int q) {
          int s, p;
          picture_of(q, per, inv, s, p);
          const uint8_t* from = source(s);
          if (!from || !(s < ks ? (O.pix_f32 || (O.npix_f32 && s >= 1 && keep)) : O.npix_f32 != nullptr)) return 0u;
          return reinterpret_cast<const uint32_t*>(from)[p];
        },
        [&](int q, uint32_t v) {
          int s, p;
          picture_of(q, per, inv, s, p);
          if (O.pix_f32 && s < ks) reinterpret_cast<float4*>(O.pix_f32 + out_row + (size_t)s * X.Pu)[p] = quotient_255(v);
          if (O.npix_f32 && s >= 1)
            reinterpret_cast<float4*>(O.npix_f32 + out_row + (size_t)(s - 1) * X.Pu)[p] = quotient_255(s == ks || keep ? v : 0u);
        });
    } else {
      const int per = X.Pu;
      const float inv = 1.0f / (float)per;
      each_unit<uint8_t>(lane, (ks + 1) * per,
        [&](int q) {
          int s, p;
          picture_of(q, per, inv, s, p);
          const uint8_t* from = source(s);
          if (!from || !(s < ks ? (O.pix_f32 || (O.npix_f32 && s >= 1 && keep)) : O.npix_f32 != nullptr)) return (uint8_t)0;
          return from[p];
        },
        [&](int q, uint8_t v) {
          int s, p;
          picture_of(q, per, inv, s, p);
          if (O.pix_f32 && s < ks) O.pix_f32[out_row + (size_t)s * X.Pu + p] = (float)v / 255.0f;
          if (O.npix_f32 && s >= 1) O.npix_f32[out_row + (size_t)(s - 1) * X.Pu + p] = (float)(s == ks || keep ? v : (uint8_t)0) / 255.0f;
        });
    }
  }
}

// ------------------------------------------------------------------------------------------------------- host side
int check_buf(const mcg_replay_img_buf* b, const char* who) {
  if (!b) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_replay_img_buf", who);
  if (!b->pixels || !b->finals || !b->final_time || !b->records || !b->counters)
    return mcg_fail(MCG_ERR_ARG, "%s: null pointer in mcg_replay_img_buf", who);
  if (b->n_envs < 1 || b->channels < 1 || b->size < 1 || b->act_dim < 1 || b->capacity < 1 || b->max_episode_steps < 1)
    return mcg_fail(MCG_ERR_ARG, "%s: n_envs, channels, size, act_dim, capacity and max_episode_steps must be >= 1", who);
  if (b->channels > 8) return mcg_fail(MCG_ERR_ARG, "%s: channels must be <= 8", who);
  if (b->size > 512) return mcg_fail(MCG_ERR_ARG, "%s: size must be <= 512", who);
  if (((long long)b->capacity + 1) * b->n_envs >= (1ll << 31))
    return mcg_fail(MCG_ERR_ARG, "%s: (capacity + 1) * n_envs must be below 2^31", who);
  if (((uintptr_t)b->pixels & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: pixels is not 16-byte aligned", who);
  if (((uintptr_t)b->finals & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: finals is not 16-byte aligned", who);
  if (((uintptr_t)b->records & 15) != 0) return mcg_fail(MCG_ERR_ARG, "%s: records is not 16-byte aligned", who);
  return MCG_OK;
}

Ring ring(const mcg_replay_img_buf* b) {
  Ring B;
  B.fin = b->finals; B.ftime = reinterpret_cast<long long*>(b->final_time); B.rec = static_cast<uint32_t*>(b->records);
  B.cnt = reinterpret_cast<unsigned long long*>(b->counters);
  B.n = b->n_envs; B.R = b->capacity + 1; B.Tm = b->max_episode_steps;
  B.F = (b->capacity + b->max_episode_steps - 1) / b->max_episode_steps + 1;
  return B;
}

Pix pixels(const mcg_replay_img_buf* b) {
  Pix X;
  X.px = b->pixels; X.SS = b->size * b->size; X.Pu = b->channels * X.SS; X.P = (X.Pu + 15) / 16 * 16;      // Pu <= 8 * 512 * 512
  X.A = b->act_dim; X.rw = padded_words(b->act_dim + 2);
  return X;
}

}  // namespace

extern "C" {

int64_t mcg_replay_img_record_bytes(int act_dim) { return act_dim < 1 ? 0 : (int64_t)padded_words(act_dim + 2) * 4; }

int mcg_replay_img_start(const mcg_replay_img_buf* buf, int64_t n_written, const uint8_t* img, int64_t env_stride, int64_t chan_stride,
                         const uint8_t* mask, void* stream) {
  if (const int rc = check_buf(buf, "mcg_replay_img_start")) return rc;
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "mcg_replay_img_start: n_written < 0");
  if (const int rc = check_src(buf->channels, buf->size, img, env_stride, chan_stride, "mcg_replay_img_start", "img")) return rc;
  const Ring B = ring(buf);
  const Pix X = pixels(buf);
  const Src S = {img, (long long)env_stride, (long long)chan_stride};
  const int row = (int)(n_written % B.R), prev = n_written >= 1 ? (int)((n_written - 1) % B.R) : -1;
  const dim3 grid(blocks((long long)B.n * (X.P / 16) + B.n, ADD_LANES)), block(ADD_LANES);
  switch (load_width(buf->channels, buf->size, img, env_stride, chan_stride)) {
    case 16: hipLaunchKernelGGL(replay_img_start_kernel<16>, grid, block, 0, (hipStream_t)stream, B, X, row, prev, S, mask); break;
    case 4: hipLaunchKernelGGL(replay_img_start_kernel<4>, grid, block, 0, (hipStream_t)stream, B, X, row, prev, S, mask); break;
    default: hipLaunchKernelGGL(replay_img_start_kernel<1>, grid, block, 0, (hipStream_t)stream, B, X, row, prev, S, mask);
  }
  return launched("mcg_replay_img");
}

int mcg_replay_img_add(const mcg_replay_img_buf* buf, int64_t n_written, const float* actions, const uint8_t* img, int64_t env_stride,
                       int64_t chan_stride, const uint8_t* final_img, int64_t final_env_stride, int64_t final_chan_stride,
                       const double* reward, const uint8_t* terminated, const uint8_t* truncated, void* stream) {
  const char* who = "mcg_replay_img_add";
  if (const int rc = check_buf(buf, who)) return rc;
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "%s: n_written < 0", who);
  if (!actions) return mcg_fail(MCG_ERR_ARG, "%s: null actions", who);
  if (!reward || !terminated || !truncated)
    return mcg_fail(MCG_ERR_ARG, "%s: reward, terminated and truncated of the step's output are required", who);
  if (const int rc = check_src(buf->channels, buf->size, img, env_stride, chan_stride, who, "img")) return rc;
  if (const int rc = check_src(buf->channels, buf->size, final_img, final_env_stride, final_chan_stride, who, "final_img")) return rc;
  const Ring B = ring(buf);
  const Pix X = pixels(buf);
  const Src S = {img, (long long)env_stride, (long long)chan_stride};
  const Src Fs = {final_img, (long long)final_env_stride, (long long)final_chan_stride};
  const long long a = n_written;
  const int row = (int)(a % B.R), next = (int)((a + 1) % B.R), frow = (int)((a / B.Tm) % B.F);
  const int w0 = load_width(buf->channels, buf->size, img, env_stride, chan_stride);
  const int w1 = load_width(buf->channels, buf->size, final_img, final_env_stride, final_chan_stride);
  const dim3 grid(blocks((long long)B.n * (X.P / 16) + (long long)B.n * (X.rw / 4 + 1), ADD_LANES)), block(ADD_LANES);
#define MCG_REPLAY_IMG_ADD(W) hipLaunchKernelGGL(replay_img_add_kernel<W>, grid, block, 0, (hipStream_t)stream, B, X, a, row, next, frow, S, \
                                                 Fs, actions, reward, terminated, truncated)
  switch (w0 < w1 ? w0 : w1) {           // one width for both pictures: the narrower
    case 16: MCG_REPLAY_IMG_ADD(16); break;
    case 4: MCG_REPLAY_IMG_ADD(4); break;
    default: MCG_REPLAY_IMG_ADD(1);
  }
#undef MCG_REPLAY_IMG_ADD
  return launched("mcg_replay_img");
}

int mcg_replay_img_sample(const mcg_replay_img_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch,
                          const mcg_replay_img_batch* out, void* stream) {
  const char* who = "mcg_replay_img_sample";
  if (const int rc = check_buf(buf, who)) return rc;
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "%s: n_written < 0", who);
  if (n_written == 0) return mcg_fail(MCG_ERR_ARG, "%s: the buffer is empty (n_written == 0)", who);
  if (batch < 1) return mcg_fail(MCG_ERR_ARG, "%s: batch must be >= 1", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_replay_img_batch", who);
  if (!out->pix && !out->next_pix && !out->pix_f32 && !out->next_pix_f32 && !out->action && !out->reward && !out->done && !out->index)
    return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  const Ring B = ring(buf);
  const Pix X = pixels(buf);
  const int Wn = (int)(n_written < buf->capacity ? n_written : buf->capacity);
  const uint32_t base = (uint32_t)((n_written - Wn) % B.R);
  const Batch O = {out->pix, out->next_pix, out->pix_f32, out->next_pix_f32, out->action, out->reward, out->done, out->index};
  const int align = store_align(X.Pu, (uint64_t)(uintptr_t)out->pix | (uint64_t)(uintptr_t)out->next_pix,
                                (uint64_t)(uintptr_t)out->pix_f32 | (uint64_t)(uintptr_t)out->next_pix_f32);
  const dim3 grid(blocks(batch, SAMPLE_LANES / 64)), block(SAMPLE_LANES);
#define MCG_REPLAY_IMG_SAMPLE(AL) hipLaunchKernelGGL(replay_img_sample_kernel<AL>, grid, block, 0, (hipStream_t)stream, B, X, \
                                                     (long long)n_written, Wn, base, (unsigned long long)seed, (unsigned long long)call, batch, O)
  switch (align) {
    case 16: MCG_REPLAY_IMG_SAMPLE(16); break;
    case 4: MCG_REPLAY_IMG_SAMPLE(4); break;
    default: MCG_REPLAY_IMG_SAMPLE(1);
  }
#undef MCG_REPLAY_IMG_SAMPLE
  return launched("mcg_replay_img");
}

int mcg_replay_img_sample_stacked(const mcg_replay_img_buf* buf, int64_t n_written, uint64_t seed, uint64_t call, int batch, int frame_stack,
                                  const mcg_replay_img_batch* out, void* stream) {
  const char* who = "mcg_replay_img_sample_stacked";
  if (const int rc = check_buf(buf, who)) return rc;
  if (frame_stack < 1 || frame_stack > 8) return mcg_fail(MCG_ERR_ARG, "%s: frame_stack must be in [1, 8]", who);
  if (buf->capacity - (frame_stack - 1) < 1)
    return mcg_fail(MCG_ERR_ARG, "%s: capacity - (frame_stack - 1) must be >= 1: no transition keeps its whole stack in the ring", who);
  if (n_written < 0) return mcg_fail(MCG_ERR_ARG, "%s: n_written < 0", who);
  if (n_written == 0) return mcg_fail(MCG_ERR_ARG, "%s: the buffer is empty (n_written == 0)", who);
  if (batch < 1) return mcg_fail(MCG_ERR_ARG, "%s: batch must be >= 1", who);
  if (!out) return mcg_fail(MCG_ERR_ARG, "%s: null mcg_replay_img_batch", who);
  if (!out->pix && !out->next_pix && !out->pix_f32 && !out->next_pix_f32 && !out->action && !out->reward && !out->done && !out->index)
    return mcg_fail(MCG_ERR_ARG, "%s: all outputs are null", who);
  const Ring B = ring(buf);
  const Pix X = pixels(buf);
  const int window = buf->capacity - (frame_stack - 1);                  // the rows older than it hold history alone
  const int Wn = (int)(n_written < window ? n_written : window);
  const uint32_t base = (uint32_t)((n_written - Wn) % B.R);
  const Batch O = {out->pix, out->next_pix, out->pix_f32, out->next_pix_f32, out->action, out->reward, out->done, out->index};
  const int align = store_align(X.Pu, (uint64_t)(uintptr_t)out->pix | (uint64_t)(uintptr_t)out->next_pix,
                                (uint64_t)(uintptr_t)out->pix_f32 | (uint64_t)(uintptr_t)out->next_pix_f32);
  const dim3 grid(blocks(batch, SAMPLE_LANES / 64)), block(SAMPLE_LANES);
#define MCG_REPLAY_IMG_SAMPLE(AL) hipLaunchKernelGGL(replay_img_sample_stacked_kernel<AL>, grid, block, 0, (hipStream_t)stream, B, X, \
                                                     (long long)n_written, Wn, base, (unsigned long long)seed, (unsigned long long)call, batch, \
                                                     frame_stack, O)
  switch (align) {
    case 16: MCG_REPLAY_IMG_SAMPLE(16); break;
    case 4: MCG_REPLAY_IMG_SAMPLE(4); break;
    default: MCG_REPLAY_IMG_SAMPLE(1);
  }
#undef MCG_REPLAY_IMG_SAMPLE
  return launched("mcg_replay_img");
}

}  // extern "C"
