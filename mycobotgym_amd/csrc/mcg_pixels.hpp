// mcg_pixels.hpp -- the pixel paths that mcg_rollout.hip (mcg_rollout_img_*) and mcg_replay_img.hip (mcg_replay_img_*) share: a
// picture as the caller holds it and its loads at three widths, the copy loop of a kernel that hands out pictures, the stores of a
// uint8 and of a normalised output row, and the host's checks and choices that go with them.  A stored picture is Pix::P bytes (a
// multiple of 16), so every access to a pixel plane is one aligned 16-byte word per lane, 1 KiB contiguous per wave instruction.
#pragma once

#include "mcg_buffer.hpp"

namespace {

constexpr int IMG_FLIGHT = 8;           // loads a lane of a copy loop issues before its first store

struct Pix {                            // a pixel plane and the record that goes with a picture, as the kernels see them
  uint8_t* px;
  int Pu, P, SS;                        // bytes of a picture, of its padded row, of one channel
  int A, rw;                            // action words and words of a record (padded: a multiple of 4)
};
struct Src { const uint8_t* img; long long es, cs; };      // a picture as the caller holds it: base, environment and channel stride in bytes

// Bytes b .. b + 15 (b a multiple of 16) of environment e's picture, channel-major; bytes from Pu on are zeros.  W is the width of a
// load: it divides the base address, both strides and S * S (the host's choice), so no load is misaligned or straddles two channels.
template <int W>
MCG_DEV uint4 load_chunk(const Pix& X, const Src& S, int e, int b) {
  const uint8_t* base = S.img + (long long)e * S.es;
  uint32_t w[4] = {0u, 0u, 0u, 0u};
  if constexpr (W == 16) {
    if (b >= X.Pu) return make_uint4(0u, 0u, 0u, 0u);
    const int c = b / X.SS;
    return *reinterpret_cast<const uint4*>(base + (long long)c * S.cs + (b - c * X.SS));
  } else if constexpr (W == 4) {
#pragma unroll
    for (int k = 0; k < 4; k++) {
      const int bb = b + 4 * k, c = bb / X.SS;
      if (bb < X.Pu) w[k] = *reinterpret_cast<const uint32_t*>(base + (long long)c * S.cs + (bb - c * X.SS));
    }
  } else {
#pragma unroll
    for (int k = 0; k < 16; k++) {
      const int bb = b + k, c = bb / X.SS;
      if (bb < X.Pu) w[k >> 2] |= (uint32_t)base[(long long)c * S.cs + (bb - c * X.SS)] << (8 * (k & 3));
    }
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

// A copy loop: the wave's sample has `per` units (a unit: what one lane loads at once), lane = unit, so a wave instruction covers 64
// consecutive units.  A lane issues IMG_FLIGHT loads before its first store.
//   load(q)      unit q of the sample
//   emit(q, v)   to its place in the sample's row of the output
template <class V, class Load, class Emit>
MCG_DEV void each_unit(int lane, int per, Load load, Emit emit) {
  for (int q0 = 0; q0 < per; q0 += 64 * IMG_FLIGHT) {
    V v[IMG_FLIGHT];
#pragma unroll
    for (int u = 0; u < IMG_FLIGHT; u++)
      if (q0 + 64 * u + lane < per) v[u] = load(q0 + 64 * u + lane);
#pragma unroll
    for (int u = 0; u < IMG_FLIGHT; u++)
      if (q0 + 64 * u + lane < per) emit(q0 + 64 * u + lane, v[u]);
  }
}

// The 16 bytes `v` of unit q to a uint8 output row of Pu bytes.  ALIGN: what divides Pu and the output pointers (the host's choice):
// 16 -- one 16-byte word, 4 -- 4-byte words, 1 -- bytes; bytes from Pu on (the stored picture's padding) are not written.
template <int ALIGN>
MCG_DEV void store_u8(uint8_t* row, int Pu, int q, uint4 v) {
  uint8_t* to = row + 16 * q;
  if constexpr (ALIGN == 16) {
    *reinterpret_cast<uint4*>(to) = v;
  } else if constexpr (ALIGN == 4) {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (16 * q + 4 * k < Pu) reinterpret_cast<uint32_t*>(to)[k] = w[k];
  } else {
    const uint32_t w[4] = {v.x, v.y, v.z, v.w};
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (16 * q + k < Pu) to[k] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
  }
}

// byte / 255 of the four bytes of `v`: the correctly rounded float32 quotient (IEEE division, nothing reciprocal)
MCG_DEV float4 quotient_255(uint32_t v) {
  return make_float4((float)(v & 255u) / 255.0f, (float)((v >> 8) & 255u) / 255.0f, (float)((v >> 16) & 255u) / 255.0f,
                     (float)(v >> 24) / 255.0f);
}

// ------------------------------------------------------------------------------------------------------- host side
inline int check_src(int channels, int size, const uint8_t* img, int64_t env_stride, int64_t chan_stride, const char* who, const char* name) {
  if (!img) return mcg_fail(MCG_ERR_ARG, "%s: null %s", who, name);
  if (env_stride < 0 || chan_stride < 0) return mcg_fail(MCG_ERR_ARG, "%s: a stride is negative", who);
  if (channels > 1 && chan_stride < (int64_t)size * size) return mcg_fail(MCG_ERR_ARG, "%s: chan_stride is below size * size", who);
  return MCG_OK;
}

// the widest load that the picture's base, strides and channel size allow
inline int load_width(int channels, int size, const uint8_t* img, int64_t env_stride, int64_t chan_stride) {
  const uint64_t all = (uint64_t)(uintptr_t)img | (uint64_t)env_stride | (channels > 1 ? (uint64_t)chan_stride : 0u) |
                       (uint64_t)((int64_t)size * size);
  return (all & 15) == 0 ? 16 : (all & 3) == 0 ? 4 : 1;
}

// what divides the rows of a uint8 output (Pu bytes apart: `u8` is the OR of the pointers) and of a float32 one (4 Pu apart)
inline int store_align(int Pu, uint64_t u8, uint64_t f32) {
  const uint64_t all = (uint64_t)Pu | u8;
  const bool f16 = (f32 & 15) == 0;
  return (all & 15) == 0 && f16 ? 16 : (all & 3) == 0 && f16 ? 4 : 1;
}

}  // namespace
