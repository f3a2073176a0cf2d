// mcg_frame_stack.hip -- the act-time half of frame stacking (include/mcg.h: mcg_frame_stack_push): SB3's StackedObservations.update
// on the device, one launch per step.  The caller's stack, uint8 [N, k * Pu], is shifted down one slot in place and takes the step's
// picture in its newest slot; the stacked final observation goes to a second tensor of the same shape.
//
// A translation unit, and so a code object, of its own, for the reason mcg_render.hip gives.  Stateless: of mcg_engine.hpp it uses the
// error reporting alone.  This is data movement, judged by bytes per second: (k + 1) pictures read and 2 k written per environment.
#include <hip/hip_runtime.h>

#include "mcg.h"
#include "mcg_buffer.hpp"        // launched, blocks
#include "mcg_pixels.hpp"        // Pix, Src, load_chunk, store_u8; check_src, load_width, store_align

using namespace mcg;

namespace {

constexpr int PUSH_LANES = 256;
constexpr int MAX_STACK = 8;

// Bytes 16 q .. 16 q + 15 of a row of Pu bytes, the counterpart of store_u8: bytes from Pu on read as zeros.
template <int ALIGN>
MCG_DEV uint4 load_u8(const uint8_t* row, int Pu, int q) {
  const uint8_t* from = row + 16 * q;
  if constexpr (ALIGN == 16) {
    return *reinterpret_cast<const uint4*>(from);
  } else if constexpr (ALIGN == 4) {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (16 * q + 4 * k < Pu) w[k] = reinterpret_cast<const uint32_t*>(from)[k];
    return make_uint4(w[0], w[1], w[2], w[3]);
  } else {
    uint32_t w[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int k = 0; k < 16; k++)
      if (16 * q + k < Pu) w[k >> 2] |= (uint32_t)from[k] << (8 * (k & 3));
    return make_uint4(w[0], w[1], w[2], w[3]);
  }
}

// Lane = one 16-byte position q of one environment's frame, neighbouring lanes on neighbouring positions.  The lane loads slots
// 1 .. k - 1 of its environment at its own position, the same position of `img` and of `final_img`, and only then stores: no other
// lane reads or writes those bytes, so the shift in place has no hazard between lanes, and every byte is read once and written once
// per output.  W: the width of every access (the host's choice: it divides the stack's base and Pu, and what load_chunk asks of the
// two pictures).  fin == nullptr: no final stack.  mask != nullptr: the environments of the mask restart from `img` (older slots
// zeros), the others are left as they are, and `done` is not read.
template <int W>
__global__ __launch_bounds__(PUSH_LANES) void frame_stack_push_kernel(uint8_t* __restrict__ stack, uint8_t* __restrict__ fin, Pix X, int n,
                                                                      int k, Src S, Src Fs, const uint8_t* __restrict__ done,
                                                                      const uint8_t* __restrict__ mask) {
  const int c16 = (X.Pu + 15) >> 4;
  const long long x = (long long)blockIdx.x * PUSH_LANES + threadIdx.x;
  if (x >= (long long)n * c16) return;
  const int e = (int)(x / c16), q = (int)(x % c16);
  if (mask && mask[e] == 0) return;
  const bool fresh = mask ? true : done[e] != 0;
  const size_t row = (size_t)e * k * X.Pu;
  uint4 old[MAX_STACK - 1];
#pragma unroll
  for (int s = 1; s < MAX_STACK; s++)
    if (s < k) old[s - 1] = load_u8<W>(stack + row + (size_t)s * X.Pu, X.Pu, q);
  const uint4 newest = load_chunk<W>(X, S, e, q * 16);
  uint4 last = make_uint4(0u, 0u, 0u, 0u);
  if (fin) last = load_chunk<W>(X, Fs, e, q * 16);
  const uint4 zero = make_uint4(0u, 0u, 0u, 0u);
#pragma unroll
  for (int s = 1; s < MAX_STACK; s++)
    if (s < k) {
      if (fin) store_u8<W>(fin + row + (size_t)(s - 1) * X.Pu, X.Pu, q, old[s - 1]);
      store_u8<W>(stack + row + (size_t)(s - 1) * X.Pu, X.Pu, q, fresh ? zero : old[s - 1]);
    }
  if (fin) store_u8<W>(fin + row + (size_t)(k - 1) * X.Pu, X.Pu, q, last);
  store_u8<W>(stack + row + (size_t)(k - 1) * X.Pu, X.Pu, q, newest);
}

}  // namespace

extern "C" {

int mcg_frame_stack_push(uint8_t* stack, uint8_t* final_stack, int n_envs, int channels, int size, int frame_stack, const uint8_t* img,
                         int64_t env_stride, int64_t chan_stride, const uint8_t* final_img, int64_t final_env_stride,
                         int64_t final_chan_stride, const uint8_t* done, const uint8_t* mask, void* stream) {
  const char* who = "mcg_frame_stack_push";
  if (!stack) return mcg_fail(MCG_ERR_ARG, "%s: null stack", who);
  if (n_envs < 1 || channels < 1 || size < 1) return mcg_fail(MCG_ERR_ARG, "%s: n_envs, channels and size must be >= 1", who);
  if (channels > 8) return mcg_fail(MCG_ERR_ARG, "%s: channels must be <= 8", who);
  if (size > 512) return mcg_fail(MCG_ERR_ARG, "%s: size must be <= 512", who);
  if (frame_stack < 1 || frame_stack > MAX_STACK) return mcg_fail(MCG_ERR_ARG, "%s: frame_stack must be in [1, 8]", who);
  if ((long long)n_envs * ((channels * size * size + 15) / 16) >= (1ll << 31))
    return mcg_fail(MCG_ERR_ARG, "%s: n_envs * ceil(channels * size * size / 16) must be below 2^31", who);
  if (final_stack == stack) return mcg_fail(MCG_ERR_ARG, "%s: final_stack is stack", who);
  if (!done && !mask) return mcg_fail(MCG_ERR_ARG, "%s: null done without a mask", who);
  if (const int rc = check_src(channels, size, img, env_stride, chan_stride, who, "img")) return rc;
  if (final_stack)
    if (const int rc = check_src(channels, size, final_img, final_env_stride, final_chan_stride, who, "final_img")) return rc;
  Pix X;
  X.px = nullptr; X.SS = size * size; X.Pu = channels * X.SS; X.P = (X.Pu + 15) / 16 * 16; X.A = 0; X.rw = 0;      // Pu <= 8 * 512 * 512
  const Src S = {img, (long long)env_stride, (long long)chan_stride};
  const Src Fs = {final_stack ? final_img : img, final_stack ? (long long)final_env_stride : (long long)env_stride,
                  final_stack ? (long long)final_chan_stride : (long long)chan_stride};
  int w = store_align(X.Pu, (uint64_t)(uintptr_t)stack | (uint64_t)(uintptr_t)final_stack, 0u);
  const int w0 = load_width(channels, size, img, env_stride, chan_stride);
  const int w1 = final_stack ? load_width(channels, size, final_img, final_env_stride, final_chan_stride) : 16;
  w = w0 < w ? w0 : w;
  w = w1 < w ? w1 : w;                   // one width for the stacks and both pictures: the narrowest
  const dim3 grid(blocks((long long)n_envs * ((X.Pu + 15) / 16), PUSH_LANES)), block(PUSH_LANES);
#define MCG_FRAME_STACK_PUSH(W) hipLaunchKernelGGL(frame_stack_push_kernel<W>, grid, block, 0, (hipStream_t)stream, stack, final_stack, X, \
                                                   n_envs, frame_stack, S, Fs, done, mask)
  switch (w) {
    case 16: MCG_FRAME_STACK_PUSH(16); break;
    case 4: MCG_FRAME_STACK_PUSH(4); break;
    default: MCG_FRAME_STACK_PUSH(1);
  }
#undef MCG_FRAME_STACK_PUSH
  return launched("mcg_frame_stack");
}

}  // extern "C"
