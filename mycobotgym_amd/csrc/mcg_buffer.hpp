// mcg_buffer.hpp -- what mcg_replay.hip, mcg_rollout.hip and mcg_replay_img.hip share: the launch check, the size of a record, the carry of the last
// observation, and the copy phase of the two kernels that hand out samples.  Each file's own rule stays in that file.
#pragma once

#include "mcg_engine.hpp"        // mcg_fail; mcg.h
#include "mcg_philox.hpp"        // MCG_DEV, and the generator both files draw from

namespace {

using namespace mcg;

constexpr int SAMPLE_LANES = 256;       // block of a kernel that hands out samples
constexpr int SPW = 16;                 // samples per wave: the index phase runs on lanes 0..SPW-1, the copy phase on all 64
constexpr int SAMPLES_PER_BLOCK = SPW * (SAMPLE_LANES / 64);

inline unsigned blocks(long long total, int per_block) { return (unsigned)((total + per_block - 1) / per_block); }

// `what`: "mcg_her", "mcg_rollout", "mcg_rollout_img" or "mcg_replay_img"
inline int launched(const char* what) {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? MCG_OK : mcg_fail(MCG_ERR_HIP, "%s kernel launch: %s", what, hipGetErrorString(e));
}

// A record is a whole number of 16-byte rows (`words`: its Layout's, padded); a refused shape has no size.
constexpr int padded_words(int words) { return (words + 3) / 4 * 4; }
inline int64_t record_bytes(int obs_dim, int act_dim, int words) { return obs_dim < 1 || act_dim < 1 ? 0 : (int64_t)words * 4; }

// What `add` stores of a carried value: the float32 kept since the last call (`start` seeded it), which the step's float64 then replaces
// (the hardware's round-to-nearest-even conversion).  Each carried element has one lane.
MCG_DEV uint32_t carry(float& kept, double next) {
  const uint32_t bits = __float_as_uint(kept);
  kept = (float)next;
  return bits;
}

// The copy phase of a wave whose index phase has picked SPW records, sample i for output row k0 + i (rows from `count` on do not
// exist): lane = 8 bytes of a record of `pairs` such pairs, four samples' loads in flight.  Both callables run on all 64 lanes.
//   src(u, i, p)      where pair p of sample i, the u-th in flight, is read from; nullptr: nowhere, the pair is zeros
//   emit(u, k, p, v)  the pair's 8 bytes to their place in row k of the outputs
template <class Src, class Emit>
MCG_DEV void copy_phase(int lane, int k0, int count, int pairs, Src src, Emit emit) {
  for (int i0 = 0; i0 < SPW && k0 + i0 < count; i0 += 4) {
    for (int p0 = 0; p0 < pairs; p0 += 64) {
      const int p = p0 + lane;
      uint2 v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const uint32_t* from = src(u, i0 + u, p);
        v[u] = make_uint2(0u, 0u);
        if (k0 + i0 + u < count && from && p < pairs) v[u] = *reinterpret_cast<const uint2*>(from);
      }
#pragma unroll
      for (int u = 0; u < 4; u++) {
        if (!(k0 + i0 + u < count && p < pairs)) continue;
        emit(u, k0 + i0 + u, p, v[u]);
      }
    }
  }
}

}  // namespace
