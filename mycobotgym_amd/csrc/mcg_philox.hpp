// mcg_philox.hpp -- Philox4x32-10, the generator behind every draw on the device: the reset and scene draws (through mcg_dynamics.hpp),
// the replay buffer's sampling and the rollout buffer's permutation (through mcg_buffer.hpp, without the robot dynamics).
#pragma once

#include <cstdint>
#include <hip/hip_runtime.h>

#define MCG_DEV __device__ __forceinline__       // mcg_dynamics.hpp's definition, token for token

namespace mcg {

// The domain byte: the low byte of a counter's last word, which keeps one user's draws apart from every other's under the same seed.
// This is the one list; a new user takes the next number.
enum Domain : uint32_t {
  DOMAIN_RESET = 0,            // reset: the goal's and the cube's place (rng_pair, mcg_hip.hip)
  DOMAIN_PHYSICS = 1,          // reset: the cube's mass and friction (rng_pair)
  DOMAIN_SCENE = 2,            // reset: cameras, light and colours of the pictures (scene_pair, mcg_render.hip)
  DOMAIN_HER = 3,              // the hindsight replay buffer's sampling (her_pair, mcg_replay.hip)
  DOMAIN_ROLLOUT = 4,          // the rollout buffers' permutation of an epoch (mcg_rollout.hip)
  DOMAIN_REPLAY_IMG = 5,       // the picture replay buffer's sampling (mcg_replay_img.hip)
  DOMAIN_POLICY = 6,           // ActorCritic's collection noise (mcg_policy.hip)
  DOMAIN_SAC_ACT = 7,          // SAC: the collection noise (mcg_sac.hip)
  DOMAIN_SAC_TARGET = 8,       // SAC: the next action of the TD target
  DOMAIN_SAC_ACTOR_LOSS = 9,   // SAC: the actor loss's action (mcg_sac_grad.hip)
  DOMAIN_TD3_ACT = 10,         // TD3 / DDPG: the exploration noise (mcg_td3.hip)
  DOMAIN_TD3_TARGET = 11,      // TD3: the target policy's smoothing noise
  DOMAIN_CNN = 12,             // CnnActorCritic's collection noise (mcg_cnn.hip)
};

MCG_DEV void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1, uint32_t* out) {
#pragma unroll
  for (int r = 0; r < 10; r++) {
    uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n1 = (uint32_t)p1;
    uint32_t n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1, n3 = (uint32_t)p0;
    c0 = n0; c1 = n1; c2 = n2; c3 = n3;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  out[0] = c0; out[1] = c1; out[2] = c2; out[3] = c3;
}

// one block keyed by `seed` as two uniforms in [0, 1) of 53 bits each.  The counter layout is the caller's: rng_pair (mcg_hip.hip),
// scene_pair (mcg_render.hip) and her_pair (mcg_replay.hip) each keep their own
MCG_DEV void philox_pair(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, unsigned long long seed, double& u0, double& u1) {
  uint32_t r[4];
  philox4x32_10(c0, c1, c2, c3, (uint32_t)seed, (uint32_t)(seed >> 32), r);
  u0 = (double)((((unsigned long long)r[0] << 32) | r[1]) >> 11) * (1.0 / 9007199254740992.0);
  u1 = (double)((((unsigned long long)r[2] << 32) | r[3]) >> 11) * (1.0 / 9007199254740992.0);
}

}  // namespace mcg
