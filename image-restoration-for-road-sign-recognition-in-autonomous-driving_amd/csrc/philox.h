// philox.h -- the Philox4x32-10 generator shared by the image distortions
// (distort.hip) and training-mode dropout (linear.hip).
#pragma once
#include <stdint.h>

#include <hip/hip_runtime.h>

__device__ __forceinline__ void philox_round(uint32_t &c0, uint32_t &c1, uint32_t &c2, uint32_t &c3,
                                             uint32_t k0, uint32_t k1) {
  const unsigned long long p0 = (unsigned long long)0xD2511F53u * c0;
  const unsigned long long p1 = (unsigned long long)0xCD9E8D57u * c2;
  const uint32_t h0 = (uint32_t)(p0 >> 32), l0 = (uint32_t)p0;
  const uint32_t h1 = (uint32_t)(p1 >> 32), l1 = (uint32_t)p1;
  const uint32_t n0 = h1 ^ c1 ^ k0, n2 = h0 ^ c3 ^ k1;
  c0 = n0; c1 = l1; c2 = n2; c3 = l0;
}

// ten rounds on the counter c under the 64-bit key
__device__ __forceinline__ void philox4(uint32_t c[4], unsigned long long key) {
  uint32_t k0 = (uint32_t)key, k1 = (uint32_t)(key >> 32);
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    philox_round(c[0], c[1], c[2], c[3], k0, k1);
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
}

// the key of call number `step` (0-based) of a stream seeded with `seed`
__device__ __forceinline__ unsigned long long philox_step_key(unsigned long long seed, long long step) {
  return seed ^ (0x9E3779B97F4A7C15ull * (unsigned long long)(step + 1));
}
