// Counter-based Philox4x32-10 (Salmon et al., SC'11), the one copy the
// stateless masks share: dropout.hip (feature dropout) and spmm_drop.hip
// (DropEdge). The counter is (idx lo, idx hi, offset, stream), the key is the
// 64-bit seed. `stream` separates the consumers: with the same seed and the
// same call offset, the feature mask and the edge mask are independent draws.
#pragma once

#include "common.h"

constexpr unsigned kPhiloxFeatureStream = 0x9E3779B9u;  // dropout.hip
constexpr unsigned kPhiloxEdgeStream = 0x7F4A7C15u;     // spmm_drop.hip

__device__ __forceinline__ uint2 philox_round(uint2 ctr01, uint2 ctr23,
                                              uint2 key, uint2* out23) {
  // one round of philox4x32
  const unsigned M0 = 0xD2511F53u, M1 = 0xCD9E8D57u;
  unsigned hi0 = __umulhi(M0, ctr01.x), lo0 = M0 * ctr01.x;
  unsigned hi1 = __umulhi(M1, ctr23.x), lo1 = M1 * ctr23.x;
  uint2 r01 = make_uint2(hi1 ^ ctr01.y ^ key.x, lo1);
  uint2 r23 = make_uint2(hi0 ^ ctr23.y ^ key.y, lo0);
  *out23 = r23;
  return r01;
}

__device__ __forceinline__ uint4 philox4x32_10(
    unsigned long long idx, unsigned offset, unsigned long long seed,
    unsigned stream = kPhiloxFeatureStream) {
  uint2 key = make_uint2((unsigned)seed, (unsigned)(seed >> 32));
  uint2 c01 = make_uint2((unsigned)idx, (unsigned)(idx >> 32));
  uint2 c23 = make_uint2(offset, stream);
  const unsigned W0 = 0x9E3779B9u, W1 = 0xBB67AE85u;
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    uint2 n23;
    uint2 n01 = philox_round(c01, c23, key, &n23);
    c01 = n01;
    c23 = n23;
    key.x += W0;
    key.y += W1;
  }
  return make_uint4(c01.x, c01.y, c23.x, c23.y);
}

// the call offset of a mask: the device epoch counter, if there is one,
// makes a captured graph draw a fresh stream on every replay
__device__ __forceinline__ unsigned philox_call_offset(
    const long long* __restrict__ counter, unsigned offset) {
  return counter ? (unsigned)(*counter) * 65536u + offset : offset;
}
