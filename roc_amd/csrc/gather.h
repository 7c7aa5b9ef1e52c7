// 16-B row-gather helpers shared by the row-team CSR kernels that read
// feature rows through colidx (spmm.hip, seg_max.hip).
#pragma once

#include "row_team.h"

namespace {

// raw 16-B gather payload: unpacking is deferred to accumulate time so
// an in-flight slot costs 4 VGPRs, not 8 (occupancy = latency hiding)
template <typename T>
struct RawVec { using type = float4; };
template <>
struct RawVec<unsigned short> { using type = uint4; };

__device__ __forceinline__ uint4 load_raw(const unsigned short* p) {
  return *reinterpret_cast<const uint4*>(p);
}
__device__ __forceinline__ float4 load_raw(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}

typedef __attribute__((ext_vector_type(4))) float f32x4v;

// Two gather engines: plain global loads (64-bit addressing), and SRSRC
// buffer loads with 32-bit offsets when the matrix fits 4 GB — fewer
// address VGPRs = more waves in flight on a latency-bound kernel
// (CDNA guide T8/T20; the descriptor is built from kernargs only, so no
// waterfall loops).
template <typename T>
struct GlobalGather {
  const T* x;
  int64_t D;
  int64_t col0;
  __device__ __forceinline__ typename RawVec<T>::type load(int u) const {
    return load_raw(x + (int64_t)u * D + col0);
  }
};

template <typename T>
struct BufferGather {
  __amdgpu_buffer_rsrc_t rsrc;
  unsigned dbytes;    // D * sizeof(T)
  unsigned colbytes;  // col0 * sizeof(T)
  __device__ __forceinline__ typename RawVec<T>::type load(int u) const {
    const f32x4v v = __builtin_amdgcn_raw_buffer_load_b128(
        rsrc, (unsigned)u * dbytes + colbytes, 0, 0);
    return __builtin_bit_cast(typename RawVec<T>::type, v);
  }
};

// One rung of the unroll ladder: read N column indices, issue N gathers
// into statically indexed slots (fully unrolled, so nothing is scratch),
// then hand the payloads to `use(i, u_i, r_i)` in ascending edge order.
template <int N, typename T, typename LD, typename USE>
__device__ __forceinline__ void gather_group(
    const LD& ld, const int* __restrict__ colidx, int64_t e, USE&& use) {
  int u[N];
  typename RawVec<T>::type r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = ld.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) use(i, u[i], r[i]);
}

}  // namespace
