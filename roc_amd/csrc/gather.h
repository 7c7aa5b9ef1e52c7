// 16-B row-gather helpers shared by the row-team CSR kernels that read
// feature rows through colidx (spmm.hip, seg_max.hip, seg_stats.hip,
// graph_attn.hip):
// the raw payload and its widen, the two gather engines and their
// factory, one rung of the unroll ladder and the ladder itself.
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

// the exact widen of one payload to EPU floats (bf16x8 / f32x4)
__device__ __forceinline__ void unpack(float* v, const uint4& r) {
  v[0] = bf16_lo(r.x); v[1] = bf16_hi(r.x);
  v[2] = bf16_lo(r.y); v[3] = bf16_hi(r.y);
  v[4] = bf16_lo(r.z); v[5] = bf16_hi(r.z);
  v[6] = bf16_lo(r.w); v[7] = bf16_hi(r.w);
}
__device__ __forceinline__ void unpack(float* v, const float4& r) {
  v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}

// one unit of winner edge indices (seg_max.hip, seg_stats.hip)
template <int EPU>
__device__ __forceinline__ void store_arg(int* p, const int (&a)[EPU]) {
#pragma unroll
  for (int q = 0; q < EPU; q += 4)
    *reinterpret_cast<int4*>(p + q) =
        make_int4(a[q], a[q + 1], a[q + 2], a[q + 3]);
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

// The engine BUF names over the matrix at x (row stride ld), at the lane's
// column offset col0. `bytes` is the byte size of THAT matrix (the number
// of records of the descriptor; GatherGeom::bytes on the host side): a
// buffer load past it returns zeros instead of faulting.
template <typename T, bool BUF>
__device__ __forceinline__ auto make_gather(const T* x, unsigned bytes,
                                            int64_t ld, int64_t col0) {
  if constexpr (BUF) {
    return BufferGather<T>{
        __builtin_amdgcn_make_buffer_rsrc((void*)x, (short)0, bytes,
                                          0x00020000),
        (unsigned)(ld * sizeof(T)), (unsigned)(col0 * sizeof(T))};
  } else {
    return GlobalGather<T>{x, ld, col0};
  }
}

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

// The unroll ladder over the edges [e, e1) of one row: groups of 16 (if
// UN >= 16), 8 (if UN >= 8), 4 and 1, so up to UN gathers are in flight
// and a short row or a remainder steps down instead of padding. `e` is the
// caller's int64_t cursor and ends at e1. The trailing argument is the
// group statement: the op's own *_group call on the ROC_LADDER_N edges
// from e on (the constant the ladder declares for it), ascending in e:
//   ROC_EDGE_LADDER(UN, e, e1,
//                   accum_group<ROC_LADDER_N, T, W>(acc, ld, colidx, w, e));
// It is a macro because a function taking the group as a lambda is not
// the same code to the register allocator: that form kept spmm's
// allocation but moved seg_max's backward and most bf16 attention
// kernels, five of them down an occupancy step (profiles/r42).
#define ROC_EDGE_LADDER(UN, e, e1, ...)              \
  do {                                               \
    if constexpr ((UN) >= 16)                        \
      for (; e + 15 < e1; e += 16) {                 \
        constexpr int ROC_LADDER_N = 16;             \
        __VA_ARGS__;                                 \
      }                                              \
    if constexpr ((UN) >= 8)                         \
      for (; e + 7 < e1; e += 8) {                   \
        constexpr int ROC_LADDER_N = 8;              \
        __VA_ARGS__;                                 \
      }                                              \
    for (; e + 3 < e1; e += 4) {                     \
      constexpr int ROC_LADDER_N = 4;                \
      __VA_ARGS__;                                   \
    }                                                \
    for (; e < e1; ++e) {                            \
      constexpr int ROC_LADDER_N = 1;                \
      __VA_ARGS__;                                   \
    }                                                \
  } while (0)

}  // namespace
