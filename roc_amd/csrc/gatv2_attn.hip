// GATv2 dynamic attention over the in-neighbourhood for CDNA4 (Brody et al.
// 2022, PyG's GATv2Conv; the reference has no attention op).
//
// xl  [n_ext, D]     D = heads * dh; the score row AND the value row
// xr  [n_local, D]
// att [heads, dh]    fp32 master, read as fp32
//
// forward   z_e = xl[u_e,h,:] + xr[v,h,:]              e over the edges of row v
//           s_e = sum_j att[h,j] * lrelu(z_e,j)        lrelu(z) = z > 0 ? z : slope*z
//           out[v,h,:] = sum_e softmax_e(s) * xl[u_e,h,:]
//           lse[v,h]   = log sum_e exp(s_e)            fp32 [n_local, heads]
// backward  p_e = exp(s_e - lse),  delta = <dy, out>,  dp_e = <dy, xl[u_e]>,
//           ds_e = p_e * (dp_e - delta),  lrelu'(z) = z > 0 ? 1 : slope
//   dst pass (forward CSR)    dxr[v]  = att * sum_e ds_e * lrelu'(z_e)
//                             datt[h] = sum_v sum_e ds_e * lrelu(z_e)
//   src pass (transpose CSR)  dxl[u]  = sum_k p_k * dy[w_k]
//                                       + att * sum_k ds_k * lrelu'(z_k)
//
// The nonlinearity sits between the sum and the dot with att, so the score
// is neither a source scalar plus a destination scalar (edge_softmax.hip)
// nor a q.K dot product (graph_attn.hip). What it shares with graph_attn is
// the frame: a row team owns one (row, head) pair at a time, blockIdx.y is
// the head, a lane owns one 16-B unit of the head slice, both gather
// engines, the unroll ladder, the online softmax and the two-pass recompute
// backward. What differs: ONE gathered row per edge serves score and value,
// so a slot of the ladder is one payload and the forward runs 16 edges deep;
// and att has a gradient that is reduced over every edge of the graph.
//
// Rules the tests pin:
//  - all arithmetic is fp32 over the exact bf16 widen; out, dxr and dxl are
//    rounded once, at the store
//  - the running maximum is seeded from the row's first group (a flag, not
//    -inf arithmetic); every group rescales; sums run in ascending edge
//    order inside one team, so per-row results do not depend on the grid or
//    on row_order
//  - a row without edges stores out = 0, lse = 0, delta = 0, dxr = 0; a
//    source without out-edges stores dxl = 0
//  - lanes past dh / EPU of a team hold att = xr = dy = 0, so they add 0 to
//    every reduction, and they store nothing (they re-read lane 0's unit)
//  - datt uses no atomics: a lane keeps EPU fp32 partials for its columns
//    over all the rows its team visits; the teams of a block fold through
//    LDS in team order into one row of a [gridDim.x, D] slab; a second
//    kernel folds the slab in a fixed segmented order. One (grid, row
//    order) gives one bit pattern; another row order regroups the fp32
//    sums and may differ by rounding.
// The fast path needs dh % EPU == 0 and dh <= 64 * EPU. Any other dh >= 1
// runs the lane-strided scalar kernels at the end of this file.

#include "csr_launch.h"
#include "gather.h"

// The kernels of this file are compiled without the packed fp32 VALU forms
// (v_pk_add/mul/fma_f32): every fp32 operation here is a scalar-lane one,
// as the rules above are written.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

// Edges in flight per lane. The forward and the dst pass hold one payload
// per edge; the src pass holds two (xr and dy) plus lse and delta, so it
// runs half as deep. docs/KERNELS.md has the resource table: no fast-path
// instantiation spills.
constexpr int kFwdDepth = 16;
constexpr int kDstDepth = 8;
constexpr int kSrcDepth = 8;
constexpr int kColdTeam = 8;
// the datt slab is [blocks, D] fp32: 8 MB at most
constexpr int64_t kSlabBytes = 8 << 20;
constexpr int kFoldCols = 16;
constexpr int kFoldSegs = kBlock / kFoldCols;

__device__ __forceinline__ float lrelu(float z, float slope) {
  return z > 0.f ? z : slope * z;
}

// the lane's partial of a head dot product, a fixed fma chain
template <int EPU>
__device__ __forceinline__ float unit_dot(const float* a, const float* b) {
  float s = a[0] * b[0];
#pragma unroll
  for (int j = 1; j < EPU; ++j) s = fmaf(a[j], b[j], s);
  return s;
}

// the lane's partial of the score: <att, lrelu(xl + xr)> over its unit
template <int EPU>
__device__ __forceinline__ float unit_score(const float* af, const float* rf,
                                            const float* xf, float slope) {
  float s = af[0] * lrelu(xf[0] + rf[0], slope);
#pragma unroll
  for (int j = 1; j < EPU; ++j)
    s = fmaf(af[j], lrelu(xf[j] + rf[j], slope), s);
  return s;
}

template <typename T>
__device__ __forceinline__ void load_unit(float* v, const T* p, bool active) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  unpack(v, load_raw(p));
  if (!active) {
#pragma unroll
    for (int j = 0; j < EPU; ++j) v[j] = 0.f;
  }
}

// the lane's EPU columns of att (fp32, 16-B aligned since dh % EPU == 0)
template <int EPU>
__device__ __forceinline__ void load_att(float* a, const float* p,
                                         bool active) {
#pragma unroll
  for (int j = 0; j < EPU; j += 4) load_f32x4(p + j, a + j);
  if (!active) {
#pragma unroll
    for (int j = 0; j < EPU; ++j) a[j] = 0.f;
  }
}

// A payload is used twice in the forward: for the score, and after the
// group's maximum is known for the fold. Left alone the compiler keeps the
// widened fp32 copy of every bf16 payload of a group live in between (8
// VGPRs a slot instead of 4, an occupancy step at 16 slots). This makes the
// raw payload opaque between the two uses, so the fold widens it again:
// two ALU ops per element, free next to the gather.
__device__ __forceinline__ void widen_again(uint4& r) {
  asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
}
__device__ __forceinline__ void widen_again(float4&) {}  // fp32: no copy

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

struct Softmax {
  float m, l;
  bool first;
};

// N consecutive edges: one gather each, scores, one rescale, then the fold
// in edge order over the same payloads
template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void fwd_group(
    Softmax& st, float* __restrict__ acc, const float* __restrict__ af,
    const float* __restrict__ rf, float slope, const LD& ld,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type x[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = ld.load(u[i]);
  float s[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float xf[EPU];
    unpack(xf, x[i]);
    s[i] = team_reduce_sum<TEAM>(unit_score<EPU>(af, rf, xf, slope));
  }
  float gm = s[0];
#pragma unroll
  for (int i = 1; i < N; ++i) gm = fmaxf(gm, s[i]);
  const float m_new = st.first ? gm : fmaxf(st.m, gm);
  const float f = st.first ? 0.f : __expf(st.m - m_new);
  st.m = m_new;
  st.first = false;
  st.l *= f;
#pragma unroll
  for (int j = 0; j < EPU; ++j) acc[j] *= f;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float p = __expf(s[i] - m_new);
    float xf[EPU];
    widen_again(x[i]);
    unpack(xf, x[i]);
    st.l += p;
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = fmaf(p, xf[j], acc[j]);
  }
}

template <typename T, int TEAM, bool BUF, bool LSE>
__global__ __launch_bounds__(kBlock) void gatv2_attn_fwd_kernel(
    T* __restrict__ out, float* __restrict__ lse, const T* __restrict__ xl,
    const T* __restrict__ xr, const float* __restrict__ att,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int heads, int dh,
    float slope, unsigned xl_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ld = make_gather<T, BUF>(xl, xl_bytes, D, col);
  float af[EPU];
  load_att<EPU>(af, att + col, active);

  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    int64_t e = rowptr[row];
    const int64_t e1 = rowptr[row + 1];
    float rf[EPU], acc[EPU];
    load_unit(rf, xr + (int64_t)row * D + col, active);
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    Softmax st{0.f, 0.f, true};
    ROC_EDGE_LADDER(kFwdDepth, e, e1,
                    fwd_group<ROC_LADDER_N, T, TEAM>(st, acc, af, rf, slope, ld,
                                                     colidx, e));
    // an empty row keeps l = 0 and acc = 0: out = 0, lse = 0
    const float inv = st.first ? 0.f : 1.f / st.l;
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] *= inv;
    if (active) store_vec(out + (int64_t)row * D + col, acc);
    if constexpr (LSE) {
      if (rt.lane == 0)
        lse[(int64_t)row * heads + h] = st.first ? 0.f : st.m + logf(st.l);
    }
  }
}

// ---------------------------------------------------------------------------
// backward, destination-major: delta, dxr and the datt slab
// ---------------------------------------------------------------------------

// acc collects sum_e ds_e * lrelu'(z_e) (att is multiplied in at the
// store); da collects ds_e * lrelu(z_e) across every row of the team
template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void dst_group(
    float* __restrict__ acc, float* __restrict__ da,
    const float* __restrict__ af, const float* __restrict__ rf,
    const float* __restrict__ gf, float slope, float lse, float delta,
    const LD& ld, const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type x[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = ld.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float xf[EPU];
    unpack(xf, x[i]);
    const float s = team_reduce_sum<TEAM>(unit_score<EPU>(af, rf, xf, slope));
    const float dp = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, xf));
    const float ds = __expf(s - lse) * (dp - delta);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float z = xf[j] + rf[j];
      acc[j] = fmaf(ds, z > 0.f ? 1.f : slope, acc[j]);
      da[j] = fmaf(ds, lrelu(z, slope), da[j]);
    }
  }
}

template <typename T, int TEAM, bool BUF>
__global__ __launch_bounds__(kBlock) void gatv2_attn_bwd_dst_kernel(
    T* __restrict__ dxr, float* __restrict__ slab, float* __restrict__ delta,
    const T* __restrict__ dy, const T* __restrict__ out,
    const float* __restrict__ lse, const T* __restrict__ xl,
    const T* __restrict__ xr, const float* __restrict__ att,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int heads, int dh,
    float slope, unsigned xl_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  constexpr int NT = kBlock / TEAM;  // teams per block
  constexpr int W = TEAM * EPU;      // columns a team covers, >= dh
  __shared__ __align__(16) float part[NT][W];

  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ld = make_gather<T, BUF>(xl, xl_bytes, D, col);
  float af[EPU], da[EPU];
  load_att<EPU>(af, att + col, active);
#pragma unroll
  for (int j = 0; j < EPU; ++j) da[j] = 0.f;

  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    int64_t e = rowptr[row];
    const int64_t e1 = rowptr[row + 1];
    const int64_t at = (int64_t)row * D + col;
    float rf[EPU], gf[EPU], of[EPU], acc[EPU];
    load_unit(rf, xr + at, active);
    load_unit(gf, dy + at, active);
    load_unit(of, out + at, active);
    const float dl = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, of));
    const float ls = lse[(int64_t)row * heads + h];
    if (rt.lane == 0) delta[(int64_t)row * heads + h] = dl;
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    ROC_EDGE_LADDER(kDstDepth, e, e1,
                    dst_group<ROC_LADDER_N, T, TEAM>(acc, da, af, rf, gf, slope,
                                                     ls, dl, ld, colidx, e));
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] *= af[j];
    if (active) store_vec(dxr + at, acc);  // the one rounding
  }

  // the block's teams, in team order, into slab[blockIdx.x][h*dh ...]
  const int t = (int)threadIdx.x / TEAM;
#pragma unroll
  for (int j = 0; j < EPU; j += 4)
    store_f32x4(&part[t][rt.lane * EPU + j], &da[j]);
  __syncthreads();
  float* srow = slab + (int64_t)blockIdx.x * D + (int64_t)h * dh;
  for (int c = threadIdx.x; c < dh; c += kBlock) {
    float s = 0.f;
#pragma unroll
    for (int q = 0; q < NT; ++q) s += part[q][c];
    srow[c] = s;
  }
}

// slab [nblocks, D] -> datt [D]. Column c is summed over each of kFoldSegs
// contiguous segments of blocks in ascending block order, then over the
// segments in ascending order: one fixed order per (nblocks, D).
__global__ __launch_bounds__(kBlock) void gatv2_attn_fold_kernel(
    float* __restrict__ datt, const float* __restrict__ slab, int nblocks,
    int64_t D) {
  __shared__ float part[kFoldSegs][kFoldCols];
  const int l = (int)threadIdx.x % kFoldCols;
  const int seg = (int)threadIdx.x / kFoldCols;
  const int64_t c = (int64_t)blockIdx.x * kFoldCols + l;
  const int per = (nblocks + kFoldSegs - 1) / kFoldSegs;
  const int b0 = seg * per;
  const int b1 = b0 + per < nblocks ? b0 + per : nblocks;
  float s = 0.f;
  if (c < D) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += slab[(int64_t)b * D + c];
  }
  part[seg][l] = s;
  __syncthreads();
  if (seg == 0 && c < D) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < kFoldSegs; ++q) tot += part[q][l];
    datt[c] = tot;
  }
}

// ---------------------------------------------------------------------------
// backward, source-major over the transpose CSR: dxl
// ---------------------------------------------------------------------------

// dv collects p_k * dy[w_k]; dz collects ds_k * lrelu'(z_k) (att is
// multiplied in at the store)
template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void src_group(
    float* __restrict__ dv, float* __restrict__ dz,
    const float* __restrict__ af, const float* __restrict__ xf, float slope,
    const float* __restrict__ lse, const float* __restrict__ delta, int heads,
    int h, const LD& ldr, const LD& ldg, const int* __restrict__ t_colidx,
    int64_t k) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int w[N];
  typename RawVec<T>::type rr[N], gr[N];
  float ls[N], dl[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = t_colidx[k + i];
#pragma unroll
  for (int i = 0; i < N; ++i) rr[i] = ldr.load(w[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) gr[i] = ldg.load(w[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ls[i] = lse[(int64_t)w[i] * heads + h];
    dl[i] = delta[(int64_t)w[i] * heads + h];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float rf[EPU], gf[EPU];
    unpack(rf, rr[i]);
    unpack(gf, gr[i]);
    // af and xf of an inactive lane are 0: a negative-side z there would
    // still be multiplied by af = 0
    const float s = team_reduce_sum<TEAM>(unit_score<EPU>(af, rf, xf, slope));
    const float dp = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, xf));
    const float p = __expf(s - ls[i]);
    const float ds = p * (dp - dl[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      dv[j] = fmaf(p, gf[j], dv[j]);
      dz[j] = fmaf(ds, xf[j] + rf[j] > 0.f ? 1.f : slope, dz[j]);
    }
  }
}

template <typename T, int TEAM, bool BUF>
__global__ __launch_bounds__(kBlock) void gatv2_attn_bwd_src_kernel(
    T* __restrict__ dxl, const T* __restrict__ xl, const T* __restrict__ xr,
    const float* __restrict__ att, const T* __restrict__ dy,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int64_t* __restrict__ t_rowptr, const int* __restrict__ t_colidx,
    const int* __restrict__ t_row_order, int num_src, int heads, int dh,
    float slope, unsigned xr_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ldr = make_gather<T, BUF>(xr, xr_bytes, D, col);
  const auto ldg = make_gather<T, BUF>(dy, xr_bytes, D, col);
  float af[EPU];
  load_att<EPU>(af, att + col, active);

  for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
    const int u = t_row_order ? t_row_order[ri] : ri;
    int64_t k = t_rowptr[u];
    const int64_t k1 = t_rowptr[u + 1];
    const int64_t at = (int64_t)u * D + col;
    float xf[EPU], dv[EPU], dz[EPU];
    load_unit(xf, xl + at, active);  // its own row, not a gather
#pragma unroll
    for (int j = 0; j < EPU; ++j) dv[j] = dz[j] = 0.f;
    ROC_EDGE_LADDER(
        kSrcDepth, k, k1,
        src_group<ROC_LADDER_N, T, TEAM>(dv, dz, af, xf, slope, lse, delta,
                                         heads, h, ldr, ldg, t_colidx, k));
#pragma unroll
    for (int j = 0; j < EPU; ++j) dv[j] = fmaf(af[j], dz[j], dv[j]);
    if (active) store_vec(dxl + at, dv);  // the one rounding
  }
}

// ---------------------------------------------------------------------------
// cold path: dh % EPU != 0, or dh > 64 * EPU. A head slice is not 16-B
// aligned, so column j of the head sits on lane j % 8 of a team of 8 and
// every load is a plain scalar one. A lane keeps ONE accumulator: the
// output columns are taken 8 at a time and every such chunk walks the
// row's edges again, recomputing the scores. The dst pass turns the nest
// inside out (chunks outside, rows inside) so that the lane's single datt
// partial of a chunk lives across all the rows of its team.
// ---------------------------------------------------------------------------

// team-wide <a[0:dh], b[0:dh]>, column j on lane j % 8
template <typename T>
__device__ __forceinline__ float cold_dot(const T* __restrict__ a,
                                          const T* __restrict__ b, int dh,
                                          int lane) {
  float s = 0.f;
  for (int j = lane; j < dh; j += kColdTeam)
    s = fmaf(elt_to_f32(a[j]), elt_to_f32(b[j]), s);
  return team_reduce_sum<kColdTeam>(s);
}

// team-wide score of one edge: l = xl[u] head slice, r = xr[v] head slice
template <typename T>
__device__ __forceinline__ float cold_score(const T* __restrict__ l,
                                            const T* __restrict__ r,
                                            const float* __restrict__ a,
                                            int dh, int lane, float slope) {
  float s = 0.f;
  for (int j = lane; j < dh; j += kColdTeam)
    s = fmaf(a[j], lrelu(elt_to_f32(l[j]) + elt_to_f32(r[j]), slope), s);
  return team_reduce_sum<kColdTeam>(s);
}

template <typename T, bool LSE>
__global__ __launch_bounds__(kBlock) void gatv2_attn_fwd_cold_kernel(
    T* __restrict__ out, float* __restrict__ lse, const T* __restrict__ xl,
    const T* __restrict__ xr, const float* __restrict__ att,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    int num_rows, int heads, int dh, float slope) {
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const float* ah = att + (int64_t)h * dh;
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    const int64_t at = (int64_t)row * D + (int64_t)h * dh;
    // the row's maximum and normaliser, online one edge at a time
    float m = 0.f, l = 0.f;
    for (int64_t e = e0; e < e1; ++e) {
      const T* lr = xl + (int64_t)colidx[e] * D + (int64_t)h * dh;
      const float s = cold_score(lr, xr + at, ah, dh, rt.lane, slope);
      const float m_new = e == e0 ? s : fmaxf(m, s);
      l = (e == e0 ? 0.f : l * __expf(m - m_new)) + __expf(s - m_new);
      m = m_new;
    }
    const float inv = e0 < e1 ? 1.f / l : 0.f;
    for (int c = 0; c < dh; c += kColdTeam) {
      const int j = c + rt.lane;
      float acc = 0.f;
      for (int64_t e = e0; e < e1; ++e) {
        const T* lr = xl + (int64_t)colidx[e] * D + (int64_t)h * dh;
        const float s = cold_score(lr, xr + at, ah, dh, rt.lane, slope);
        if (j < dh) acc = fmaf(__expf(s - m), elt_to_f32(lr[j]), acc);
      }
      if (j < dh) f32_to_elt(acc * inv, out + at + j);
    }
    if constexpr (LSE) {
      if (rt.lane == 0)
        lse[(int64_t)row * heads + h] = e0 < e1 ? m + logf(l) : 0.f;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gatv2_attn_bwd_dst_cold_kernel(
    T* __restrict__ dxr, float* __restrict__ slab, float* __restrict__ delta,
    const T* __restrict__ dy, const T* __restrict__ out,
    const float* __restrict__ lse, const T* __restrict__ xl,
    const T* __restrict__ xr, const float* __restrict__ att,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    int num_rows, int heads, int dh, float slope) {
  constexpr int NT = kBlock / kColdTeam;
  __shared__ float part[NT][kColdTeam];
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const float* ah = att + (int64_t)h * dh;
  const int t = (int)threadIdx.x / kColdTeam;
  float* srow = slab + (int64_t)blockIdx.x * D + (int64_t)h * dh;
  for (int c = 0; c < dh; c += kColdTeam) {  // uniform over the block
    const int j = c + rt.lane;
    const float aj = j < dh ? ah[j] : 0.f;
    float da = 0.f;
    for (int row = rt.team; row < num_rows; row += rt.nteams) {
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      const int64_t at = (int64_t)row * D + (int64_t)h * dh;
      const float dl = cold_dot(dy + at, out + at, dh, rt.lane);
      const float ls = lse[(int64_t)row * heads + h];
      if (c == 0 && rt.lane == 0) delta[(int64_t)row * heads + h] = dl;
      const float rj = j < dh ? elt_to_f32(xr[at + j]) : 0.f;
      float acc = 0.f;
      for (int64_t e = e0; e < e1; ++e) {
        const T* lr = xl + (int64_t)colidx[e] * D + (int64_t)h * dh;
        const float s = cold_score(lr, xr + at, ah, dh, rt.lane, slope);
        const float dp = cold_dot(dy + at, lr, dh, rt.lane);
        const float ds = __expf(s - ls) * (dp - dl);
        if (j < dh) {
          const float z = elt_to_f32(lr[j]) + rj;
          acc = fmaf(ds, z > 0.f ? 1.f : slope, acc);
          da = fmaf(ds, lrelu(z, slope), da);
        }
      }
      if (j < dh) f32_to_elt(aj * acc, dxr + at + j);
    }
    // this chunk's datt partials: the block's teams in team order
    part[t][rt.lane] = da;
    __syncthreads();
    if ((int)threadIdx.x < kColdTeam && c + (int)threadIdx.x < dh) {
      float s = 0.f;
#pragma unroll
      for (int q = 0; q < NT; ++q) s += part[q][threadIdx.x];
      srow[c + threadIdx.x] = s;
    }
    __syncthreads();
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void gatv2_attn_bwd_src_cold_kernel(
    T* __restrict__ dxl, const T* __restrict__ xl, const T* __restrict__ xr,
    const float* __restrict__ att, const T* __restrict__ dy,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const int64_t* __restrict__ t_rowptr, const int* __restrict__ t_colidx,
    int num_src, int heads, int dh, float slope) {
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const float* ah = att + (int64_t)h * dh;
  for (int u = rt.team; u < num_src; u += rt.nteams) {
    const int64_t k0 = t_rowptr[u], k1 = t_rowptr[u + 1];
    const int64_t at = (int64_t)u * D + (int64_t)h * dh;
    for (int c = 0; c < dh; c += kColdTeam) {
      const int j = c + rt.lane;
      const float aj = j < dh ? ah[j] : 0.f;
      const float xj = j < dh ? elt_to_f32(xl[at + j]) : 0.f;
      float dv = 0.f, dz = 0.f;
      for (int64_t k = k0; k < k1; ++k) {
        const int w = t_colidx[k];
        const int64_t wt = (int64_t)w * D + (int64_t)h * dh;
        const float s = cold_score(xl + at, xr + wt, ah, dh, rt.lane, slope);
        const float dp = cold_dot(dy + wt, xl + at, dh, rt.lane);
        const float p = __expf(s - lse[(int64_t)w * heads + h]);
        const float ds = p * (dp - delta[(int64_t)w * heads + h]);
        if (j < dh) {
          dv = fmaf(p, elt_to_f32(dy[wt + j]), dv);
          dz = fmaf(ds, xj + elt_to_f32(xr[wt + j]) > 0.f ? 1.f : slope, dz);
        }
      }
      if (j < dh) f32_to_elt(fmaf(aj, dz, dv), dxl + at + j);
    }
  }
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

// ---------------------------------------------------------------------------
// launchers
// ---------------------------------------------------------------------------

// The frame's geometry with a head per column tile, and whether the fast
// kernels serve this dh (the cold ones run teams of kColdTeam, in natural
// row order).
struct AttnGeom {
  bool fast;
  GatherGeom g;
};

template <typename T>
AttnGeom attn_geom(int num_rows, int heads, int dh, size_t gathered_elems) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const bool fast = dh % EPU == 0 && dh <= 64 * EPU;
  return {fast, gather_geom<T>(num_rows, dh / EPU, heads, gathered_elems, true,
                               fast ? 0 : kColdTeam)};
}

const int* attn_order(const c10::optional<torch::Tensor>& order, int64_t n,
                      const AttnGeom& a, const char* what) {
  const int* p = row_order_ptr(order, n, a.g.team, what);
  return a.fast ? p : nullptr;
}

void check_rowstat(const torch::Tensor& t, int64_t n, int64_t heads,
                   const char* what, const char* name) {
  ROC_CHECK_DEV_CONT(t);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.dim() == 2 &&
                  t.size(0) == n && t.size(1) == heads,
              what, ": ", name, " must be fp32 [num_rows, heads]");
}

void check_att(const torch::Tensor& a, int64_t heads, int64_t dh,
               const char* what, const char* name) {
  ROC_CHECK_DEV_CONT(a);
  TORCH_CHECK(a.scalar_type() == torch::kFloat32 && a.dim() == 2 &&
                  a.size(0) == heads && a.size(1) == dh,
              what, ": ", name, " must be fp32 [heads, dh]");
}

// xl [n_ext, D] against xr [n_local, D] and att [heads, dh]; returns dh
int check_inputs(const torch::Tensor& xl, const torch::Tensor& xr,
                 const torch::Tensor& att, int64_t heads, const char* what) {
  check_mat_pair(xl, "xl", xr, "xr", what);
  TORCH_CHECK(xl.scalar_type() == xr.scalar_type(), what,
              ": xl and xr must share a dtype");
  const int64_t D = xr.size(1);
  TORCH_CHECK(heads >= 1 && heads <= 65535 && D >= heads && D % heads == 0,
              what, ": D must be a positive multiple of heads (<= 65535)");
  TORCH_CHECK(D < INT_MAX / 8, what, ": feature dim too large");
  check_att(att, heads, D / heads, what, "att");
  return (int)(D / heads);
}

}  // namespace

void gatv2_attn_fwd(torch::Tensor out, c10::optional<torch::Tensor> lse,
                    torch::Tensor xl, torch::Tensor xr, torch::Tensor att,
                    torch::Tensor rowptr, torch::Tensor colidx,
                    c10::optional<torch::Tensor> row_order, int64_t heads,
                    double slope) {
  const int dh = check_inputs(xl, xr, att, heads, "gatv2_attn_fwd");
  check_like(out, xr, "gatv2_attn_fwd", "out");
  const int num_rows = (int)xr.size(0);
  check_csr(rowptr, colidx, num_rows, "gatv2_attn_fwd");
  float* lsep = nullptr;
  if (lse.has_value()) {
    check_rowstat(*lse, num_rows, heads, "gatv2_attn_fwd", "lse");
    lsep = lse->data_ptr<float>();
  }
  if (num_rows == 0) return;
  if (colidx.numel() == 0) {  // no edge at all: zeros, no launch
    out.zero_();
    if (lsep) lse->zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(xr.scalar_type(), "gatv2_attn_fwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const AttnGeom a =
        attn_geom<T>(num_rows, (int)heads, dh, (size_t)xl.numel());
    const int* order = attn_order(row_order, num_rows, a, "gatv2_attn_fwd");
    dispatch_bool(lsep != nullptr, [&](auto lse_c) {
      if (!a.fast) {
        hipLaunchKernelGGL(
            (gatv2_attn_fwd_cold_kernel<T, decltype(lse_c)::value>), a.g.grid,
            dim3(kBlock), 0, stream, (T*)out.data_ptr(), lsep,
            (const T*)xl.data_ptr(), (const T*)xr.data_ptr(),
            att.data_ptr<float>(), rowptr.data_ptr<int64_t>(),
            colidx.data_ptr<int>(), num_rows, (int)heads, dh, (float)slope);
        return;
      }
      dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
        hipLaunchKernelGGL(
            (gatv2_attn_fwd_kernel<T, decltype(team_c)::value,
                                   decltype(buf_c)::value,
                                   decltype(lse_c)::value>),
            a.g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), lsep,
            (const T*)xl.data_ptr(), (const T*)xr.data_ptr(),
            att.data_ptr<float>(), rowptr.data_ptr<int64_t>(),
            colidx.data_ptr<int>(), order, num_rows, (int)heads, dh,
            (float)slope, a.g.bytes);
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void gatv2_attn_bwd_dst(torch::Tensor dxr, torch::Tensor datt,
                        torch::Tensor delta, torch::Tensor dy,
                        torch::Tensor out, torch::Tensor lse, torch::Tensor xl,
                        torch::Tensor xr, torch::Tensor att,
                        torch::Tensor rowptr, torch::Tensor colidx,
                        c10::optional<torch::Tensor> row_order, int64_t heads,
                        double slope) {
  const int dh = check_inputs(xl, xr, att, heads, "gatv2_attn_bwd_dst");
  check_like(dxr, xr, "gatv2_attn_bwd_dst", "dxr");
  check_like(dy, xr, "gatv2_attn_bwd_dst", "dy");
  check_like(out, xr, "gatv2_attn_bwd_dst", "out");
  check_att(datt, heads, dh, "gatv2_attn_bwd_dst", "datt");
  const int num_rows = (int)xr.size(0);
  check_csr(rowptr, colidx, num_rows, "gatv2_attn_bwd_dst");
  check_rowstat(lse, num_rows, heads, "gatv2_attn_bwd_dst", "lse");
  check_rowstat(delta, num_rows, heads, "gatv2_attn_bwd_dst", "delta");
  if (num_rows == 0) {
    datt.zero_();
    return;
  }
  if (colidx.numel() == 0) {
    dxr.zero_();
    delta.zero_();
    datt.zero_();
    return;
  }
  auto stream = roc_stream();
  const int64_t D = xr.size(1);
  dispatch_elt(xr.scalar_type(), "gatv2_attn_bwd_dst", [&](auto xt) {
    using T = typename decltype(xt)::type;
    AttnGeom a = attn_geom<T>(num_rows, (int)heads, dh, (size_t)xl.numel());
    const int* order =
        attn_order(row_order, num_rows, a, "gatv2_attn_bwd_dst");
    // one slab row per block of a head: cap the grid so the slab stays
    // within kSlabBytes (the rows are grid-strided, so any grid is right)
    const int64_t cap = kSlabBytes / (D * (int64_t)sizeof(float));
    if ((int64_t)a.g.grid.x > cap) a.g.grid.x = (unsigned)(cap < 1 ? 1 : cap);
    const int nblocks = (int)a.g.grid.x;
    // from the torch allocator: capturable, and freed in stream order
    torch::Tensor slab =
        torch::empty({nblocks, D}, xr.options().dtype(torch::kFloat32));
    if (!a.fast) {
      hipLaunchKernelGGL(
          (gatv2_attn_bwd_dst_cold_kernel<T>), a.g.grid, dim3(kBlock), 0,
          stream, (T*)dxr.data_ptr(), slab.data_ptr<float>(),
          delta.data_ptr<float>(), (const T*)dy.data_ptr(),
          (const T*)out.data_ptr(), lse.data_ptr<float>(),
          (const T*)xl.data_ptr(), (const T*)xr.data_ptr(),
          att.data_ptr<float>(), rowptr.data_ptr<int64_t>(),
          colidx.data_ptr<int>(), num_rows, (int)heads, dh, (float)slope);
    } else {
      dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
        hipLaunchKernelGGL(
            (gatv2_attn_bwd_dst_kernel<T, decltype(team_c)::value,
                                       decltype(buf_c)::value>),
            a.g.grid, dim3(kBlock), 0, stream, (T*)dxr.data_ptr(),
            slab.data_ptr<float>(), delta.data_ptr<float>(),
            (const T*)dy.data_ptr(), (const T*)out.data_ptr(),
            lse.data_ptr<float>(), (const T*)xl.data_ptr(),
            (const T*)xr.data_ptr(), att.data_ptr<float>(),
            rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), order,
            num_rows, (int)heads, dh, (float)slope, a.g.bytes);
      });
    }
    hipLaunchKernelGGL(gatv2_attn_fold_kernel,
                       dim3((unsigned)((D + kFoldCols - 1) / kFoldCols)),
                       dim3(kBlock), 0, stream, datt.data_ptr<float>(),
                       slab.data_ptr<float>(), nblocks, D);
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void gatv2_attn_bwd_src(torch::Tensor dxl, torch::Tensor xl, torch::Tensor xr,
                        torch::Tensor att, torch::Tensor dy, torch::Tensor lse,
                        torch::Tensor delta, torch::Tensor t_rowptr,
                        torch::Tensor t_colidx,
                        c10::optional<torch::Tensor> t_row_order,
                        int64_t heads, double slope) {
  const int dh = check_inputs(xl, xr, att, heads, "gatv2_attn_bwd_src");
  check_like(dxl, xl, "gatv2_attn_bwd_src", "dxl");
  check_like(dy, xr, "gatv2_attn_bwd_src", "dy");
  const int num_rows = (int)xr.size(0);
  const int num_src = (int)xl.size(0);
  check_csr(t_rowptr, t_colidx, num_src, "gatv2_attn_bwd_src");
  check_rowstat(lse, num_rows, heads, "gatv2_attn_bwd_src", "lse");
  check_rowstat(delta, num_rows, heads, "gatv2_attn_bwd_src", "delta");
  if (num_src == 0) return;
  if (t_colidx.numel() == 0 || num_rows == 0) {
    dxl.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(xr.scalar_type(), "gatv2_attn_bwd_src", [&](auto xt) {
    using T = typename decltype(xt)::type;
    // the src pass gathers rows of xr and dy, so the buffer spans xr
    const AttnGeom a =
        attn_geom<T>(num_src, (int)heads, dh, (size_t)xr.numel());
    const int* order =
        attn_order(t_row_order, num_src, a, "gatv2_attn_bwd_src");
    if (!a.fast) {
      hipLaunchKernelGGL(
          (gatv2_attn_bwd_src_cold_kernel<T>), a.g.grid, dim3(kBlock), 0,
          stream, (T*)dxl.data_ptr(), (const T*)xl.data_ptr(),
          (const T*)xr.data_ptr(), att.data_ptr<float>(),
          (const T*)dy.data_ptr(), lse.data_ptr<float>(),
          delta.data_ptr<float>(), t_rowptr.data_ptr<int64_t>(),
          t_colidx.data_ptr<int>(), num_src, (int)heads, dh, (float)slope);
      return;
    }
    dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
      hipLaunchKernelGGL(
          (gatv2_attn_bwd_src_kernel<T, decltype(team_c)::value,
                                     decltype(buf_c)::value>),
          a.g.grid, dim3(kBlock), 0, stream, (T*)dxl.data_ptr(),
          (const T*)xl.data_ptr(), (const T*)xr.data_ptr(),
          att.data_ptr<float>(), (const T*)dy.data_ptr(),
          lse.data_ptr<float>(), delta.data_ptr<float>(),
          t_rowptr.data_ptr<int64_t>(), t_colidx.data_ptr<int>(), order,
          num_src, (int)heads, dh, (float)slope, a.g.bytes);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}
