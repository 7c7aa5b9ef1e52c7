// CSR softmax aggregation for CDNA4: DeeperGCN's aggregator (Li et al. 2020,
// PyG's GENConv / SoftmaxAggregation), a per-COLUMN temperature softmax over
// each in-neighbourhood, out of ONE gather of each neighbour row.
//
// forward   p_e,j    = exp(t*x[u_e,j]) / sum_e' exp(t*x[u_e',j])
//           out[v,j] = sum_e p_e,j * x[u_e,j]               [n_rows, D]
//           stats[v] = [ lse | out32 ]  fp32, unrounded     [n_rows, 2*D]
//                      lse = log sum_e exp(t*(x[u_e,j] - out32[v,j])),
//                      the log-sum-exp of the scores CENTRED on the output
// backward  over the transposed edges k of source u (v = its destination),
//           ascending, with d = x[u] - out32[v], p = exp(t*d - lse[v]):
//             dx[u] = sum_k p * dy[v] * (1 + t*d)
//             dt    = sum over every edge and column of p * dy[v] * d^2
//
// t is a fp32 [1] DEVICE tensor that the kernels read themselves, so a
// captured epoch sees the optimiser's updates. t = 0 is the mean, t -> inf
// the max.
//
// Same frame as seg_stats.hip: a row team owns one row at a time, wide rows
// are column-tiled over blockIdx.y, the gathers go through the shared unroll
// ladder into statically indexed slots. Every column has a softmax of its
// own, so a lane carries an online softmax (m, l, a) per column of its unit
// and the team never reduces. No [E, D] intermediate, no atomic.
//
// Rules the tests pin:
//  - all arithmetic is fp32 over the exact widen, out and dx are rounded
//    once, at the store; exp is __expf, the log is logf
//  - per ladder group and column: gm = max_i t*x_i, m' = max(m, gm),
//    f = exp(m - m'), p_i = exp(fma(t, x_i, -m')), l = l*f + sum p_i,
//    a = a*f + sum p_i*(x_i - x0), ascending in e. x0 is the row's first
//    edge: the weighted sum is shifted as seg_stats shifts its sums, so a
//    row of equal values near 100 gives that value exactly. The first group
//    seeds m and x0 through a flag, never through -inf arithmetic.
//    out = x0 + a/l, lse = fma(-t, out, m) + log(l). The fused
//    multiply-adds keep the products' rounding (2^-24 * |t*x|, 3e-5 at
//    t*x = 800) out of p, here and in the backward's p = exp(fma(t, d, -lse)).
//    A row's result depends on its own edges only: not on the grid, not on
//    row_order.
//  - the saved lse is centred on out32 because the plain one,
//    log sum exp(t*x), is as large as t*x: at 800 its fp32 rounding alone
//    puts 3e-5 of relative error into every p of the backward, and dx of
//    inputs near 100 at t = 8 then misses the project's fp32 tolerance by
//    half. The centred one is of the size of log(deg), d = x[u] - out32[v]
//    is exact for close values, and the rounding of out32 cancels between
//    the two.
//  - stats = None is the same arithmetic without the state stores
//  - the backward reads lse and out32 from the fp32 stats, never from the
//    rounded out (seg_stats's rule)
//  - an empty row stores out = 0 and stats = 0 and passes no gradient; a
//    source without out-edges gets dx = 0; duplicate edges each count
//  - dt uses no atomics: a lane keeps one fp32 partial over all the rows its
//    team visits; a block folds its 256 partials through LDS in a fixed
//    order into one slab entry per (column tile, block); a one-block kernel
//    folds the slab in fixed segments and OVERWRITES dt. One (grid, row
//    order) gives one bit pattern; another row order regroups the fp32 sums
//    and may differ by rounding. dx does not depend on either.
// NaN and +-inf inputs are out of contract.

#include "csr_launch.h"
#include "gather.h"

// Every fp32 operation of this file is a scalar-lane one and none is
// contracted behind the source's back: the variants of a kernel (depth,
// stats or not, dt or not) must round alike.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#pragma clang fp contract(off)

namespace {

// Gathers in flight per lane; the launchers take an override so that
// scripts/bench_seg_softmax.py can repeat the comparison. docs/KERNELS.md
// has the resource table.
// Forward: the state is m, l, a and x0 per column, 32 VGPRs in bf16, and the
// group's maxima 8 more. 8 deep fits 91-96 VGPRs (5 waves per SIMD, 40
// gathers in flight), 16 deep needs 132-142 (3 waves, 48 gathers). The
// report alone favours 8; measured at the Reddit shape in bf16
// (profiles/r49, medians of 20, D=256 / D=64 in ms) 16 deep wins at D=256
// and ties inside the spread at D=64: with stats 8.16 / 10.88 against
// 9.32 / 10.77, without 8.13 / 11.09 against 8.75 / 10.85.
// Backward: a slot holds one dy unit and two fp32 stats units, 10 (bf16) or
// 12 (fp32) VGPRs; 8 deep 40.02 / 8.73 against 4 deep 40.28 / 9.04. 16 deep
// would need 192 VGPRs of slots and is not compiled.
constexpr int kFwdDepth = 16;
constexpr int kBwdDepth = 8;
constexpr int kBwdCols = 4;  // columns per lane of the backward launches
constexpr int kSlabMax = 8192;  // dt slab entries: the backward's grid cap

// the vector paths need 4-B aligned units: every fp32 width, even bf16 ones
template <typename T>
__device__ __forceinline__ bool vec_ok(int64_t D) {
  return (D * sizeof(T)) % 4 == 0;
}

// columns of the `width`-wide unit at col0 that lie inside D
__device__ __forceinline__ int valid_cols(int64_t col0, int64_t D, int width) {
  return col0 >= D ? 0 : (D - col0 < width ? (int)(D - col0) : width);
}

// A payload is used twice, for the group's column maxima and then for the
// fold; see gatv2_attn.hip: without this the compiler keeps the widened fp32
// copy of every bf16 payload of a group live in between.
__device__ __forceinline__ void widen_again(uint4& r) {
  asm volatile("" : "+v"(r.x), "+v"(r.y), "+v"(r.z), "+v"(r.w));
}
__device__ __forceinline__ void widen_again(float4&) {}  // fp32: no copy

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// the online softmax of one lane: one (m, l, a) per column of its unit
template <int EPU>
struct ColSoftmax {
  float m[EPU], l[EPU], a[EPU], x0[EPU];
  bool first;
};

// N consecutive edges: one gather each, the column maxima, one rescale,
// then the fold in edge order over the same payloads
template <int N, typename T, typename LD>
__device__ __forceinline__ void fwd_group(
    ColSoftmax<EltTraits<T>::kPerVec>& st, float t, const LD& ld,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type r[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = ld.load(u[i]);
  float gm[EPU];
  {
    float v[EPU];
    unpack(v, r[0]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      gm[j] = t * v[j];
      if (st.first) st.x0[j] = v[j];
    }
  }
#pragma unroll
  for (int i = 1; i < N; ++i) {
    float v[EPU];
    unpack(v, r[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) gm[j] = fmaxf(gm[j], t * v[j]);
  }
#pragma unroll
  for (int j = 0; j < EPU; ++j) {
    const float m_new = st.first ? gm[j] : fmaxf(st.m[j], gm[j]);
    const float f = st.first ? 0.f : __expf(st.m[j] - m_new);
    st.m[j] = m_new;
    st.l[j] *= f;
    st.a[j] *= f;
  }
  st.first = false;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float v[EPU];
    widen_again(r[i]);
    unpack(v, r[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float p = __expf(fmaf(t, v[j], -st.m[j]));
      st.l[j] += p;
      st.a[j] = fmaf(p, v[j] - st.x0[j], st.a[j]);
    }
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool SAVE>
__global__ __launch_bounds__(kBlock) void seg_softmax_fwd_kernel(
    T* __restrict__ out, float* __restrict__ stats, const T* __restrict__ x,
    const float* __restrict__ tp, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const int* __restrict__ row_order,
    int num_rows, int64_t D, unsigned x_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, EPU);
  const float t = tp[0];

  if (full) {
    const auto g = make_gather<T, BUF>(x, x_bytes, D, col0);
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      int64_t e = rowptr[row];
      const int64_t e1 = rowptr[row + 1];
      ColSoftmax<EPU> st;
#pragma unroll
      for (int j = 0; j < EPU; ++j) st.m[j] = st.l[j] = st.a[j] = st.x0[j] = 0.f;
      st.first = true;
      ROC_EDGE_LADDER(UN, e, e1,
                      fwd_group<ROC_LADDER_N, T>(st, t, g, colidx, e));
      // an empty row keeps first: out = 0, stats = 0
      float o[EPU], lse[EPU];
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        o[j] = st.first ? 0.f : st.x0[j] + st.a[j] / st.l[j];
        if constexpr (SAVE)
          lse[j] = st.first ? 0.f : fmaf(-t, o[j], st.m[j]) + logf(st.l[j]);
      }
      store_vec(out + (int64_t)row * D + col0, o);  // the one rounding
      if constexpr (SAVE) {
        float* s = stats + (int64_t)row * 2 * D + col0;
        store_vec(s, lse);
        store_vec(s + D, o);
      }
    }
  } else if (nvalid > 0) {
    // cold path: the unit straddles D, or the rows are not 4-B aligned
    // (odd bf16 widths). One column at a time, scalar loads, two walks over
    // the row: the maximum first, so nothing is rescaled.
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        float o = 0.f, lse = 0.f;
        if (e0 < e1) {
          const float x0 = elt_to_f32(x[(int64_t)colidx[e0] * D + c]);
          float m = t * x0;
          for (int64_t e = e0 + 1; e < e1; ++e)
            m = fmaxf(m, t * elt_to_f32(x[(int64_t)colidx[e] * D + c]));
          float l = 0.f, a = 0.f;
          for (int64_t e = e0; e < e1; ++e) {
            const float v = elt_to_f32(x[(int64_t)colidx[e] * D + c]);
            const float p = __expf(fmaf(t, v, -m));
            l += p;
            a = fmaf(p, v - x0, a);
          }
          o = x0 + a / l;
          lse = fmaf(-t, o, m) + logf(l);
        }
        f32_to_elt(o, out + (int64_t)row * D + c);
        if constexpr (SAVE) {
          float* s = stats + (int64_t)row * 2 * D + c;
          s[0] = lse;
          s[D] = o;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward, source-major: 4 columns per lane
// ---------------------------------------------------------------------------

// one transposed edge of one column into dx's accumulator and the lane's dt
template <bool DT>
__device__ __forceinline__ void bwd_term(float& acc, float& dtl, float t,
                                         float xu, float lse, float o,
                                         float dy) {
  const float d = xu - o;
  const float w = __expf(fmaf(t, d, -lse)) * dy;
  acc = fmaf(w, fmaf(t, d, 1.f), acc);
  if constexpr (DT) dtl = fmaf(w * d, d, dtl);
}

// N consecutive transposed edges of source row u: per edge the lane's units
// of lse and out32 (through the gather engine) and of dy, all loads issued
// before the first use
template <int N, typename T, bool DT, typename LD>
__device__ __forceinline__ void bwd_group(
    float* __restrict__ acc, float& dtl, float t,
    const float* __restrict__ xu, const LD& ldl, const LD& ldo, const T* __restrict__ dy, int64_t D,
    int64_t col0, const int* __restrict__ t_colidx, int64_t k) {
  int v[N];
  float4 ls[N], o[N];
  typename Raw4<T>::type g[N];
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = t_colidx[k + i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ls[i] = ldl.load(v[i]);
    o[i] = ldo.load(v[i]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) g[i] = load4(dy + (int64_t)v[i] * D + col0);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float gy[4];
    widen4(gy, g[i]);
    bwd_term<DT>(acc[0], dtl, t, xu[0], ls[i].x, o[i].x, gy[0]);
    bwd_term<DT>(acc[1], dtl, t, xu[1], ls[i].y, o[i].y, gy[1]);
    bwd_term<DT>(acc[2], dtl, t, xu[2], ls[i].z, o[i].z, gy[2]);
    bwd_term<DT>(acc[3], dtl, t, xu[3], ls[i].w, o[i].w, gy[3]);
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool DT>
__global__ __launch_bounds__(kBlock) void seg_softmax_bwd_kernel(
    T* __restrict__ dx, float* __restrict__ slab, const T* __restrict__ dy,
    const T* __restrict__ x, const float* __restrict__ stats,
    const float* __restrict__ tp, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, const int* __restrict__ t_row_order,
    int num_src, int64_t D, unsigned stats_bytes) {
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * kBwdCols;
  const bool full = (col0 + kBwdCols) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, kBwdCols);
  const float t = tp[0];
  float dtl = 0.f;  // the lane's share of dt, over every row it visits

  if (full) {
    const auto ldl = make_gather<float, BUF>(stats, stats_bytes, 2 * D, col0);
    const auto ldo = make_gather<float, BUF>(stats, stats_bytes, 2 * D,
                                             D + col0);
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      int64_t k = t_rowptr[u];
      const int64_t k1 = t_rowptr[u + 1];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      float xu[4];
      widen4(xu, load4(x + (int64_t)u * D + col0));
      ROC_EDGE_LADDER(UN, k, k1,
                      bwd_group<ROC_LADDER_N, T, DT>(acc, dtl, t, xu, ldl,
                                                     ldo, dy, D, col0,
                                                     t_colidx, k));
      store4(dx + (int64_t)u * D + col0, acc);  // the one rounding
    }
  } else if (nvalid > 0) {
    // cold path: one column at a time, scalar loads
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      const int64_t k0 = t_rowptr[u], k1 = t_rowptr[u + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        const float xu = elt_to_f32(x[(int64_t)u * D + c]);
        float acc = 0.f;
        for (int64_t k = k0; k < k1; ++k) {
          const int64_t v = t_colidx[k];
          const float* s = stats + v * 2 * D + c;
          bwd_term<DT>(acc, dtl, t, xu, s[0], s[D],
                       elt_to_f32(dy[v * D + c]));
        }
        f32_to_elt(acc, dx + (int64_t)u * D + c);
      }
    }
  }

  if constexpr (DT) {
    // the block's 256 lane partials in a fixed order: four per lane of the
    // first wave in ascending thread order, then that wave's xor tree
    __shared__ float part[kBlock];
    part[threadIdx.x] = dtl;
    __syncthreads();
    if (threadIdx.x < 64) {
      float s = part[threadIdx.x];
#pragma unroll
      for (int q = 1; q < kBlock / 64; ++q) s += part[threadIdx.x + 64 * q];
      s = team_reduce_sum<64>(s);
      if (threadIdx.x == 0)
        slab[(int64_t)blockIdx.y * gridDim.x + blockIdx.x] = s;
    }
  }
}

// slab [n] -> dt [1]: thread i sums the i-th of kBlock contiguous segments
// in ascending order, thread 0 the segment sums in ascending order. One
// fixed order per n.
__global__ __launch_bounds__(kBlock) void seg_softmax_fold_kernel(
    float* __restrict__ dt, const float* __restrict__ slab, int n) {
  __shared__ float part[kBlock];
  const int per = (n + kBlock - 1) / kBlock;
  const int b0 = (int)threadIdx.x * per;
  const int b1 = b0 + per < n ? b0 + per : n;
  float s = 0.f;
  for (int b = b0; b < b1; ++b) s += slab[b];
  part[threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.x == 0) {
    float tot = 0.f;
    for (int q = 0; q < kBlock; ++q) tot += part[q];
    dt[0] = tot;
  }
}

// rung of the unroll ladder a launch runs at: 0 asks for the default, and
// each direction compiles two
int pick_depth(int64_t depth, int dflt, int shallow, int deep,
               const char* what) {
  if (depth == 0) return dflt;
  TORCH_CHECK(depth == shallow || depth == deep, what,
              ": depth must be 0 (default), ", shallow, " or ", deep);
  return (int)depth;
}

template <int SHALLOW, int DEEP, typename F>
void dispatch_depth(int depth, F&& f) {
  if (depth == DEEP) return f(std::integral_constant<int, DEEP>{});
  f(std::integral_constant<int, SHALLOW>{});
}

void check_stats(const torch::Tensor& stats, int64_t rows, int64_t D,
                 const char* what) {
  ROC_CHECK_DEV_CONT(stats);
  TORCH_CHECK(stats.dim() == 2 && stats.size(0) == rows &&
                  stats.size(1) == 2 * D &&
                  stats.scalar_type() == torch::kFloat32,
              what, ": stats must be fp32 [", rows, ", ", 2 * D, "]");
}

void check_scalar(const torch::Tensor& t, const char* name, const char* what) {
  ROC_CHECK_DEV_CONT(t);
  TORCH_CHECK(t.scalar_type() == torch::kFloat32 && t.numel() == 1, what,
              ": ", name, " must be a fp32 device tensor of one element");
}

}  // namespace

void seg_softmax_fwd(torch::Tensor out, c10::optional<torch::Tensor> stats,
                     torch::Tensor x, torch::Tensor t, torch::Tensor rowptr,
                     torch::Tensor colidx,
                     c10::optional<torch::Tensor> row_order, int64_t depth) {
  const char* what = "seg_softmax_fwd";
  check_mat_pair(out, "out", x, "x", what);
  TORCH_CHECK(out.scalar_type() == x.scalar_type(), what,
              ": out must have x's dtype");
  check_scalar(t, "t", what);
  const int num_rows = (int)out.size(0);
  const int64_t D = x.size(1);
  check_csr_i32(rowptr, colidx, num_rows, what);
  float* statsp = nullptr;
  if (stats.has_value()) {
    check_stats(*stats, num_rows, D, what);
    statsp = stats->data_ptr<float>();
  }
  const int un = pick_depth(depth, kFwdDepth, 8, 16, what);
  if (num_rows == 0 || D == 0) return;
  if (colidx.numel() == 0) {  // every row is empty
    out.zero_();
    if (statsp) stats->zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    constexpr int EPU = EltTraits<T>::kPerVec;
    const GatherGeom g = gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0,
                                        (size_t)x.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(statsp != nullptr, [&](auto save_c) {
        dispatch_depth<8, 16>(un, [&](auto un_c) {
          hipLaunchKernelGGL(
              (seg_softmax_fwd_kernel<T, decltype(team_c)::value,
                                      decltype(un_c)::value,
                                      decltype(buf_c)::value,
                                      decltype(save_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), statsp,
              (const T*)x.data_ptr(), t.data_ptr<float>(),
              rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), order,
              num_rows, D, g.bytes);
        });
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void seg_softmax_bwd(torch::Tensor dx, c10::optional<torch::Tensor> dt_out,
                     torch::Tensor dy, torch::Tensor x, torch::Tensor stats,
                     torch::Tensor t, torch::Tensor t_rowptr,
                     torch::Tensor t_colidx,
                     c10::optional<torch::Tensor> t_row_order, int64_t depth) {
  const char* what = "seg_softmax_bwd";
  check_mat(dx, what, "dx");
  check_mat(dy, what, "dy");
  check_like(x, dx, what, "x");
  check_scalar(t, "t", what);
  const int num_src = (int)dx.size(0);
  const int64_t D = dx.size(1);
  const int64_t num_rows = dy.size(0);
  TORCH_CHECK(dy.size(1) == D && dy.scalar_type() == dx.scalar_type(), what,
              ": dy must be [num_rows, D] in dx's dtype");
  check_stats(stats, num_rows, D, what);
  check_csr_i32(t_rowptr, t_colidx, num_src, what);
  float* dtp = nullptr;
  if (dt_out.has_value()) {
    check_scalar(*dt_out, "dt_out", what);
    dtp = dt_out->data_ptr<float>();
  }
  const int un = pick_depth(depth, kBwdDepth, 4, 8, what);
  if (num_src == 0 || D == 0 || t_colidx.numel() == 0) {
    dx.zero_();
    if (dtp) dt_out->zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(dy.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    GatherGeom g = gather_geom<float>(
        num_src, (D + kBwdCols - 1) / kBwdCols, 0, (size_t)stats.numel());
    torch::Tensor slab;
    float* slabp = nullptr;
    if (dtp) {
      // one slab entry per block: cap the grid so the fold stays short
      const unsigned cap = kSlabMax / g.grid.y > 0 ? kSlabMax / g.grid.y : 1;
      if (g.grid.x > cap) g.grid.x = cap;
      slab = torch::empty({(int64_t)g.grid.x * g.grid.y},
                          stats.options().dtype(torch::kFloat32));
      slabp = slab.data_ptr<float>();
    }
    const int* order = row_order_ptr(t_row_order, num_src, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(dtp != nullptr, [&](auto dt_c) {
        dispatch_depth<4, 8>(un, [&](auto un_c) {
          hipLaunchKernelGGL(
              (seg_softmax_bwd_kernel<T, decltype(team_c)::value,
                                      decltype(un_c)::value,
                                      decltype(buf_c)::value,
                                      decltype(dt_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)dx.data_ptr(), slabp,
              (const T*)dy.data_ptr(), (const T*)x.data_ptr(),
              stats.data_ptr<float>(), t.data_ptr<float>(),
              t_rowptr.data_ptr<int64_t>(), t_colidx.data_ptr<int>(), order,
              num_src, D, g.bytes);
        });
      });
    });
    if (dtp)
      hipLaunchKernelGGL(seg_softmax_fold_kernel, dim3(1), dim3(kBlock), 0,
                         stream, dtp, slabp, (int)(g.grid.x * g.grid.y));
  });
  ROC_HIP_CHECK(hipGetLastError());
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
