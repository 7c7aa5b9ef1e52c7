// CSR segment statistics for CDNA4: the four PNA aggregators (mean, std,
// max, min over the in-neighbourhood; Corso et al. 2020) out of ONE gather
// of each neighbour row.
//
// forward   out[v]   = [ mean | std | max | min ]          [n_rows, 4*D]
//           stats[v] = [ mean | 1/std ]  fp32, unrounded   [n_rows, 2*D]
//           arg[v]   = [ argmax | argmin ] forward edge ids [n_rows, 2*D]
// backward  dx[u] = sum over transposed edges k of u (v = its destination,
//                   f = t_eperm[k]), ascending, of
//                     g_mean[v]/deg_v + g_std[v]*(x[u]-mean[v])*rstd[v]/deg_v
//                     + (argmax[v]==f)*g_max[v] + (argmin[v]==f)*g_min[v]
//
// Same frame as seg_max.hip: a row team owns one row at a time, wide rows
// are column-tiled over blockIdx.y, the gathers go through the shared
// unroll ladder into statically indexed slots. No [E, D] intermediate, no
// atomic; both directions are bit-reproducible.
//
// Rules the tests pin:
//  - sums are SHIFTED by the row's first edge: x0 = x[colidx[e0]],
//    s1 = sum(x-x0), s2 = sum((x-x0)^2) in fp32, ascending in e;
//    mean = x0 + s1/deg, var = max(s2/deg - (s1/deg)^2, 0) (population),
//    std = sqrt(var + eps). Degree-1 and all-equal rows have var == 0.
//  - max / min are seg_max's: seeded from the first edge, strict
//    comparison (first edge wins ties), stored bit for bit
//  - an empty row stores 0 in all four blocks, arg -1, stats 0
//  - the backward reads mean and 1/std from the fp32 stats, never from the
//    rounded out
// NaN and +-inf inputs are out of contract.
//
// The backward is one launch: every transposed edge forms
// g_std*(x[u]-mean[v])*rstd[v] itself. The linear split
// dx[u] = x[u]*sum A[v] + sum B[v], A = g_std*rstd/deg, B = g_mean/deg -
// A*mean, over a row-local coefficient pre-pass gathers the same 24 B per
// edge and bf16 element once its cancellation is repaired, and unrepaired
// it is wrong by |x|*rstd*2^-24 per edge: on a row of equal values near 100
// (rstd = 1/sqrt(eps) = 316) that is 1e-3 where the gradient is 0. Its lane
// unit is 4 columns in both dtypes: a slot holds two fp32 stats units, two
// arg units and four dy units, and at 8 columns that is 48 VGPRs per edge
// in flight.

#include "csr_launch.h"
#include "gather.h"

namespace {

// Gathers in flight per lane, by measurement at the Reddit shape in bf16
// (profiles/r43, one run, medians of 20, D=256 / D=64 in ms; the launchers
// take an override so that scripts/bench_seg_stats.py can repeat it).
// Forward with stats and arg: 16 deep 7.97 / 10.93, 8 deep 8.34 / 11.63,
// 4 deep 8.25 / 11.17. Forward alone (no stats, no arg): 16 deep
// 7.50 / 7.30, 8 deep 7.46 / 8.30, 4 deep 8.97 / 8.82. kFwdBareDepth = 8
// dates from an earlier source, where 16 deep cost a wave per SIMD; on
// these kernels it ties at D=256 and loses at D=64, so 16 is the follow-up.
// Backward: 8 deep 94.94 / 20.76, 4 deep 96.72 / 23.25. 16 deep needs 256
// VGPRs plus AGPR copies, runs at 1 wave per SIMD and took 2.2x as long on
// an earlier source, so it is not compiled.
constexpr int kFwdDepth = 16;
constexpr int kFwdBareDepth = 8;
constexpr int kBwdDepth = 8;
constexpr int kBwdCols = 4;  // columns per lane of the backward launches

// the vector paths need 4-B aligned units: every fp32 width, even bf16 ones
template <typename T>
__device__ __forceinline__ bool vec_ok(int64_t D) {
  return (D * sizeof(T)) % 4 == 0;
}

// columns of the `width`-wide unit at col0 that lie inside D
__device__ __forceinline__ int valid_cols(int64_t col0, int64_t D, int width) {
  return col0 >= D ? 0 : (D - col0 < width ? (int)(D - col0) : width);
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// N consecutive edges into the running sums and extrema, ascending in e
template <int N, typename T, bool SAVE, typename LD>
__device__ __forceinline__ void stats_group(
    const float* __restrict__ x0, float* __restrict__ s1,
    float* __restrict__ s2, float* __restrict__ mx, float* __restrict__ mn,
    int* __restrict__ amx, int* __restrict__ amn, const LD& ld,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  gather_group<N, T>(ld, colidx, e,
                     [&](int i, int, const typename RawVec<T>::type& r) {
    float v[EPU];
    unpack(v, r);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float d = v[j] - x0[j];
      s1[j] += d;
      s2[j] = fmaf(d, d, s2[j]);  // spelled out: see finish_stats
      if (v[j] > mx[j]) {
        mx[j] = v[j];
        if constexpr (SAVE) amx[j] = (int)e + i;
      }
      if (v[j] < mn[j]) {
        mn[j] = v[j];
        if constexpr (SAVE) amn[j] = (int)e + i;
      }
    }
  });
}

// mean, std and 1/std of one column from its shifted sums. The fused
// multiply-adds here and in the sums are spelled out, so that every variant
// of the kernel (depth, stats and arg or not, cold path) rounds alike: left
// to the compiler, the 8-deep and 16-deep fp32 forwards contracted
// differently and disagreed in the last bit.
__device__ __forceinline__ void finish_stats(float x0, float s1, float s2,
                                             float inv_deg, float eps,
                                             float& mean, float& sd,
                                             float& rstd) {
  const float m = s1 * inv_deg;
  const float var = fmaxf(fmaf(s2, inv_deg, -(m * m)), 0.f);
  mean = x0 + m;
  sd = sqrtf(var + eps);
  rstd = 1.f / sd;
}

// hot path of the forward: every row this team owns, one full unit per lane
template <typename T, int UN, bool SAVE, typename TEAM_T, typename LD>
__device__ __forceinline__ void fwd_rows_vec(
    const TEAM_T& rt, const LD& g, T* __restrict__ out,
    float* __restrict__ stats, int* __restrict__ arg,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int64_t D, int64_t col0,
    float eps) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    float mean[EPU], sd[EPU], rstd[EPU], mx[EPU], mn[EPU];
    int amx[EPU], amn[EPU];
    if (e0 < e1) {
      float x0[EPU], s1[EPU], s2[EPU];
      gather_group<1, T>(g, colidx, e0,
                         [&](int, int, const typename RawVec<T>::type& r) {
        unpack(x0, r);
      });
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        s1[j] = 0.f; s2[j] = 0.f;
        mx[j] = x0[j]; mn[j] = x0[j];
        amx[j] = (int)e0; amn[j] = (int)e0;
      }
      int64_t e = e0 + 1;
      ROC_EDGE_LADDER(UN, e, e1,
                      stats_group<ROC_LADDER_N, T, SAVE>(
                          x0, s1, s2, mx, mn, amx, amn, g, colidx, e));
      const float inv_deg = 1.f / (float)(e1 - e0);
#pragma unroll
      for (int j = 0; j < EPU; ++j)
        finish_stats(x0[j], s1[j], s2[j], inv_deg, eps, mean[j], sd[j],
                     rstd[j]);
    } else {
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        mean[j] = sd[j] = rstd[j] = mx[j] = mn[j] = 0.f;
        amx[j] = amn[j] = -1;
      }
    }
    T* o = out + (int64_t)row * 4 * D + col0;
    store_vec(o, mean);
    store_vec(o + D, sd);
    // a widened bf16 has a zero low half, so these two rounds are exact
    store_vec(o + 2 * D, mx);
    store_vec(o + 3 * D, mn);
    if constexpr (SAVE) {
      float* s = stats + (int64_t)row * 2 * D + col0;
      store_vec(s, mean);
      store_vec(s + D, rstd);
      int* a = arg + (int64_t)row * 2 * D + col0;
      store_arg(a, amx);
      store_arg(a + D, amn);
    }
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool SAVE>
__global__ __launch_bounds__(kBlock) void seg_stats_fwd_kernel(
    T* __restrict__ out, float* __restrict__ stats, int* __restrict__ arg,
    const T* __restrict__ x, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const int* __restrict__ row_order,
    int num_rows, int64_t D, unsigned x_bytes, float eps) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, EPU);

  if (full) {
    const auto g = make_gather<T, BUF>(x, x_bytes, D, col0);
    fwd_rows_vec<T, UN, SAVE>(rt, g, out, stats, arg, rowptr, colidx,
                              row_order, num_rows, D, col0, eps);
  } else if (nvalid > 0) {
    // cold path: the unit straddles D, or the rows are not 4-B aligned
    // (odd bf16 widths). One column at a time, scalar loads.
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        float mean = 0.f, sd = 0.f, rstd = 0.f;
        T bmx = T(0), bmn = T(0);
        int amx = -1, amn = -1;
        if (e0 < e1) {
          bmx = bmn = x[(int64_t)colidx[e0] * D + c];
          amx = amn = (int)e0;
          const float x0 = elt_to_f32(bmx);
          float s1 = 0.f, s2 = 0.f, mx = x0, mn = x0;
          for (int64_t e = e0 + 1; e < e1; ++e) {
            const T b = x[(int64_t)colidx[e] * D + c];
            const float v = elt_to_f32(b);
            const float d = v - x0;
            s1 += d;
            s2 = fmaf(d, d, s2);
            if (v > mx) { mx = v; bmx = b; amx = (int)e; }
            if (v < mn) { mn = v; bmn = b; amn = (int)e; }
          }
          finish_stats(x0, s1, s2, 1.f / (float)(e1 - e0), eps, mean, sd,
                       rstd);
        }
        T* o = out + (int64_t)row * 4 * D + c;
        f32_to_elt(mean, o);
        f32_to_elt(sd, o + D);
        o[2 * D] = bmx;
        o[3 * D] = bmn;
        if constexpr (SAVE) {
          float* s = stats + (int64_t)row * 2 * D + c;
          s[0] = mean;
          s[D] = rstd;
          int* a = arg + (int64_t)row * 2 * D + c;
          a[0] = amx;
          a[D] = amn;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: 4 columns per lane
// ---------------------------------------------------------------------------

template <typename T>
struct Raw4 { using type = float4; };
template <>
struct Raw4<unsigned short> { using type = uint2; };

__device__ __forceinline__ float4 load4(const float* p) {
  return *reinterpret_cast<const float4*>(p);
}
__device__ __forceinline__ uint2 load4(const unsigned short* p) {
  return *reinterpret_cast<const uint2*>(p);
}
__device__ __forceinline__ void widen4(float* v, const float4& r) {
  v[0] = r.x; v[1] = r.y; v[2] = r.z; v[3] = r.w;
}
__device__ __forceinline__ void widen4(float* v, const uint2& r) {
  v[0] = bf16_lo(r.x); v[1] = bf16_hi(r.x);
  v[2] = bf16_lo(r.y); v[3] = bf16_hi(r.y);
}
__device__ __forceinline__ void store4(float* p, const float* a) {
  store_f32x4(p, a);
}
__device__ __forceinline__ void store4(unsigned short* p, const float* a) {
  *reinterpret_cast<uint2*>(p) =
      make_uint2(pack_bf16(a[0], a[1]), pack_bf16(a[2], a[3]));
}

// in-degree of destination row v from the low words of its rowptr pair
// (check_csr_i32 keeps every edge offset below 2^31)
__device__ __forceinline__ int2 load_deg(const int64_t* __restrict__ rowptr,
                                         int v) {
  const int* lo = reinterpret_cast<const int*>(rowptr + v);
  return make_int2(lo[0], lo[2]);
}

// N consecutive transposed edges of source row u. Per edge the lane's units
// of mean and 1/std (through the gather engine), of all four blocks of dy
// and of both args, and the destination's degree; all loads issued before
// the first use.
template <int N, typename T, typename LD>
__device__ __forceinline__ void stats_bwd_group(
    float* __restrict__ acc, const float* __restrict__ xu, const LD& ldm,
    const LD& ldr, const T* __restrict__ dy, const int* __restrict__ arg,
    const int64_t* __restrict__ rowptr, int64_t D, int64_t col0,
    const int* __restrict__ t_colidx, const int* __restrict__ t_eperm,
    int64_t k) {
  int v[N], f[N];
  int2 rp[N];
  float4 mean[N], rstd[N];
  int4 ax[N], an[N];
  typename Raw4<T>::type gm[N], gs[N], gx[N], gn[N];
#pragma unroll
  for (int i = 0; i < N; ++i) { v[i] = t_colidx[k + i]; f[i] = t_eperm[k + i]; }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    mean[i] = ldm.load(v[i]);
    rstd[i] = ldr.load(v[i]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rp[i] = load_deg(rowptr, v[i]);
    const int* ap = arg + (int64_t)v[i] * 2 * D + col0;
    ax[i] = *reinterpret_cast<const int4*>(ap);
    an[i] = *reinterpret_cast<const int4*>(ap + D);
    const T* gp = dy + (int64_t)v[i] * 4 * D + col0;
    gm[i] = load4(gp);
    gs[i] = load4(gp + D);
    gx[i] = load4(gp + 2 * D);
    gn[i] = load4(gp + 3 * D);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float m[4], s[4], a[4], b[4];
    widen4(m, gm[i]);
    widen4(s, gs[i]);
    widen4(a, gx[i]);
    widen4(b, gn[i]);
    const float inv_deg = 1.f / (float)(rp[i].y - rp[i].x);
    acc[0] += (m[0] + s[0] * (xu[0] - mean[i].x) * rstd[i].x) * inv_deg;
    acc[1] += (m[1] + s[1] * (xu[1] - mean[i].y) * rstd[i].y) * inv_deg;
    acc[2] += (m[2] + s[2] * (xu[2] - mean[i].z) * rstd[i].z) * inv_deg;
    acc[3] += (m[3] + s[3] * (xu[3] - mean[i].w) * rstd[i].w) * inv_deg;
    acc[0] += ax[i].x == f[i] ? a[0] : 0.f;
    acc[1] += ax[i].y == f[i] ? a[1] : 0.f;
    acc[2] += ax[i].z == f[i] ? a[2] : 0.f;
    acc[3] += ax[i].w == f[i] ? a[3] : 0.f;
    acc[0] += an[i].x == f[i] ? b[0] : 0.f;
    acc[1] += an[i].y == f[i] ? b[1] : 0.f;
    acc[2] += an[i].z == f[i] ? b[2] : 0.f;
    acc[3] += an[i].w == f[i] ? b[3] : 0.f;
  }
}

template <typename T, int TEAM, int UN, bool BUF>
__global__ __launch_bounds__(kBlock) void seg_stats_bwd_kernel(
    T* __restrict__ dx, const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ stats, const int* __restrict__ arg,
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, const int* __restrict__ t_eperm,
    const int* __restrict__ t_row_order, int num_src, int64_t D,
    unsigned stats_bytes) {
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * kBwdCols;
  const bool full = (col0 + kBwdCols) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, kBwdCols);

  if (full) {
    const auto ldm = make_gather<float, BUF>(stats, stats_bytes, 2 * D, col0);
    const auto ldr = make_gather<float, BUF>(stats, stats_bytes, 2 * D,
                                             D + col0);
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      int64_t k = t_rowptr[u];
      const int64_t k1 = t_rowptr[u + 1];
      float acc[4] = {0.f, 0.f, 0.f, 0.f};
      float xu[4];
      widen4(xu, load4(x + (int64_t)u * D + col0));
      ROC_EDGE_LADDER(UN, k, k1,
                      stats_bwd_group<ROC_LADDER_N, T>(
                          acc, xu, ldm, ldr, dy, arg, rowptr, D, col0,
                          t_colidx, t_eperm, k));
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
          const int f = t_eperm[k];
          const T* g = dy + v * 4 * D + c;
          const float* s = stats + v * 2 * D + c;
          const int* a = arg + v * 2 * D + c;
          const float inv_deg = 1.f / (float)(rowptr[v + 1] - rowptr[v]);
          acc += (elt_to_f32(g[0]) +
                  elt_to_f32(g[D]) * (xu - s[0]) * s[D]) * inv_deg;
          if (a[0] == f) acc += elt_to_f32(g[2 * D]);
          if (a[D] == f) acc += elt_to_f32(g[3 * D]);
        }
        f32_to_elt(acc, dx + (int64_t)u * D + c);
      }
    }
  }
}

// rung of the depth ladder a launch runs at: 0 asks for the default
int pick_depth(int64_t depth, int dflt, int deepest, const char* what) {
  if (depth == 0) return dflt;
  TORCH_CHECK((depth == 4 || depth == 8 || depth == 16) && depth <= deepest,
              what, ": depth must be 0 (default), 4, 8 or 16, at most ",
              deepest);
  return (int)depth;
}

template <int DEEPEST, typename F>
void dispatch_depth(int depth, F&& f) {
  if (depth == 4) return f(std::integral_constant<int, 4>{});
  if constexpr (DEEPEST >= 16)
    if (depth == 16) return f(std::integral_constant<int, 16>{});
  f(std::integral_constant<int, 8>{});
}

void check_blocks(const torch::Tensor& t, const char* name, int64_t rows,
                  int64_t cols, torch::ScalarType st, const char* what) {
  ROC_CHECK_DEV_CONT(t);
  TORCH_CHECK(t.dim() == 2 && t.size(0) == rows && t.size(1) == cols &&
                  t.scalar_type() == st,
              what, ": ", name, " must be [", rows, ", ", cols, "] of ", st);
}

}  // namespace

void seg_stats_fwd(torch::Tensor out, c10::optional<torch::Tensor> stats,
                   c10::optional<torch::Tensor> arg, torch::Tensor x,
                   torch::Tensor rowptr, torch::Tensor colidx,
                   c10::optional<torch::Tensor> row_order, double eps,
                   int64_t depth) {
  const char* what = "seg_stats_fwd";
  check_mat(out, what, "out");
  check_mat(x, what, "x");
  const int num_rows = (int)out.size(0);
  const int64_t D = x.size(1);
  TORCH_CHECK(out.size(1) == 4 * D && out.scalar_type() == x.scalar_type(),
              what, ": out must be [num_rows, 4*D] in x's dtype");
  TORCH_CHECK(stats.has_value() == arg.has_value(), what,
              ": stats and arg are given together or not at all");
  TORCH_CHECK(eps > 0, what, ": eps must be positive");
  check_csr_i32(rowptr, colidx, num_rows, what);
  float* statsp = nullptr;
  int* argp = nullptr;
  if (arg.has_value()) {
    check_blocks(*stats, "stats", num_rows, 2 * D, torch::kFloat32, what);
    check_blocks(*arg, "arg", num_rows, 2 * D, torch::kInt32, what);
    statsp = stats->data_ptr<float>();
    argp = arg->data_ptr<int>();
  }
  const int un =
      pick_depth(depth, argp ? kFwdDepth : kFwdBareDepth, 16, what);
  if (num_rows == 0 || D == 0) return;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    constexpr int EPU = EltTraits<T>::kPerVec;
    const GatherGeom g = gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0,
                                        (size_t)x.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(argp != nullptr, [&](auto save_c) {
        dispatch_depth<16>(un, [&](auto un_c) {
          hipLaunchKernelGGL(
              (seg_stats_fwd_kernel<T, decltype(team_c)::value,
                                    decltype(un_c)::value,
                                    decltype(buf_c)::value,
                                    decltype(save_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), statsp,
              argp, (const T*)x.data_ptr(), rowptr.data_ptr<int64_t>(),
              colidx.data_ptr<int>(), order, num_rows, D, g.bytes,
              (float)eps);
        });
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void seg_stats_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor x,
                   torch::Tensor stats, torch::Tensor arg,
                   torch::Tensor rowptr, torch::Tensor t_rowptr,
                   torch::Tensor t_colidx, torch::Tensor t_eperm,
                   c10::optional<torch::Tensor> t_row_order, int64_t depth) {
  const char* what = "seg_stats_bwd";
  check_mat(dx, what, "dx");
  check_mat(dy, what, "dy");
  check_like(x, dx, what, "x");
  ROC_CHECK_DEV_CONT(t_eperm);
  ROC_CHECK_DEV_CONT(rowptr);
  const int num_src = (int)dx.size(0);
  const int64_t D = dx.size(1);
  const int64_t num_rows = dy.size(0);
  TORCH_CHECK(dy.size(1) == 4 * D && dy.scalar_type() == dx.scalar_type(),
              what, ": dy must be [num_rows, 4*D] in dx's dtype");
  check_blocks(stats, "stats", num_rows, 2 * D, torch::kFloat32, what);
  check_blocks(arg, "arg", num_rows, 2 * D, torch::kInt32, what);
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64 && rowptr.dim() == 1 &&
                  rowptr.size(0) == num_rows + 1,
              what, ": rowptr must be int64 [num_rows + 1]");
  check_csr_i32(t_rowptr, t_colidx, num_src, what);
  TORCH_CHECK(t_eperm.scalar_type() == torch::kInt32 &&
                  t_eperm.numel() == t_colidx.numel(),
              what, ": t_eperm must be int32, one entry per edge");
  const int un = pick_depth(depth, kBwdDepth, 8, what);
  if (num_src == 0 || D == 0) return;
  auto stream = roc_stream();
  dispatch_elt(dy.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    const GatherGeom g = gather_geom<float>(
        num_src, (D + kBwdCols - 1) / kBwdCols, 0, (size_t)stats.numel());
    const int* order = row_order_ptr(t_row_order, num_src, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_depth<8>(un, [&](auto un_c) {
        hipLaunchKernelGGL(
            (seg_stats_bwd_kernel<T, decltype(team_c)::value,
                                  decltype(un_c)::value,
                                  decltype(buf_c)::value>),
            g.grid, dim3(kBlock), 0, stream, (T*)dx.data_ptr(),
            (const T*)dy.data_ptr(), (const T*)x.data_ptr(),
            stats.data_ptr<float>(), arg.data_ptr<int>(),
            rowptr.data_ptr<int64_t>(), t_rowptr.data_ptr<int64_t>(),
            t_colidx.data_ptr<int>(), t_eperm.data_ptr<int>(), order, num_src,
            D, g.bytes);
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}
