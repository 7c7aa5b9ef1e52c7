// Edge-gated neighbour aggregation for CDNA4: the aggregator of Bresson &
// Laurent's residual gated graph ConvNet (PyG's ResGatedGraphConv, the
// GatedGCN of "Benchmarking GNNs"). Every edge carries a per-COLUMN sigmoid
// gate that depends on both of its end points.
//
//   eta[e,j]  = sigmoid(q[v,j] + k[u_e,j])          e = (v <- u_e)
//   sum form  : out[v,j] = sum_e eta[e,j] * val[u_e,j]
//   mean form : out[v,j] = sum_e eta[e,j] * val[u_e,j] / (sum_e eta[e,j] + eps)
//
// Operands as in graph_attn.hip: kv [n_ext, 2*D] = [k | val] is the
// halo-extended source projection, q [n_rows, D] the destination one. Nothing
// is split into heads: the columns are independent, so the geometry is
// seg_softmax's. A row team owns one row at a time, a lane one 16-B unit of
// columns, wide rows are column-tiled over blockIdx.y. A ladder slot is TWO
// payloads, the k unit and the val unit of the same gathered row.
//
// The gate is a sigmoid, not a softmax: no running maximum, no rescale, no
// cross-lane reduction. Per edge and column the forward is one add, one exp,
// one add, one reciprocal, one fma and (mean form) one add.
//
// forward   saves, in the mean form, stats [n_rows, 2*D] fp32 =
//           [den | out32]: den = l + eps, out32 the unrounded output.
// backward  with g = dy/den, c = out32 (mean form) or g = dy, c = 0 (sum):
//             dpre[e,j] = g[v,j] * (val[u,j] - c[v,j]) * eta * (1 - eta)
//           dst pass, destination-major:  dq[v]   = sum_e dpre
//           src pass, source-major over the transpose CSR:
//             dk[u] = sum_k dpre,  dval[u] = sum_k eta * g[w_k]
//           Both recompute eta. No atomics, no edge permutation, no [E, D]
//           tensor.
//
// Rules the tests pin:
//  - all arithmetic is fp32 over the exact widen, in ascending
//    (transposed-)edge order inside one lane; out, dq and dkv are rounded
//    once, at the store. A row's result depends on its own edges only: not on
//    the grid, the gather engine or row_order.
//  - the gate is rcp(1 + __expf(-z)) (gate() below). __expf(-z) lies in
//    [0, +inf]: it overflows to +inf for z below about -88, 1 + inf = inf and
//    rcp(inf) = 0, so eta = 0 exactly; it underflows to 0 for large z and
//    eta = 1. eta and 1 - eta lie in [0, 1], g is finite because den >= eps
//    > 0, val - c is a difference of finite values: no inf - inf, no
//    0 * inf, no NaN at any z.
//  - stats = None is the same arithmetic without the state stores; the
//    backward reads den and out32 from the fp32 stats, never the rounded out
//  - an empty row stores out = 0, stats = 0 and dq = 0; a source without
//    out-edges gets dkv = 0; duplicate edges each count
// NaN and +-inf inputs are out of contract.

#include "csr_launch.h"
#include "gather.h"

// As in seg_softmax.hip: scalar-lane fp32 only and no contraction behind the
// source's back, so that the variants of a kernel (depth, stats or not)
// round alike. Every fma is spelled out.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif
#pragma clang fp contract(off)

namespace {

// Edges in flight per lane; the launchers take an override so that
// scripts/bench_gated.py can repeat the comparison. docs/KERNELS.md has the
// resource table, profiles/r51 the measurements.
// Forward and dst pass: a slot is two 16-B payloads, 8 VGPRs; 8 deep, the
// depth graph_attn.hip uses for K + V, is 103-126 VGPRs in bf16 (4 waves per
// SIMD), 16 deep 167-245 (2-3 waves). Measured at the Reddit shape in bf16
// (medians of 9, D=256 / D=64 in ms): forward with stats 15.45 / 11.14 at 8
// deep against 15.16 / 12.70 at 16, dst pass 15.53 / 13.00 against 15.11 /
// 15.31: 16 deep gains 2-3 % where the bytes set the time and loses 14-18 %
// at D=64.
// Src pass: a slot is a q and a dy unit of 4 columns and, in the mean form,
// two fp32 stats units: 4 / 8 VGPRs (sum form, bf16 / fp32), 12 / 16 (mean).
// Mean form 45.32 / 10.38 at 8 deep against 45.91 / 10.49 at 4 deep, sum form
// 14.83 / 3.23 against 15.02 / 3.23, although the report gives 4 deep 5
// waves and 8 deep 3.
constexpr int kFwdDepth = 8;
constexpr int kDstDepth = 8;
constexpr int kSrcDepth = 8;
constexpr int kSrcCols = 4;  // columns per lane of the src pass

// the vector paths need 4-B aligned units: every fp32 width, even bf16 ones
template <typename T>
__device__ __forceinline__ bool vec_ok(int64_t D) {
  return (D * sizeof(T)) % 4 == 0;
}

// columns of the `width`-wide unit at col0 that lie inside D
__device__ __forceinline__ int valid_cols(int64_t col0, int64_t D, int width) {
  return col0 >= D ? 0 : (D - col0 < width ? (int)(D - col0) : width);
}

// sigmoid(q + k), finite at any z (see the rules above). The reciprocal is
// the hardware's (v_rcp_f32, 1 ulp): its operand lies in [1, +inf].
__device__ __forceinline__ float gate(float q, float k) {
  return __builtin_amdgcn_rcpf(1.f + __expf(-(q + k)));
}

// EPU consecutive fp32 of the saved state
template <int EPU>
__device__ __forceinline__ void load_state(float (&v)[EPU], const float* p) {
#pragma unroll
  for (int j = 0; j < EPU; j += 4) load_f32x4(p + j, v + j);
}

template <int EPU>
__device__ __forceinline__ void zero(float (&v)[EPU]) {
#pragma unroll
  for (int j = 0; j < EPU; ++j) v[j] = 0.f;
}

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

// N consecutive edges: the indices, then the 2N payloads, then the fold in
// edge order
template <int N, typename T, bool NORM, typename LD>
__device__ __forceinline__ void fwd_group(
    float (&a)[EltTraits<T>::kPerVec], float (&l)[EltTraits<T>::kPerVec],
    const float (&qf)[EltTraits<T>::kPerVec], const LD& ldk, const LD& ldv,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type rk[N], rv[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rk[i] = ldk.load(u[i]);
    rv[i] = ldv.load(u[i]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float kf[EPU], vf[EPU];
    unpack(kf, rk[i]);
    unpack(vf, rv[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float eta = gate(qf[j], kf[j]);
      a[j] = fmaf(eta, vf[j], a[j]);
      if constexpr (NORM) l[j] += eta;
    }
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool NORM, bool SAVE>
__global__ __launch_bounds__(kBlock) void gated_agg_fwd_kernel(
    T* __restrict__ out, float* __restrict__ stats, const T* __restrict__ q,
    const T* __restrict__ kv, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const int* __restrict__ row_order,
    int num_rows, int64_t D, float eps, unsigned kv_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, EPU);

  if (full) {
    const auto ldk = make_gather<T, BUF>(kv, kv_bytes, 2 * D, col0);
    const auto ldv = make_gather<T, BUF>(kv, kv_bytes, 2 * D, D + col0);
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      int64_t e = rowptr[row];
      const int64_t e1 = rowptr[row + 1];
      const bool empty = e == e1;
      float qf[EPU], a[EPU], l[EPU];
      unpack(qf, load_raw(q + (int64_t)row * D + col0));
      zero(a);
      zero(l);
      ROC_EDGE_LADDER(UN, e, e1,
                      (fwd_group<ROC_LADDER_N, T, NORM>(a, l, qf, ldk, ldv,
                                                        colidx, e)));
      if constexpr (NORM) {
        // an empty row keeps a = 0: out = 0, and its stats are stored as 0
#pragma unroll
        for (int j = 0; j < EPU; ++j) {
          l[j] = empty ? 0.f : l[j] + eps;
          a[j] = empty ? 0.f : a[j] / l[j];
        }
      }
      store_vec(out + (int64_t)row * D + col0, a);  // the one rounding
      if constexpr (SAVE) {
        float* s = stats + (int64_t)row * 2 * D + col0;
        store_vec(s, l);
        store_vec(s + D, a);
      }
    }
  } else if (nvalid > 0) {
    // cold path: the unit straddles D, or the rows are not 4-B aligned (odd
    // bf16 widths). One column at a time, scalar loads.
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        const float qf = elt_to_f32(q[(int64_t)row * D + c]);
        float a = 0.f, l = 0.f;
        for (int64_t e = e0; e < e1; ++e) {
          const T* src = kv + (int64_t)colidx[e] * 2 * D + c;
          const float eta = gate(qf, elt_to_f32(src[0]));
          a = fmaf(eta, elt_to_f32(src[D]), a);
          if constexpr (NORM) l += eta;
        }
        if constexpr (NORM) {
          l = e0 == e1 ? 0.f : l + eps;
          a = e0 == e1 ? 0.f : a / l;
        }
        f32_to_elt(a, out + (int64_t)row * D + c);
        if constexpr (SAVE) {
          float* s = stats + (int64_t)row * 2 * D + c;
          s[0] = l;
          s[D] = a;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward, destination-major: dq
// ---------------------------------------------------------------------------

// one edge of one column into an accumulator of dpre
template <bool NORM>
__device__ __forceinline__ void dpre_term(float& acc, float eta, float g,
                                          float val, float c) {
  const float t = NORM ? g * (val - c) : g * val;
  acc = fmaf(t, eta * (1.f - eta), acc);
}

template <int N, typename T, bool NORM, typename LD>
__device__ __forceinline__ void dst_group(
    float (&acc)[EltTraits<T>::kPerVec],
    const float (&qf)[EltTraits<T>::kPerVec],
    const float (&g)[EltTraits<T>::kPerVec],
    const float (&c)[EltTraits<T>::kPerVec], const LD& ldk, const LD& ldv,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type rk[N], rv[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rk[i] = ldk.load(u[i]);
    rv[i] = ldv.load(u[i]);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float kf[EPU], vf[EPU];
    unpack(kf, rk[i]);
    unpack(vf, rv[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j)
      dpre_term<NORM>(acc[j], gate(qf[j], kf[j]), g[j], vf[j], c[j]);
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool NORM>
__global__ __launch_bounds__(kBlock) void gated_agg_bwd_dst_kernel(
    T* __restrict__ dq, const T* __restrict__ dy,
    const float* __restrict__ stats, const T* __restrict__ q,
    const T* __restrict__ kv, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const int* __restrict__ row_order,
    int num_rows, int64_t D, unsigned kv_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, EPU);

  if (full) {
    const auto ldk = make_gather<T, BUF>(kv, kv_bytes, 2 * D, col0);
    const auto ldv = make_gather<T, BUF>(kv, kv_bytes, 2 * D, D + col0);
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      int64_t e = rowptr[row];
      const int64_t e1 = rowptr[row + 1];
      float acc[EPU], qf[EPU], g[EPU], c[EPU];
      zero(acc);
      zero(c);
      if (e < e1) {  // an empty row has den = 0 and nothing to add
        unpack(qf, load_raw(q + (int64_t)row * D + col0));
        unpack(g, load_raw(dy + (int64_t)row * D + col0));
        if constexpr (NORM) {
          float den[EPU];
          const float* s = stats + (int64_t)row * 2 * D + col0;
          load_state(den, s);
          load_state(c, s + D);
#pragma unroll
          for (int j = 0; j < EPU; ++j) g[j] = g[j] / den[j];
        }
        ROC_EDGE_LADDER(UN, e, e1,
                        (dst_group<ROC_LADDER_N, T, NORM>(acc, qf, g, c, ldk,
                                                          ldv, colidx, e)));
      }
      store_vec(dq + (int64_t)row * D + col0, acc);  // the one rounding
    }
  } else if (nvalid > 0) {
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t cj = col0 + j;
        float acc = 0.f;
        if (e0 < e1) {
          const float qf = elt_to_f32(q[(int64_t)row * D + cj]);
          float g = elt_to_f32(dy[(int64_t)row * D + cj]), c = 0.f;
          if constexpr (NORM) {
            const float* s = stats + (int64_t)row * 2 * D + cj;
            g = g / s[0];
            c = s[D];
          }
          for (int64_t e = e0; e < e1; ++e) {
            const T* src = kv + (int64_t)colidx[e] * 2 * D + cj;
            dpre_term<NORM>(acc, gate(qf, elt_to_f32(src[0])), g,
                            elt_to_f32(src[D]), c);
          }
        }
        f32_to_elt(acc, dq + (int64_t)row * D + cj);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward, source-major over the transpose CSR: dkv, 4 columns per lane
// ---------------------------------------------------------------------------

// one transposed edge of one column: den and c are the destination's state
template <bool NORM>
__device__ __forceinline__ void src_term(float& dk, float& dv, float ku,
                                         float vu, float qw, float gy,
                                         float den, float c) {
  const float eta = gate(qw, ku);
  // den >= eps > 0; its reciprocal is the hardware's, as the gate's
  const float g = NORM ? gy * __builtin_amdgcn_rcpf(den) : gy;
  dv = fmaf(eta, g, dv);
  dpre_term<NORM>(dk, eta, g, vu, c);
}

// N consecutive transposed edges of source row u: per edge the destination's
// q and dy units and, in the mean form, its two stats units (through the
// gather engine), all loads issued before the first use
template <int N, typename T, bool NORM, typename LD>
__device__ __forceinline__ void src_group(
    float* __restrict__ dk, float* __restrict__ dv,
    const float* __restrict__ ku, const float* __restrict__ vu, const LD& ldd,
    const LD& ldo, const T* __restrict__ q, const T* __restrict__ dy,
    int64_t D, int64_t col0, const int* __restrict__ t_colidx, int64_t k) {
  int w[N];
  float4 den[N], o[N];
  typename Raw4<T>::type rq[N], rg[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = t_colidx[k + i];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    if constexpr (NORM) {
      den[i] = ldd.load(w[i]);
      o[i] = ldo.load(w[i]);
    } else {
      den[i] = o[i] = make_float4(0.f, 0.f, 0.f, 0.f);
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    rq[i] = load4(q + (int64_t)w[i] * D + col0);
    rg[i] = load4(dy + (int64_t)w[i] * D + col0);
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float qw[4], gy[4];
    widen4(qw, rq[i]);
    widen4(gy, rg[i]);
    src_term<NORM>(dk[0], dv[0], ku[0], vu[0], qw[0], gy[0], den[i].x, o[i].x);
    src_term<NORM>(dk[1], dv[1], ku[1], vu[1], qw[1], gy[1], den[i].y, o[i].y);
    src_term<NORM>(dk[2], dv[2], ku[2], vu[2], qw[2], gy[2], den[i].z, o[i].z);
    src_term<NORM>(dk[3], dv[3], ku[3], vu[3], qw[3], gy[3], den[i].w, o[i].w);
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool NORM>
__global__ __launch_bounds__(kBlock) void gated_agg_bwd_src_kernel(
    T* __restrict__ dkv, const T* __restrict__ dy,
    const float* __restrict__ stats, const T* __restrict__ q,
    const T* __restrict__ kv, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, const int* __restrict__ t_row_order,
    int num_src, int64_t D, unsigned stats_bytes) {
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * kSrcCols;
  const bool full = (col0 + kSrcCols) <= D && vec_ok<T>(D);
  const int nvalid = valid_cols(col0, D, kSrcCols);

  if (full) {
    // the sum form has no stats: its engines are never used
    const auto ldd = make_gather<float, BUF>(stats, stats_bytes, 2 * D, col0);
    const auto ldo = make_gather<float, BUF>(stats, stats_bytes, 2 * D,
                                             D + col0);
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      int64_t k = t_rowptr[u];
      const int64_t k1 = t_rowptr[u + 1];
      float dk[4] = {0.f, 0.f, 0.f, 0.f}, dv[4] = {0.f, 0.f, 0.f, 0.f};
      float ku[4], vu[4];
      const T* own = kv + (int64_t)u * 2 * D + col0;
      widen4(ku, load4(own));
      widen4(vu, load4(own + D));
      ROC_EDGE_LADDER(UN, k, k1,
                      (src_group<ROC_LADDER_N, T, NORM>(dk, dv, ku, vu, ldd,
                                                        ldo, q, dy, D, col0,
                                                        t_colidx, k)));
      T* d = dkv + (int64_t)u * 2 * D + col0;
      store4(d, dk);  // the one rounding
      store4(d + D, dv);
    }
  } else if (nvalid > 0) {
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      const int64_t k0 = t_rowptr[u], k1 = t_rowptr[u + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        const T* own = kv + (int64_t)u * 2 * D + c;
        const float ku = elt_to_f32(own[0]), vu = elt_to_f32(own[D]);
        float dk = 0.f, dv = 0.f;
        for (int64_t k = k0; k < k1; ++k) {
          const int64_t w = t_colidx[k];
          float den = 0.f, o = 0.f;
          if constexpr (NORM) {
            const float* s = stats + w * 2 * D + c;
            den = s[0];
            o = s[D];
          }
          src_term<NORM>(dk, dv, ku, vu, elt_to_f32(q[w * D + c]),
                         elt_to_f32(dy[w * D + c]), den, o);
        }
        T* d = dkv + (int64_t)u * 2 * D + c;
        f32_to_elt(dk, d);
        f32_to_elt(dv, d + D);
      }
    }
  }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------

// rung of the unroll ladder a launch runs at: 0 asks for the default, and
// each kernel compiles two
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

// The operands every launcher takes. `rows` names the [n_rows, D] matrix the
// launch writes or reads next to q (out / dy), kv's row count is the number
// of sources. Returns the stats pointer, null in the sum form.
const float* check_operands(const torch::Tensor& rows, const char* rows_name,
                            const c10::optional<torch::Tensor>& stats,
                            const torch::Tensor& q, const torch::Tensor& kv,
                            bool normalize, bool need_stats,
                            const char* what) {
  check_mat_pair(rows, rows_name, q, "q", what);
  check_like(rows, q, what, rows_name);
  check_mat(kv, what, "kv");
  const int64_t D = q.size(1);
  TORCH_CHECK(kv.size(1) == 2 * D && kv.scalar_type() == q.scalar_type(), what,
              ": kv must be [n_src, ", 2 * D, "] = [k | val] in q's dtype");
  TORCH_CHECK(!stats.has_value() || normalize, what,
              ": the sum form saves no stats");
  TORCH_CHECK(stats.has_value() || !need_stats, what,
              ": the mean form needs the forward's stats");
  if (!stats.has_value()) return nullptr;
  ROC_CHECK_DEV_CONT(*stats);
  TORCH_CHECK(stats->dim() == 2 && stats->size(0) == q.size(0) &&
                  stats->size(1) == 2 * D &&
                  stats->scalar_type() == torch::kFloat32,
              what, ": stats must be fp32 [", q.size(0), ", ", 2 * D, "]");
  return stats->data_ptr<float>();
}

}  // namespace

void gated_agg_fwd(torch::Tensor out, c10::optional<torch::Tensor> stats,
                   torch::Tensor q, torch::Tensor kv, torch::Tensor rowptr,
                   torch::Tensor colidx,
                   c10::optional<torch::Tensor> row_order, bool normalize,
                   double eps, int64_t depth) {
  const char* what = "gated_agg_fwd";
  float* statsp = const_cast<float*>(
      check_operands(out, "out", stats, q, kv, normalize, false, what));
  TORCH_CHECK(!normalize || eps > 0.0, what,
              ": the mean form needs eps > 0 (the denominator of a row whose "
              "gates all underflow)");
  const int num_rows = (int)out.size(0);
  const int64_t D = q.size(1);
  check_csr_i32(rowptr, colidx, num_rows, what);
  const int un = pick_depth(depth, kFwdDepth, 8, 16, what);
  if (num_rows == 0 || D == 0) return;
  if (colidx.numel() == 0) {  // every row is empty
    out.zero_();
    if (statsp) stats->zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    constexpr int EPU = EltTraits<T>::kPerVec;
    const GatherGeom g = gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0,
                                        (size_t)kv.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, what);
    auto launch = [&](auto team_c, auto buf_c, auto norm_c, auto save_c) {
      dispatch_depth<8, 16>(un, [&](auto un_c) {
        hipLaunchKernelGGL(
            (gated_agg_fwd_kernel<T, decltype(team_c)::value,
                                  decltype(un_c)::value,
                                  decltype(buf_c)::value,
                                  decltype(norm_c)::value,
                                  decltype(save_c)::value>),
            g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), statsp,
            (const T*)q.data_ptr(), (const T*)kv.data_ptr(),
            rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), order,
            num_rows, D, (float)eps, g.bytes);
      });
    };
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      // the sum form saves nothing: three variants, not four
      if (!normalize)
        launch(team_c, buf_c, std::false_type{}, std::false_type{});
      else if (statsp)
        launch(team_c, buf_c, std::true_type{}, std::true_type{});
      else
        launch(team_c, buf_c, std::true_type{}, std::false_type{});
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void gated_agg_bwd_dst(torch::Tensor dq, torch::Tensor dy,
                       c10::optional<torch::Tensor> stats, torch::Tensor q,
                       torch::Tensor kv, torch::Tensor rowptr,
                       torch::Tensor colidx,
                       c10::optional<torch::Tensor> row_order, bool normalize,
                       int64_t depth) {
  const char* what = "gated_agg_bwd_dst";
  const float* statsp =
      check_operands(dy, "dy", stats, q, kv, normalize, normalize, what);
  check_like(dq, q, what, "dq");
  const int num_rows = (int)q.size(0);
  const int64_t D = q.size(1);
  check_csr_i32(rowptr, colidx, num_rows, what);
  const int un = pick_depth(depth, kDstDepth, 8, 16, what);
  if (num_rows == 0 || D == 0) return;
  if (colidx.numel() == 0) {
    dq.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    constexpr int EPU = EltTraits<T>::kPerVec;
    const GatherGeom g = gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0,
                                        (size_t)kv.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(normalize, [&](auto norm_c) {
        dispatch_depth<8, 16>(un, [&](auto un_c) {
          hipLaunchKernelGGL(
              (gated_agg_bwd_dst_kernel<T, decltype(team_c)::value,
                                        decltype(un_c)::value,
                                        decltype(buf_c)::value,
                                        decltype(norm_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)dq.data_ptr(),
              (const T*)dy.data_ptr(), statsp, (const T*)q.data_ptr(),
              (const T*)kv.data_ptr(), rowptr.data_ptr<int64_t>(),
              colidx.data_ptr<int>(), order, num_rows, D, g.bytes);
        });
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void gated_agg_bwd_src(torch::Tensor dkv, torch::Tensor dy,
                       c10::optional<torch::Tensor> stats, torch::Tensor q,
                       torch::Tensor kv, torch::Tensor t_rowptr,
                       torch::Tensor t_colidx,
                       c10::optional<torch::Tensor> t_row_order,
                       bool normalize, int64_t depth) {
  const char* what = "gated_agg_bwd_src";
  const float* statsp =
      check_operands(dy, "dy", stats, q, kv, normalize, normalize, what);
  check_like(dkv, kv, what, "dkv");
  const int num_src = (int)kv.size(0);
  const int64_t D = q.size(1);
  check_csr_i32(t_rowptr, t_colidx, num_src, what);
  const int un = pick_depth(depth, kSrcDepth, 4, 8, what);
  if (num_src == 0 || D == 0) return;
  if (t_colidx.numel() == 0 || q.size(0) == 0) {
    dkv.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), what, [&](auto xt) {
    using T = typename decltype(xt)::type;
    // the engine serves the stats gathers only: the sum form has none
    const GatherGeom g = gather_geom<float>(
        num_src, (D + kSrcCols - 1) / kSrcCols, 0,
        normalize ? (size_t)stats->numel() : 0, normalize);
    const int* order = row_order_ptr(t_row_order, num_src, g.team, what);
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(normalize, [&](auto norm_c) {
        dispatch_depth<4, 8>(un, [&](auto un_c) {
          hipLaunchKernelGGL(
              (gated_agg_bwd_src_kernel<T, decltype(team_c)::value,
                                        decltype(un_c)::value,
                                        decltype(buf_c)::value,
                                        decltype(norm_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)dkv.data_ptr(),
              (const T*)dy.data_ptr(), statsp, (const T*)q.data_ptr(),
              (const T*)kv.data_ptr(), t_rowptr.data_ptr<int64_t>(),
              t_colidx.data_ptr<int>(), order, num_src, D, g.bytes);
        });
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif
