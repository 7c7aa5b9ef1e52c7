// CSR segment max / min neighbor aggregation for CDNA4 (AGGR_MAX / AGGR_MIN
// of the reference operator layer, `gnn.h:75-79`, which it declares and
// never implements).
//
// forward   out[v, j] = ext_{e in row v} x[colidx[e], j]
//           arg[v, j] = the forward CSR edge index e of the winner
// backward  dx[u, j]  = sum over transposed edges k of u, ascending, of
//                       dy[v_k, j] where arg[v_k, j] == t_eperm[k]
//
// Same frame as spmm_kernel: a row team owns one row at a time, a lane owns
// one 16-B unit of the row, wide rows are column-tiled over blockIdx.y, and
// the gathers go through the shared unroll ladder (gather.h) into statically
// indexed slots. The running best (and its edge index) lives in registers;
// there is no [E, D] intermediate and no atomic.
//
// Rules the tests pin:
//  - the running best is seeded from the row's FIRST edge, never from 0 or
//    -FLT_MAX, so all-negative rows and rows holding -inf come out right
//  - a later edge replaces the best only on a strict comparison, so among
//    equal values the first edge in CSR order wins
//  - an empty row stores 0 and arg -1
//  - values are compared as fp32 after the exact bf16 widen and the stored
//    result is one of the inputs bit for bit (nothing is rounded)
//  - arg names an EDGE, not a source row: with duplicate (u, v) edges a
//    source id would make the backward count the winner once per duplicate
// NaN inputs are out of contract.

#include "csr_launch.h"
#include "gather.h"

namespace {

// Gathers in flight per lane. Forward: 16 and 8 measure the same, 4 is 23%
// slower. Backward: a slot also carries EPU arg words, so 16 deep costs 189
// VGPRs / 2 waves per SIMD in bf16 and still beats 8 deep (112 / 4 waves)
// by 9% at the Reddit shape, without scratch (profiles/r39).
constexpr int kFwdDepth = 16;
constexpr int kBwdDepth = 16;

template <bool MIN>
__device__ __forceinline__ bool beats(float v, float best) {
  return MIN ? v < best : v > best;
}

// N consecutive edges against the running best, ascending in e
template <int N, typename T, bool MIN, bool ARG, typename LD>
__device__ __forceinline__ void ext_group(
    float* __restrict__ best, int* __restrict__ barg, const LD& ld,
    const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  gather_group<N, T>(ld, colidx, e,
                     [&](int i, int, const typename RawVec<T>::type& r) {
    float v[EPU];
    unpack(v, r);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      if (beats<MIN>(v[j], best[j])) {
        best[j] = v[j];
        if constexpr (ARG) barg[j] = (int)e + i;
      }
    }
  });
}

template <typename T, int UN, bool MIN, bool ARG, typename LD>
__device__ __forceinline__ void row_ext_vec(
    float* __restrict__ best, int* __restrict__ barg, const LD& ld,
    const int* __restrict__ colidx, int64_t e, int64_t e1) {
  ROC_EDGE_LADDER(
      UN, e, e1,
      ext_group<ROC_LADDER_N, T, MIN, ARG>(best, barg, ld, colidx, e));
}

// hot path of the forward: every row this team owns, one full unit per lane
template <typename T, int UN, bool MIN, bool ARG, typename TEAM_T, typename LD>
__device__ __forceinline__ void fwd_rows_vec(
    const TEAM_T& rt, const LD& g, T* __restrict__ out, int* __restrict__ arg,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int64_t D, int64_t col0) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    float best[EPU];
    int barg[EPU];
    if (e0 < e1) {
      gather_group<1, T>(g, colidx, e0,
                         [&](int, int, const typename RawVec<T>::type& r) {
        unpack(best, r);
      });
#pragma unroll
      for (int j = 0; j < EPU; ++j) barg[j] = (int)e0;
      row_ext_vec<T, UN, MIN, ARG>(best, barg, g, colidx, e0 + 1, e1);
    } else {
#pragma unroll
      for (int j = 0; j < EPU; ++j) { best[j] = 0.f; barg[j] = -1; }
    }
    // a widened bf16 has a zero low half, so the round in store_vec is exact
    store_vec(out + (int64_t)row * D + col0, best);
    if constexpr (ARG) store_arg(arg + (int64_t)row * D + col0, barg);
  }
}

template <typename T, int TEAM, int UN, bool BUF, bool MIN, bool ARG>
__global__ __launch_bounds__(kBlock) void seg_max_fwd_kernel(
    T* __restrict__ out, int* __restrict__ arg, const T* __restrict__ x,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int64_t D,
    unsigned x_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D;
  const int nvalid = full ? EPU : (col0 < D ? (int)(D - col0) : 0);

  if (full) {
    const auto g = make_gather<T, BUF>(x, x_bytes, D, col0);
    fwd_rows_vec<T, UN, MIN, ARG>(rt, g, out, arg, rowptr, colidx, row_order,
                                  num_rows, D, col0);
  } else if (nvalid > 0) {
    // cold path: the unit straddles D (D % EPU != 0). One column at a time,
    // scalar loads, the running best in two scalars.
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        T bits = T(0);
        int ba = -1;
        if (e0 < e1) {
          bits = x[(int64_t)colidx[e0] * D + c];
          ba = (int)e0;
          float best = elt_to_f32(bits);
          for (int64_t e = e0 + 1; e < e1; ++e) {
            const T b = x[(int64_t)colidx[e] * D + c];
            const float v = elt_to_f32(b);
            if (beats<MIN>(v, best)) { best = v; bits = b; ba = (int)e; }
          }
        }
        out[(int64_t)row * D + c] = bits;
        if constexpr (ARG) arg[(int64_t)row * D + c] = ba;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// backward: gather over the transpose CSR
// ---------------------------------------------------------------------------

// N consecutive transposed edges of source row u: the lane's unit of dy[v]
// and of arg[v] per edge, all loads issued before the first use
template <int N, typename T, typename LD>
__device__ __forceinline__ void route_group(
    float* __restrict__ acc, const LD& ld, const int* __restrict__ arg,
    int64_t D, int64_t col0, const int* __restrict__ t_colidx,
    const int* __restrict__ t_eperm, int64_t k) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int v[N], f[N];
  typename RawVec<T>::type r[N];
  int4 a[N][EPU / 4];
#pragma unroll
  for (int i = 0; i < N; ++i) { v[i] = t_colidx[k + i]; f[i] = t_eperm[k + i]; }
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = ld.load(v[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const int4* ap =
        reinterpret_cast<const int4*>(arg + (int64_t)v[i] * D + col0);
#pragma unroll
    for (int q = 0; q < EPU / 4; ++q) a[i][q] = ap[q];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float d[EPU];
    unpack(d, r[i]);
#pragma unroll
    for (int q = 0; q < EPU / 4; ++q) {
      acc[4 * q + 0] += a[i][q].x == f[i] ? d[4 * q + 0] : 0.f;
      acc[4 * q + 1] += a[i][q].y == f[i] ? d[4 * q + 1] : 0.f;
      acc[4 * q + 2] += a[i][q].z == f[i] ? d[4 * q + 2] : 0.f;
      acc[4 * q + 3] += a[i][q].w == f[i] ? d[4 * q + 3] : 0.f;
    }
  }
}

template <typename T, int UN, typename TEAM_T, typename LD>
__device__ __forceinline__ void bwd_rows_vec(
    const TEAM_T& rt, const LD& g, T* __restrict__ dx,
    const int* __restrict__ arg, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, const int* __restrict__ t_eperm,
    const int* __restrict__ t_row_order, int num_src, int64_t D,
    int64_t col0) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
    const int u = t_row_order ? t_row_order[ri] : ri;
    int64_t k = t_rowptr[u];
    const int64_t k1 = t_rowptr[u + 1];
    float acc[EPU];
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    ROC_EDGE_LADDER(UN, k, k1,
                    route_group<ROC_LADDER_N, T>(acc, g, arg, D, col0, t_colidx,
                                                 t_eperm, k));
    store_vec(dx + (int64_t)u * D + col0, acc);  // the one rounding
  }
}

template <typename T, int TEAM, int UN, bool BUF>
__global__ __launch_bounds__(kBlock) void seg_max_bwd_kernel(
    T* __restrict__ dx, const T* __restrict__ dy, const int* __restrict__ arg,
    const int64_t* __restrict__ t_rowptr, const int* __restrict__ t_colidx,
    const int* __restrict__ t_eperm, const int* __restrict__ t_row_order,
    int num_src, int64_t D, unsigned dy_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= D;
  const int nvalid = full ? EPU : (col0 < D ? (int)(D - col0) : 0);

  if (full) {
    const auto g = make_gather<T, BUF>(dy, dy_bytes, D, col0);
    bwd_rows_vec<T, UN>(rt, g, dx, arg, t_rowptr, t_colidx, t_eperm,
                        t_row_order, num_src, D, col0);
  } else if (nvalid > 0) {
    // cold path: one column at a time, scalar loads
    for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
      const int u = t_row_order ? t_row_order[ri] : ri;
      const int64_t k0 = t_rowptr[u], k1 = t_rowptr[u + 1];
      for (int j = 0; j < nvalid; ++j) {
        const int64_t c = col0 + j;
        float acc = 0.f;
        for (int64_t k = k0; k < k1; ++k) {
          const int64_t at = (int64_t)t_colidx[k] * D + c;
          if (arg[at] == t_eperm[k]) acc += elt_to_f32(dy[at]);
        }
        f32_to_elt(acc, dx + (int64_t)u * D + c);
      }
    }
  }
}

template <typename T>
GatherGeom seg_geom(int num_rows, int64_t D, size_t gathered_elems) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  return gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0, gathered_elems);
}

}  // namespace

void seg_max_fwd(torch::Tensor out, c10::optional<torch::Tensor> arg,
                 torch::Tensor x, torch::Tensor rowptr, torch::Tensor colidx,
                 c10::optional<torch::Tensor> row_order, bool is_min) {
  check_mat_pair(out, "out", x, "x", "seg_max_fwd");
  TORCH_CHECK(out.scalar_type() == x.scalar_type(),
              "seg_max_fwd: out and x must share a dtype");
  const int num_rows = (int)out.size(0);
  const int64_t D = out.size(1);
  check_csr_i32(rowptr, colidx, num_rows, "seg_max_fwd");
  int* argp = nullptr;
  if (arg.has_value()) {
    ROC_CHECK_DEV_CONT(*arg);
    TORCH_CHECK(arg->scalar_type() == torch::kInt32 &&
                    arg->sizes() == out.sizes(),
                "seg_max_fwd: arg must be int32 with the shape of out");
    argp = arg->data_ptr<int>();
  }
  if (num_rows == 0 || D == 0) return;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "seg_max_fwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const GatherGeom g = seg_geom<T>(num_rows, D, (size_t)x.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, "seg_max_fwd");
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(is_min, [&](auto min_c) {
        dispatch_bool(argp != nullptr, [&](auto arg_c) {
          hipLaunchKernelGGL(
              (seg_max_fwd_kernel<T, decltype(team_c)::value, kFwdDepth,
                                  decltype(buf_c)::value,
                                  decltype(min_c)::value,
                                  decltype(arg_c)::value>),
              g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), argp,
              (const T*)x.data_ptr(), rowptr.data_ptr<int64_t>(),
              colidx.data_ptr<int>(), order, num_rows, D, g.bytes);
        });
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void seg_max_bwd(torch::Tensor dx, torch::Tensor dy, torch::Tensor arg,
                 torch::Tensor t_rowptr, torch::Tensor t_colidx,
                 torch::Tensor t_eperm,
                 c10::optional<torch::Tensor> t_row_order) {
  check_mat_pair(dx, "dx", dy, "dy", "seg_max_bwd");
  ROC_CHECK_DEV_CONT(arg);
  ROC_CHECK_DEV_CONT(t_eperm);
  TORCH_CHECK(dx.scalar_type() == dy.scalar_type(),
              "seg_max_bwd: dx and dy must share a dtype");
  const int num_src = (int)dx.size(0);
  const int64_t D = dx.size(1);
  TORCH_CHECK(arg.scalar_type() == torch::kInt32 && arg.sizes() == dy.sizes(),
              "seg_max_bwd: arg must be int32 with the shape of dy");
  check_csr_i32(t_rowptr, t_colidx, num_src, "seg_max_bwd");
  TORCH_CHECK(t_eperm.scalar_type() == torch::kInt32 &&
                  t_eperm.numel() == t_colidx.numel(),
              "seg_max_bwd: t_eperm must be int32, one entry per edge");
  if (num_src == 0 || D == 0) return;
  auto stream = roc_stream();
  dispatch_elt(dy.scalar_type(), "seg_max_bwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const GatherGeom g = seg_geom<T>(num_src, D, (size_t)dy.numel());
    const int* order = row_order_ptr(t_row_order, num_src, g.team, "seg_max_bwd");
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      hipLaunchKernelGGL(
          (seg_max_bwd_kernel<T, decltype(team_c)::value, kBwdDepth,
                              decltype(buf_c)::value>),
          g.grid, dim3(kBlock), 0, stream, (T*)dx.data_ptr(),
          (const T*)dy.data_ptr(), arg.data_ptr<int>(),
          t_rowptr.data_ptr<int64_t>(), t_colidx.data_ptr<int>(),
          t_eperm.data_ptr<int>(), order, num_src, D, g.bytes);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}
