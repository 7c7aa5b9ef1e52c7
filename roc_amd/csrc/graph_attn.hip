// Scaled dot-product attention over the in-neighbourhood for CDNA4 (the
// TransformerConv / UniMP family; the reference has no attention op).
//
// q  [n_local, D]   D = heads * dh
// kv [n_ext, 2*D]   columns [0, D) are K, [D, 2D) are V
//
// forward   s_e = scale * <q[v,h,:], K[u_e,h,:]>      e over the edges of row v
//           out[v,h,:] = sum_e softmax_e(s) * V[u_e,h,:]
//           lse[v,h]   = log sum_e exp(s_e)            fp32 [n_local, heads]
// backward  p_e = exp(s_e - lse),  delta = <dy, out>,  dp_e = <dy, V[u_e]>,
//           ds_e = p_e * (dp_e - delta)
//   dst pass (forward CSR)    dq[v]  = scale * sum_e ds_e * K[u_e]
//   src pass (transpose CSR)  dK[u]  = scale * sum_k ds_k * q[w_k]
//                             dV[u]  = sum_k p_k * dy[w_k]
//
// Same frame as spmm / seg_max: a row team owns one (row, head) pair at a
// time, blockIdx.y is the head, a lane owns one 16-B unit of the head
// slice. K and V (q and dy in the src pass) of a group of edges are
// gathered into statically indexed slots before the first use. The
// forward is an online softmax that rescales at every group; both
// backward passes recompute p from lse, so no [E] tensor exists in either
// direction and nothing is accumulated with atomics.
//
// Rules the tests pin:
//  - all arithmetic is fp32 over the exact bf16 widen; every stored value
//    is rounded once, at the store
//  - the running maximum is seeded from the row's first group (a flag, not
//    -inf arithmetic), so rows of very negative scores come out right
//  - sums run in ascending edge order inside a row and nowhere else, so
//    the result does not depend on the grid or on row_order
//  - a row without edges stores out = 0, lse = 0, dq = 0, delta = 0; a
//    source without out-edges stores dkv = 0
//  - lanes past dh / EPU of a team carry zeros into every reduction and
//    store nothing (they re-read lane 0's unit, which shares its line)
// The fast path needs dh % EPU == 0 and dh <= 64 * EPU. Any other dh >= 1
// runs the lane-strided scalar kernels at the end of this file.

#include "csr_launch.h"
#include "gather.h"

namespace {

// Edges in flight per lane; a group of G holds 2G payload slots. 8 keeps
// every fast-path instantiation out of scratch (docs/KERNELS.md has the
// resource table).
constexpr int kDepth = 8;
constexpr int kColdTeam = 8;

// the lane's partial of a head dot product, a fixed fma chain
template <int EPU>
__device__ __forceinline__ float unit_dot(const float* a, const float* b) {
  float s = a[0] * b[0];
#pragma unroll
  for (int j = 1; j < EPU; ++j) s = fmaf(a[j], b[j], s);
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

// Every kernel below makes two gather engines (gather.h): over one matrix
// (the K and V halves of kv) or over two matrices of one shape (q and dy),
// at the lane's column offsets.

// ---------------------------------------------------------------------------
// forward
// ---------------------------------------------------------------------------

struct Softmax {
  float m, l;
  bool first;
};

// N consecutive edges: scores, one rescale, then the fold in edge order
template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void fwd_group(
    Softmax& st, float* __restrict__ acc, const float* __restrict__ qf,
    float scale, const LD& ldk, const LD& ldv, const int* __restrict__ colidx,
    int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type k[N], v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) k[i] = ldk.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ldv.load(u[i]);
  float s[N];
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float kf[EPU];
    unpack(kf, k[i]);
    s[i] = scale * team_reduce_sum<TEAM>(unit_dot<EPU>(qf, kf));
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
    float vf[EPU];
    unpack(vf, v[i]);
    st.l += p;
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = fmaf(p, vf[j], acc[j]);
  }
}

template <typename T, int TEAM, bool BUF, bool LSE>
__global__ __launch_bounds__(kBlock) void graph_attn_fwd_kernel(
    T* __restrict__ out, float* __restrict__ lse, const T* __restrict__ q,
    const T* __restrict__ kv, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const int* __restrict__ row_order,
    int num_rows, int heads, int dh, float scale, unsigned kv_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ldk = make_gather<T, BUF>(kv, kv_bytes, 2 * D, col);
  const auto ldv = make_gather<T, BUF>(kv, kv_bytes, 2 * D, D + col);

  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    int64_t e = rowptr[row];
    const int64_t e1 = rowptr[row + 1];
    float qf[EPU], acc[EPU];
    load_unit(qf, q + (int64_t)row * D + col, active);
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    Softmax st{0.f, 0.f, true};
    ROC_EDGE_LADDER(kDepth, e, e1,
                    fwd_group<ROC_LADDER_N, T, TEAM>(st, acc, qf, scale, ldk,
                                                     ldv, colidx, e));
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
// backward, destination-major: delta and dq
// ---------------------------------------------------------------------------

template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void dst_group(
    float* __restrict__ acc, const float* __restrict__ qf,
    const float* __restrict__ gf, float scale, float lse, float delta,
    const LD& ldk, const LD& ldv, const int* __restrict__ colidx, int64_t e) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int u[N];
  typename RawVec<T>::type k[N], v[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) k[i] = ldk.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) v[i] = ldv.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float kf[EPU], vf[EPU];
    unpack(kf, k[i]);
    unpack(vf, v[i]);
    const float s = scale * team_reduce_sum<TEAM>(unit_dot<EPU>(qf, kf));
    const float dp = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, vf));
    const float ds = __expf(s - lse) * (dp - delta);
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = fmaf(ds, kf[j], acc[j]);
  }
}

template <typename T, int TEAM, bool BUF>
__global__ __launch_bounds__(kBlock) void graph_attn_bwd_dst_kernel(
    T* __restrict__ dq, float* __restrict__ delta, const T* __restrict__ dy,
    const T* __restrict__ out, const float* __restrict__ lse,
    const T* __restrict__ q, const T* __restrict__ kv,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int* __restrict__ row_order, int num_rows, int heads, int dh,
    float scale, unsigned kv_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ldk = make_gather<T, BUF>(kv, kv_bytes, 2 * D, col);
  const auto ldv = make_gather<T, BUF>(kv, kv_bytes, 2 * D, D + col);

  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    int64_t e = rowptr[row];
    const int64_t e1 = rowptr[row + 1];
    const int64_t at = (int64_t)row * D + col;
    float qf[EPU], gf[EPU], of[EPU], acc[EPU];
    load_unit(qf, q + at, active);
    load_unit(gf, dy + at, active);
    load_unit(of, out + at, active);
    const float dl = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, of));
    const float ls = lse[(int64_t)row * heads + h];
    if (rt.lane == 0) delta[(int64_t)row * heads + h] = dl;
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    ROC_EDGE_LADDER(kDepth, e, e1,
                    dst_group<ROC_LADDER_N, T, TEAM>(acc, qf, gf, scale, ls, dl,
                                                     ldk, ldv, colidx, e));
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] *= scale;
    if (active) store_vec(dq + at, acc);  // the one rounding
  }
}

// ---------------------------------------------------------------------------
// backward, source-major over the transpose CSR: dK and dV
// ---------------------------------------------------------------------------

template <int N, typename T, int TEAM, typename LD>
__device__ __forceinline__ void src_group(
    float* __restrict__ dk, float* __restrict__ dv,
    const float* __restrict__ kf, const float* __restrict__ vf, float scale,
    const float* __restrict__ lse, const float* __restrict__ delta, int heads,
    int h, const LD& ldq, const LD& ldg, const int* __restrict__ t_colidx,
    int64_t k) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  int w[N];
  typename RawVec<T>::type qr[N], gr[N];
  float ls[N], dl[N];
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = t_colidx[k + i];
#pragma unroll
  for (int i = 0; i < N; ++i) qr[i] = ldq.load(w[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) gr[i] = ldg.load(w[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) {
    ls[i] = lse[(int64_t)w[i] * heads + h];
    dl[i] = delta[(int64_t)w[i] * heads + h];
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    float qf[EPU], gf[EPU];
    unpack(qf, qr[i]);
    unpack(gf, gr[i]);
    const float s = scale * team_reduce_sum<TEAM>(unit_dot<EPU>(qf, kf));
    const float dp = team_reduce_sum<TEAM>(unit_dot<EPU>(gf, vf));
    const float p = __expf(s - ls[i]);
    const float ds = p * (dp - dl[i]);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      dk[j] = fmaf(ds, qf[j], dk[j]);
      dv[j] = fmaf(p, gf[j], dv[j]);
    }
  }
}

template <typename T, int TEAM, bool BUF>
__global__ __launch_bounds__(kBlock) void graph_attn_bwd_src_kernel(
    T* __restrict__ dkv, const T* __restrict__ q, const T* __restrict__ dy,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const T* __restrict__ kv, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, const int* __restrict__ t_row_order,
    int num_src, int heads, int dh, float scale, unsigned q_bytes) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  const bool active = rt.lane * EPU < dh;
  const int64_t col = (int64_t)h * dh + (active ? rt.lane * EPU : 0);
  const auto ldq = make_gather<T, BUF>(q, q_bytes, D, col);
  const auto ldg = make_gather<T, BUF>(dy, q_bytes, D, col);

  for (int ri = rt.team; ri < num_src; ri += rt.nteams) {
    const int u = t_row_order ? t_row_order[ri] : ri;
    int64_t k = t_rowptr[u];
    const int64_t k1 = t_rowptr[u + 1];
    const int64_t at = (int64_t)u * 2 * D + col;
    float kf[EPU], vf[EPU], dk[EPU], dv[EPU];
    load_unit(kf, kv + at, active);  // its own row, not a gather
    load_unit(vf, kv + at + D, active);
#pragma unroll
    for (int j = 0; j < EPU; ++j) dk[j] = dv[j] = 0.f;
    ROC_EDGE_LADDER(
        kDepth, k, k1,
        src_group<ROC_LADDER_N, T, TEAM>(dk, dv, kf, vf, scale, lse, delta,
                                         heads, h, ldq, ldg, t_colidx, k));
#pragma unroll
    for (int j = 0; j < EPU; ++j) dk[j] *= scale;
    if (active) {
      store_vec(dkv + at, dk);
      store_vec(dkv + at + D, dv);
    }
  }
}

// ---------------------------------------------------------------------------
// cold path: dh % EPU != 0, or dh > 64 * EPU. A head slice is not 16-B
// aligned, so column j of the head sits on lane j % 8 of a team of 8 and
// every load is a plain scalar one. A lane keeps ONE accumulator: the
// output columns are taken 8 at a time and every such chunk walks the
// row's edges again, recomputing the scores. That is dh / 8 walks of dh
// columns each; the path exists for narrow heads, where it is one or two.
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

template <typename T, bool LSE>
__global__ __launch_bounds__(kBlock) void graph_attn_fwd_cold_kernel(
    T* __restrict__ out, float* __restrict__ lse, const T* __restrict__ q,
    const T* __restrict__ kv, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, int num_rows, int heads, int dh,
    float scale) {
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    const T* qr = q + (int64_t)row * D + (int64_t)h * dh;
    // the row's maximum and normaliser, online one edge at a time
    float m = 0.f, l = 0.f;
    for (int64_t e = e0; e < e1; ++e) {
      const T* kr = kv + (int64_t)colidx[e] * 2 * D + (int64_t)h * dh;
      const float s = scale * cold_dot(qr, kr, dh, rt.lane);
      const float m_new = e == e0 ? s : fmaxf(m, s);
      l = (e == e0 ? 0.f : l * __expf(m - m_new)) + __expf(s - m_new);
      m = m_new;
    }
    const float inv = e0 < e1 ? 1.f / l : 0.f;
    for (int c = 0; c < dh; c += kColdTeam) {
      const int j = c + rt.lane;
      float acc = 0.f;
      for (int64_t e = e0; e < e1; ++e) {
        const T* kr = kv + (int64_t)colidx[e] * 2 * D + (int64_t)h * dh;
        const float s = scale * cold_dot(qr, kr, dh, rt.lane);
        if (j < dh) acc = fmaf(__expf(s - m), elt_to_f32(kr[D + j]), acc);
      }
      if (j < dh)
        f32_to_elt(acc * inv, out + (int64_t)row * D + (int64_t)h * dh + j);
    }
    if constexpr (LSE) {
      if (rt.lane == 0)
        lse[(int64_t)row * heads + h] = e0 < e1 ? m + logf(l) : 0.f;
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void graph_attn_bwd_dst_cold_kernel(
    T* __restrict__ dq, float* __restrict__ delta, const T* __restrict__ dy,
    const T* __restrict__ out, const float* __restrict__ lse,
    const T* __restrict__ q, const T* __restrict__ kv,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    int num_rows, int heads, int dh, float scale) {
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    const int64_t at = (int64_t)row * D + (int64_t)h * dh;
    const float dl = cold_dot(dy + at, out + at, dh, rt.lane);
    const float ls = lse[(int64_t)row * heads + h];
    if (rt.lane == 0) delta[(int64_t)row * heads + h] = dl;
    for (int c = 0; c < dh; c += kColdTeam) {
      const int j = c + rt.lane;
      float acc = 0.f;
      for (int64_t e = e0; e < e1; ++e) {
        const T* kr = kv + (int64_t)colidx[e] * 2 * D + (int64_t)h * dh;
        const float s = scale * cold_dot(q + at, kr, dh, rt.lane);
        const float dp = cold_dot(dy + at, kr + D, dh, rt.lane);
        const float ds = __expf(s - ls) * (dp - dl);
        if (j < dh) acc = fmaf(ds, elt_to_f32(kr[j]), acc);
      }
      if (j < dh) f32_to_elt(scale * acc, dq + at + j);
    }
  }
}

template <typename T>
__global__ __launch_bounds__(kBlock) void graph_attn_bwd_src_cold_kernel(
    T* __restrict__ dkv, const T* __restrict__ q, const T* __restrict__ dy,
    const float* __restrict__ lse, const float* __restrict__ delta,
    const T* __restrict__ kv, const int64_t* __restrict__ t_rowptr,
    const int* __restrict__ t_colidx, int num_src, int heads, int dh,
    float scale) {
  const RowTeam<kColdTeam> rt;
  const int h = blockIdx.y;
  const int64_t D = (int64_t)heads * dh;
  for (int u = rt.team; u < num_src; u += rt.nteams) {
    const int64_t k0 = t_rowptr[u], k1 = t_rowptr[u + 1];
    const int64_t at = (int64_t)u * 2 * D + (int64_t)h * dh;
    for (int c = 0; c < dh; c += kColdTeam) {
      const int j = c + rt.lane;
      float dk = 0.f, dv = 0.f;
      for (int64_t k = k0; k < k1; ++k) {
        const int w = t_colidx[k];
        const int64_t wt = (int64_t)w * D + (int64_t)h * dh;
        const float s = scale * cold_dot(q + wt, kv + at, dh, rt.lane);
        const float dp = cold_dot(dy + wt, kv + at + D, dh, rt.lane);
        const float p = __expf(s - lse[(int64_t)w * heads + h]);
        const float ds = p * (dp - delta[(int64_t)w * heads + h]);
        if (j < dh) {
          dk = fmaf(ds, elt_to_f32(q[wt + j]), dk);
          dv = fmaf(p, elt_to_f32(dy[wt + j]), dv);
        }
      }
      if (j < dh) {
        f32_to_elt(scale * dk, dkv + at + j);
        f32_to_elt(dv, dkv + at + D + j);
      }
    }
  }
}

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

// q-shaped [n, D] against kv-shaped [n_ext, 2D]; returns dh
int check_qkv(const torch::Tensor& q, const torch::Tensor& kv, int64_t heads,
              const char* what) {
  check_mat(q, what, "q");
  check_mat(kv, what, "kv");
  TORCH_CHECK(q.scalar_type() == kv.scalar_type(), what,
              ": q and kv must share a dtype");
  const int64_t D = q.size(1);
  TORCH_CHECK(kv.size(1) == 2 * D, what, ": kv must be [n_ext, 2*D]");
  TORCH_CHECK(heads >= 1 && heads <= 65535 && D >= heads && D % heads == 0,
              what, ": D must be a positive multiple of heads (<= 65535)");
  TORCH_CHECK(D < INT_MAX / 8, what, ": feature dim too large");
  return (int)(D / heads);
}

}  // namespace

void graph_attn_fwd(torch::Tensor out, c10::optional<torch::Tensor> lse,
                    torch::Tensor q, torch::Tensor kv, torch::Tensor rowptr,
                    torch::Tensor colidx,
                    c10::optional<torch::Tensor> row_order, int64_t heads,
                    double scale) {
  const int dh = check_qkv(q, kv, heads, "graph_attn_fwd");
  check_like(out, q, "graph_attn_fwd", "out");
  const int num_rows = (int)q.size(0);
  check_csr(rowptr, colidx, num_rows, "graph_attn_fwd");
  float* lsep = nullptr;
  if (lse.has_value()) {
    check_rowstat(*lse, num_rows, heads, "graph_attn_fwd", "lse");
    lsep = lse->data_ptr<float>();
  }
  if (num_rows == 0) return;
  if (colidx.numel() == 0) {  // no edge at all: zeros, no launch
    out.zero_();
    if (lsep) lse->zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), "graph_attn_fwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const AttnGeom a =
        attn_geom<T>(num_rows, (int)heads, dh, (size_t)kv.numel());
    const int* order = attn_order(row_order, num_rows, a, "graph_attn_fwd");
    dispatch_bool(lsep != nullptr, [&](auto lse_c) {
      if (!a.fast) {
        hipLaunchKernelGGL(
            (graph_attn_fwd_cold_kernel<T, decltype(lse_c)::value>), a.g.grid,
            dim3(kBlock), 0, stream, (T*)out.data_ptr(), lsep,
            (const T*)q.data_ptr(), (const T*)kv.data_ptr(),
            rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), num_rows,
            (int)heads, dh, (float)scale);
        return;
      }
      dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
        hipLaunchKernelGGL(
            (graph_attn_fwd_kernel<T, decltype(team_c)::value,
                                   decltype(buf_c)::value,
                                   decltype(lse_c)::value>),
            a.g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(), lsep,
            (const T*)q.data_ptr(), (const T*)kv.data_ptr(),
            rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), order,
            num_rows, (int)heads, dh, (float)scale, a.g.bytes);
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void graph_attn_bwd_dst(torch::Tensor dq, torch::Tensor delta,
                        torch::Tensor dy, torch::Tensor out, torch::Tensor lse,
                        torch::Tensor q, torch::Tensor kv,
                        torch::Tensor rowptr, torch::Tensor colidx,
                        c10::optional<torch::Tensor> row_order, int64_t heads,
                        double scale) {
  const int dh = check_qkv(q, kv, heads, "graph_attn_bwd_dst");
  check_like(dq, q, "graph_attn_bwd_dst", "dq");
  check_like(dy, q, "graph_attn_bwd_dst", "dy");
  check_like(out, q, "graph_attn_bwd_dst", "out");
  const int num_rows = (int)q.size(0);
  check_csr(rowptr, colidx, num_rows, "graph_attn_bwd_dst");
  check_rowstat(lse, num_rows, heads, "graph_attn_bwd_dst", "lse");
  check_rowstat(delta, num_rows, heads, "graph_attn_bwd_dst", "delta");
  if (num_rows == 0) return;
  if (colidx.numel() == 0) {
    dq.zero_();
    delta.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), "graph_attn_bwd_dst", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const AttnGeom a =
        attn_geom<T>(num_rows, (int)heads, dh, (size_t)kv.numel());
    const int* order =
        attn_order(row_order, num_rows, a, "graph_attn_bwd_dst");
    if (!a.fast) {
      hipLaunchKernelGGL(
          (graph_attn_bwd_dst_cold_kernel<T>), a.g.grid, dim3(kBlock), 0, stream,
          (T*)dq.data_ptr(), delta.data_ptr<float>(), (const T*)dy.data_ptr(),
          (const T*)out.data_ptr(), lse.data_ptr<float>(),
          (const T*)q.data_ptr(), (const T*)kv.data_ptr(),
          rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), num_rows,
          (int)heads, dh, (float)scale);
      return;
    }
    dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
      hipLaunchKernelGGL(
          (graph_attn_bwd_dst_kernel<T, decltype(team_c)::value,
                                     decltype(buf_c)::value>),
          a.g.grid, dim3(kBlock), 0, stream, (T*)dq.data_ptr(),
          delta.data_ptr<float>(), (const T*)dy.data_ptr(),
          (const T*)out.data_ptr(), lse.data_ptr<float>(),
          (const T*)q.data_ptr(), (const T*)kv.data_ptr(),
          rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(), order, num_rows,
          (int)heads, dh, (float)scale, a.g.bytes);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void graph_attn_bwd_src(torch::Tensor dkv, torch::Tensor q, torch::Tensor dy,
                        torch::Tensor lse, torch::Tensor delta,
                        torch::Tensor kv, torch::Tensor t_rowptr,
                        torch::Tensor t_colidx,
                        c10::optional<torch::Tensor> t_row_order,
                        int64_t heads, double scale) {
  const int dh = check_qkv(q, kv, heads, "graph_attn_bwd_src");
  check_like(dkv, kv, "graph_attn_bwd_src", "dkv");
  check_like(dy, q, "graph_attn_bwd_src", "dy");
  const int num_rows = (int)q.size(0);
  const int num_src = (int)kv.size(0);
  check_csr(t_rowptr, t_colidx, num_src, "graph_attn_bwd_src");
  check_rowstat(lse, num_rows, heads, "graph_attn_bwd_src", "lse");
  check_rowstat(delta, num_rows, heads, "graph_attn_bwd_src", "delta");
  if (num_src == 0) return;
  if (t_colidx.numel() == 0 || num_rows == 0) {
    dkv.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(q.scalar_type(), "graph_attn_bwd_src", [&](auto xt) {
    using T = typename decltype(xt)::type;
    // the src pass gathers rows of q and dy, so the buffer spans q
    const AttnGeom a =
        attn_geom<T>(num_src, (int)heads, dh, (size_t)q.numel());
    const int* order = attn_order(t_row_order, num_src, a, "graph_attn_bwd_src");
    if (!a.fast) {
      hipLaunchKernelGGL(
          (graph_attn_bwd_src_cold_kernel<T>), a.g.grid, dim3(kBlock), 0, stream,
          (T*)dkv.data_ptr(), (const T*)q.data_ptr(), (const T*)dy.data_ptr(),
          lse.data_ptr<float>(), delta.data_ptr<float>(),
          (const T*)kv.data_ptr(), t_rowptr.data_ptr<int64_t>(),
          t_colidx.data_ptr<int>(), num_src, (int)heads, dh, (float)scale);
      return;
    }
    dispatch_gather(a.g, [&](auto team_c, auto buf_c) {
      hipLaunchKernelGGL(
          (graph_attn_bwd_src_kernel<T, decltype(team_c)::value,
                                     decltype(buf_c)::value>),
          a.g.grid, dim3(kBlock), 0, stream, (T*)dkv.data_ptr(),
          (const T*)q.data_ptr(), (const T*)dy.data_ptr(),
          lse.data_ptr<float>(), delta.data_ptr<float>(),
          (const T*)kv.data_ptr(), t_rowptr.data_ptr<int64_t>(),
          t_colidx.data_ptr<int>(), order, num_src, (int)heads, dh,
          (float)scale, a.g.bytes);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}
