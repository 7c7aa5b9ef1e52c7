// CSR SpMM neighbor aggregation for CDNA4 — the hot GNN op.
//
// out[v, :] = (deg_dst[v] *) sum_{e in row v} (w_e *) x[u_e, :]
// with w_e one of: nothing, deg_src[u_e] (per source), edge_val[e] (per
// edge) — one kernel body, the weight source is a compile-time policy.
//
// MI355X-native design (vs reference `scattergather_kernel.cu:20-76`,
// which staged the full graph tensor host->FB per task and used
// cub-scan + LDS atomics):
//  - features stay HBM/L3-resident; no host staging
//  - a "row team" of TEAM lanes owns one row at a time (row_team.h); each
//    lane accumulates EPU output elements in registers (no LDS, no atomics)
//  - 16-B vectorized gathers (uint4 of 8 bf16 / float4), up to 16 in flight
//  - optional fused degree scaling (deg_* are precomputed factors); the
//    fast GCN path pre-scales sources in the GEMM epilogue so only the
//    cheap per-row dst factor remains here
//  - rows are visited in degree-descending order (row_order) so hub rows
//    start first and the skew tail is hidden (Reddit max degree >> mean)
//  - wide feature dims are column-tiled across blockIdx.y
//  - source-strip passes (fp32 partials) start the rows that are heavy in
//    their strip first, from a short list, and the last pass stores the
//    bf16 result itself (HEAVY / FINAL variants of spmm_kernel)
//
// The vector path and the (rare) partial-unit tail path are fully
// separated: the hot path's per-slot buffers are only ever statically
// indexed, so nothing lands in scratch (a shared runtime-indexed array
// cost 144 B/lane of scratch and 3x wall time — see
// profiles/r02 notes / CDNA guide §5.4 rule 20).
// Backward runs this same kernel on the transpose CSR (exact on
// asymmetric graphs; the reference assumed symmetry).

#include "csr_launch.h"
#include "gather.h"

namespace {

__device__ __forceinline__ void acc_add(float* acc, const uint4& r, float w) {
  acc[0] += w * bf16_lo(r.x); acc[1] += w * bf16_hi(r.x);
  acc[2] += w * bf16_lo(r.y); acc[3] += w * bf16_hi(r.y);
  acc[4] += w * bf16_lo(r.z); acc[5] += w * bf16_hi(r.z);
  acc[6] += w * bf16_lo(r.w); acc[7] += w * bf16_hi(r.w);
}
__device__ __forceinline__ void acc_add(float* acc, const float4& r, float w) {
  acc[0] += w * r.x; acc[1] += w * r.y; acc[2] += w * r.z; acc[3] += w * r.w;
}

// Where the per-gather weight comes from. It is compile-time because the
// fused GCN path has none: kNone must stay a plain add, and dropping the
// dead deg_src lookups frees the index registers (they otherwise stay
// live across all in-flight gathers).
enum class Weight { kNone, kSrc, kEdge };  // 1 | w[u_e] | w[e]

// acc += w_e * x[u_e, unit] for N consecutive edges. Per-edge weights are
// sequential, so they load before the gathers issue (one scalar broadcast
// per gather); per-source weights are looked up as the payloads land.
template <int N, typename T, Weight W, typename LD>
__device__ __forceinline__ void accum_group(
    float* __restrict__ acc, const LD& ld, const int* __restrict__ colidx,
    const float* __restrict__ weight, int64_t e) {
  float w[N];
  if constexpr (W == Weight::kEdge) {
#pragma unroll
    for (int i = 0; i < N; ++i) w[i] = weight[e + i];
  }
  gather_group<N, T>(ld, colidx, e,
                     [&](int i, int u, const typename RawVec<T>::type& r) {
    if constexpr (W == Weight::kEdge) acc_add(acc, r, w[i]);
    else if constexpr (W == Weight::kSrc) acc_add(acc, r, weight[u]);
    else acc_add(acc, r, 1.f);
  });
}

// hot path: this lane's 16-B unit is entirely inside the column window.
// The ladder keeps UN gathers in flight, then steps down; within a row
// the accumulation order is always ascending in e.
template <typename T, int UN, Weight W, typename LD>
__device__ __forceinline__ void row_accum_vec(
    float* __restrict__ acc, const LD& ld, const int* __restrict__ colidx,
    const float* __restrict__ weight, int64_t e, int64_t e1) {
  ROC_EDGE_LADDER(
      UN, e, e1,
      accum_group<ROC_LADDER_N, T, W>(acc, ld, colidx, weight, e));
}

// tail path: unit straddles the column window (only when its width is
// not a multiple of EPU; engine pads dims to 8 so this is cold).
// Scalar loads, dynamic-bound loops. The per-source weight keeps a
// run-time null check here (weight is null for Weight::kNone): resolving
// it at compile time changes nothing on this path, but without it the
// allocator packs the 8-deep no-weight kernels into 58 VGPRs / 8 waves
// and serialises their unpack behind the last gather, which measured
// 2-4% slower than 88 VGPRs / 5 waves (profiles/r37).
template <typename T, Weight W>
__device__ void row_accum_tail(
    float* __restrict__ acc, const T* __restrict__ x, int64_t ld, int64_t col0,
    int nvalid, const int* __restrict__ colidx,
    const float* __restrict__ weight, int64_t e0, int64_t e1) {
  for (int64_t e = e0; e < e1; ++e) {
    const int u0 = colidx[e];
    const T* r = x + (int64_t)u0 * ld + col0;
    const float w0 =
        W == Weight::kEdge ? weight[e] : (weight ? weight[u0] : 1.f);
    for (int j = 0; j < nvalid; ++j) acc[j] += w0 * elt_to_f32(r[j]);
  }
}

// (a forced 6-waves/SIMD __launch_bounds__ hint was measured NEUTRAL:
//  the allocator spills 28 B/lane on half the hot variants and any
//  occupancy gain washes out — keep the default allocation)
// OT (output type) may differ from T: OT=float with T=bf16 is the
// strip-blocked accumulation path — fp32 partials in HBM, one rounding
// at the final cast instead of one per strip pass.
// ld is the row stride; [col_base, col_end) is the column window this
// launch covers (ld == col_end, col_base == 0 for a whole-matrix pass;
// a column-phase pass sweeps a 64-col window of a wider matrix so the
// fp32 partial buffer is touched once per much-wider source strip).
// `weight` is deg_src (indexed by source) or edge_val (indexed by edge)
// as W says; unused for Weight::kNone.
//
// Two compile-time variants serve the strip passes (bf16 x, fp32
// partials, no weight); with both off the kernel is the plain one:
//  HEAVY  heavy-first schedule. `heavy_rows` lists exactly the rows with
//         e1 - e0 >= heavy_min, longest first. A team takes its share of
//         that list before its natural sweep, and the sweep skips those
//         rows by the rowptr values it has loaded anyway: light rows pay
//         no indirection. The list is dealt out a wave at a time: the
//         64/TEAM teams of one wave take consecutive entries (rows of
//         about equal length, so no team idles while its wave-mates
//         finish a long row — measured 3-11% of a pass over dealing
//         single entries, profiles/r38), and consecutive waves' worth go
//         to consecutive workgroups, so the longest rows start in the
//         first resident wave on different CUs. One loop serves both
//         phases, so a wave whose teams are in different phases still
//         shares the gather code.
//         Which team owns a row never changes the row's own summation
//         order, so results equal the plain pass bit for bit.
//  FINAL  last strip pass: the finished row goes to `final_out` as bf16
//         (after the optional deg_dst scale) and the fp32 partials are
//         only read — the separate cast pass over memory disappears.
template <typename T, typename OT, int TEAM, int UN, bool BUF, Weight W,
          bool HEAVY = false, bool FINAL = false>
__global__ __launch_bounds__(kBlock) void spmm_kernel(
    OT* __restrict__ out, const T* __restrict__ x,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const float* __restrict__ deg_dst, const float* __restrict__ weight,
    const int* __restrict__ row_order, int num_rows, int64_t ld,
    int64_t col_base, int64_t col_end, bool accumulate, unsigned x_bytes,
    const int* __restrict__ heavy_rows, int num_heavy, int heavy_min,
    unsigned short* __restrict__ final_out) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;

  const int64_t col0 =
      col_base + ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = (col0 + EPU) <= col_end;
  const int nvalid =
      full ? EPU : (col0 < col_end ? (int)(col_end - col0) : 0);

  if (full) {
    auto do_row = [&](int row, int64_t e0, int64_t e1) {
      float acc[EPU];
      OT* o = out + (int64_t)row * ld + col0;
      if (accumulate) {  // strip / halo-overlap pass 2: from partials
#pragma unroll
        for (int j = 0; j < EPU; ++j) acc[j] = elt_to_f32(o[j]);
      } else {
#pragma unroll
        for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
      }
      const auto g = make_gather<T, BUF>(x, x_bytes, ld, col0);
      row_accum_vec<T, UN, W>(acc, g, colidx, weight, e0, e1);
      if (deg_dst) {
        const float s = deg_dst[row];
#pragma unroll
        for (int j = 0; j < EPU; ++j) acc[j] *= s;
      }
      if constexpr (FINAL) store_vec(final_out + (int64_t)row * ld + col0, acc);
      else store_vec(o, acc);
    };
    if constexpr (HEAVY) {
      // list entry h: wave-sized runs of entries go round the workgroups
      constexpr int TPW = 64 / TEAM;  // teams per wave
      const int lt = (int)threadIdx.x / TEAM;
      int h = ((lt / TPW) * (int)gridDim.x + (int)blockIdx.x) * TPW + lt % TPW;
      int ri = rt.team;
      for (;;) {
        int row;
        const bool from_list = h < num_heavy;
        if (from_list) {
          row = heavy_rows[h];
          h += rt.nteams;
          if ((unsigned)row >= (unsigned)num_rows) continue;  // bad entry
        } else {
          if (ri >= num_rows) break;
          row = ri;
          ri += rt.nteams;
        }
        const int64_t e0 = rowptr[row];
        const int64_t e1 = rowptr[row + 1];
        if (!from_list && e1 - e0 >= heavy_min) continue;  // done above
        do_row(row, e0, e1);
      }
    } else {
      for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
        const int row = row_order ? row_order[ri] : ri;
        do_row(row, rowptr[row], rowptr[row + 1]);
      }
    }
  } else if (nvalid > 0) {
    // cold path: natural sweep whatever the schedule variant
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      float acc[EPU];
      OT* o = out + (int64_t)row * ld + col0;
      for (int j = 0; j < nvalid; ++j)
        acc[j] = accumulate ? elt_to_f32(o[j]) : 0.f;
      row_accum_tail<T, W>(acc, x, ld, col0, nvalid, colidx, weight,
                           rowptr[row], rowptr[row + 1]);
      const float s = deg_dst ? deg_dst[row] : 1.f;
      if constexpr (FINAL) {
        unsigned short* fo = final_out + (int64_t)row * ld + col0;
        for (int j = 0; j < nvalid; ++j) f32_to_elt(acc[j] * s, fo + j);
      } else {
        for (int j = 0; j < nvalid; ++j) f32_to_elt(acc[j] * s, o + j);
      }
    }
  }
}

// A/B geometry knobs, pinned ONCE at first launch (a per-launch getenv
// on the hot path is a footgun under hipGraph capture: replays would
// silently keep whatever value was live at capture; now ALL launches —
// captured or eager — use the same process-lifetime values).
struct SpmmKnobs {
  int team_override;  // 0 = auto (by D); else 8/16/32/64
  int unroll;         // 4 | 8 | 16 (16 measured best)
  bool allow_buffer;  // SRSRC buffer_load gather path
};

static SpmmKnobs read_spmm_knobs() {
  SpmmKnobs k{0, 16, true};
  if (const char* e = getenv("ROC_SPMM_TEAM")) {
    const int t = atoi(e);
    if (t == 8 || t == 16 || t == 32 || t == 64) k.team_override = t;
  }
  if (const char* e = getenv("ROC_SPMM_UNROLL")) k.unroll = atoi(e);
  if (const char* e = getenv("ROC_SPMM_BUFFER")) k.allow_buffer = e[0] != '0';
  return k;
}

static SpmmKnobs g_spmm_knobs;
static bool g_spmm_knobs_read = false;

static const SpmmKnobs& spmm_knobs() {
  if (!g_spmm_knobs_read) {
    g_spmm_knobs = read_spmm_knobs();
    g_spmm_knobs_read = true;
  }
  return g_spmm_knobs;
}

// The one spmm_kernel launch: geometry from the column window, gather
// engine from the matrix size (csr_launch.h). team_override == 0 picks the
// team by width; `what` names the op in the row_order message.
// The strip-pass extras of one launch (see spmm_kernel): the heavy-first
// list with its threshold, and the bf16 destination of a final pass.
struct StripPass {
  bool heavy = false;  // heavy_rows given (it may be empty)
  const int* heavy_rows = nullptr;
  int num_heavy = 0;
  int heavy_min = 0;
  unsigned short* final_out = nullptr;
};

template <typename T, typename OT, int UN, Weight W, bool HEAVY = false,
          bool FINAL = false>
void launch_spmm(OT* out, const T* x, const int64_t* rowptr,
                 const int* colidx, const float* deg_dst, const float* weight,
                 const c10::optional<torch::Tensor>& row_order, int num_rows,
                 int64_t ld, int64_t col_base, int64_t col_end,
                 bool accumulate, size_t x_elems, int team_override,
                 const char* what, hipStream_t stream,
                 const StripPass& sp = {}) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const GatherGeom g = gather_geom<T>(
      num_rows, (col_end - col_base + EPU - 1) / EPU, 0, x_elems,
      spmm_knobs().allow_buffer, team_override);
  const int* order = row_order_ptr(row_order, num_rows, g.team, what);
  dispatch_gather(g, [&](auto team_c, auto buf_c) {
    hipLaunchKernelGGL(
        (spmm_kernel<T, OT, decltype(team_c)::value, UN,
                     decltype(buf_c)::value, W, HEAVY, FINAL>),
        g.grid, dim3(kBlock), 0, stream, out, x, rowptr, colidx, deg_dst,
        weight, order, num_rows, ld, col_base, col_end, accumulate, g.bytes,
        sp.heavy_rows, sp.num_heavy, sp.heavy_min, sp.final_out);
  });
}

// dw[e] = <dy[row_e,:], x[col_e,:]>  (fp32 accumulate) — the edge-value
// gradient of the per-edge-weighted SpMM.
// Team per row; per edge each lane dots its strided D-chunks, then a
// team_reduce_sum folds the team partials; lane 0 stores.
template <typename T, int EPU>
__device__ __forceinline__ float dot_unit(
    const float (&a)[EPU], const typename RawVec<T>::type& r) {
  float b[EPU];
#pragma unroll
  for (int j = 0; j < EPU; ++j) b[j] = 0.f;
  acc_add(b, r, 1.f);
  float p = 0.f;
#pragma unroll
  for (int j = 0; j < EPU; ++j) p += a[j] * b[j];
  return p;
}

// N edges of the fast path: gathers queued N deep, N team folds, N stores
template <int N, typename T, int TEAM, int EPU>
__device__ __forceinline__ void edge_dot_group(
    float* __restrict__ dw, const float (&a)[EPU], const GlobalGather<T>& g,
    const int* __restrict__ colidx, int64_t e, bool live, int lane) {
  float p[N];
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = 0.f;
  if (live)
    gather_group<N, T>(g, colidx, e,
                       [&](int i, int, const typename RawVec<T>::type& r) {
      p[i] = dot_unit<T>(a, r);
    });
#pragma unroll
  for (int i = 0; i < N; ++i) p[i] = team_reduce_sum<TEAM>(p[i]);
  if (lane == 0) {
#pragma unroll
    for (int i = 0; i < N; ++i) dw[e + i] = p[i];
  }
}

template <typename T, int TEAM>
__global__ __launch_bounds__(kBlock) void edge_dot_kernel(
    float* __restrict__ dw, const T* __restrict__ dy,
    const T* __restrict__ x, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, int num_rows, int64_t D) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  using Raw = typename RawVec<T>::type;
  const RowTeam<TEAM> rt;
  const int lane = rt.lane;
  // fast path: one chunk covers D (TEAM*EPU >= D, e.g. TEAM=8 D<=64
  // bf16). The dy row chunk is loaded ONCE per row (hoisted out of the
  // edge loop) and x gathers are queued 4 deep — the naive per-edge
  // load/reduce version was 4x off the gather-service rate (r2c16).
  if ((int64_t)TEAM * EPU >= D && D % EPU == 0) {
    const bool live = lane < (int)(D / EPU);  // lane has a chunk
    const GlobalGather<T> g{x, D, (int64_t)lane * EPU};
    for (int row = rt.team; row < num_rows; row += rt.nteams) {
      const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
      float a[EPU] = {0.f};
      if (live) acc_add(a, load_raw(dy + (int64_t)row * D + g.col0), 1.f);
      int64_t e = e0;
      ROC_EDGE_LADDER(4, e, e1,
                      edge_dot_group<ROC_LADDER_N, T, TEAM>(dw, a, g, colidx, e,
                                                            live, lane));
    }
    return;
  }
  // general path (wide D): chunk loop per edge
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t e0 = rowptr[row], e1 = rowptr[row + 1];
    const T* dyr = dy + (int64_t)row * D;
    for (int64_t e = e0; e < e1; ++e) {
      const T* xr = x + (int64_t)colidx[e] * D;
      float p = 0.f;
      for (int64_t c = (int64_t)lane * EPU; c + EPU <= D;
           c += (int64_t)TEAM * EPU) {
        const Raw a = load_raw(dyr + c);
        const Raw b = load_raw(xr + c);
        float ta[EPU] = {0.f}, tb[EPU] = {0.f};
        acc_add(ta, a, 1.f);
        acc_add(tb, b, 1.f);
#pragma unroll
        for (int j = 0; j < EPU; ++j) p += ta[j] * tb[j];
      }
      // scalar tail, lane-strided, for D % EPU != 0 (cold; dims padded)
      for (int64_t j = (D / EPU) * EPU + lane; j < D; j += TEAM)
        p += elt_to_f32(dyr[j]) * elt_to_f32(xr[j]);
      p = team_reduce_sum<TEAM>(p);
      if (lane == 0) dw[e] = p;
    }
  }
}

template <typename T>
void launch_edge_dot(float* dw, const T* dy, const T* x,
                     const int64_t* rowptr, const int* colidx, int num_rows,
                     int64_t D, hipStream_t stream) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const int team = row_team_size((D + EPU - 1) / EPU);
  dispatch_team(team, [&](auto team_c) {
    hipLaunchKernelGGL((edge_dot_kernel<T, decltype(team_c)::value>),
                       row_team_grid(num_rows, team), dim3(kBlock), 0, stream,
                       dw, dy, x, rowptr, colidx, num_rows, D);
  });
}

template <typename T>
const T* opt_ptr(const c10::optional<torch::Tensor>& t) {
  return t.has_value() ? t->data_ptr<T>() : nullptr;
}

}  // namespace

// A/B harness hook (scripts/bench_spmm.py): re-read the geometry env
// vars. Never call while a hipGraph capture of spmm launches is live.
void spmm_refresh_knobs() { g_spmm_knobs_read = false; }

void spmm(torch::Tensor out, torch::Tensor x, torch::Tensor rowptr,
          torch::Tensor colidx, c10::optional<torch::Tensor> deg_dst,
          c10::optional<torch::Tensor> deg_src,
          c10::optional<torch::Tensor> row_order, bool accumulate,
          int64_t col_base, int64_t ncols,
          c10::optional<torch::Tensor> heavy_rows, int64_t heavy_min,
          c10::optional<torch::Tensor> final_out) {
  check_mat_pair(out, "out", x, "x", "spmm");
  // strip-pass extras: heavy-first schedule and fused final bf16 store
  StripPass sp;
  if (heavy_rows.has_value() || final_out.has_value()) {
    TORCH_CHECK(out.scalar_type() == torch::kFloat32 &&
                    x.scalar_type() == torch::kBFloat16 &&
                    !deg_src.has_value(),
                "spmm: heavy_rows / final_out are strip-pass options: "
                "bf16 x, fp32 out, no deg_src");
  }
  if (heavy_rows.has_value()) {
    ROC_CHECK_DEV_CONT(*heavy_rows);
    TORCH_CHECK(heavy_rows->scalar_type() == torch::kInt32,
                "spmm: heavy_rows must be int32");
    TORCH_CHECK(!row_order.has_value(),
                "spmm: heavy_rows and row_order are exclusive");
    TORCH_CHECK(heavy_min >= 0 && heavy_min <= INT_MAX,
                "spmm: bad heavy_min");
    sp.heavy = true;
    sp.heavy_rows = heavy_rows->data_ptr<int>();
    sp.num_heavy = (int)heavy_rows->numel();
    sp.heavy_min = (int)heavy_min;
  }
  if (final_out.has_value()) {
    ROC_CHECK_DEV_CONT(*final_out);
    TORCH_CHECK(final_out->scalar_type() == torch::kBFloat16,
                "spmm: final_out must be bf16");
    TORCH_CHECK(final_out->sizes() == out.sizes(),
                "spmm: final_out shape mismatch");
    TORCH_CHECK(col_base == 0 && ncols == 0,
                "spmm: final_out needs a whole-row pass");
    sp.final_out = (unsigned short*)final_out->data_ptr();
  }
  TORCH_CHECK(out.scalar_type() == x.scalar_type() ||
                  (out.scalar_type() == torch::kFloat32 &&
                   x.scalar_type() == torch::kBFloat16),
              "spmm: dtype mismatch (out must match x, or be fp32 for bf16 x)");
  const int num_rows = (int)out.size(0);
  const int64_t D = out.size(1);
  check_csr(rowptr, colidx, num_rows, "spmm");
  // column-phase pass: touch only [col_base, col_base+ncols) of every
  // row (ncols == 0 -> the whole row). The stride stays D.
  const int64_t col_end = ncols > 0 ? col_base + ncols : D;
  TORCH_CHECK(col_base >= 0 && col_base < col_end && col_end <= D,
              "spmm: bad column window");
  const float* ds = opt_ptr<float>(deg_src);
  const SpmmKnobs& kn = spmm_knobs();
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "spmm", [&](auto xt) {
    dispatch_elt(out.scalar_type(), "spmm", [&](auto ot) {
      using T = typename decltype(xt)::type;
      using OT = typename decltype(ot)::type;
      // (fp32 x with bf16 out is rejected above and never instantiated)
      if constexpr (sizeof(OT) >= sizeof(T)) {
        auto go = [&](auto un_c, auto w_c) {
          constexpr int UN = decltype(un_c)::value;
          constexpr Weight W = decltype(w_c)::value;
          auto launch = [&](auto heavy_c, auto final_c) {
            launch_spmm<T, OT, UN, W, decltype(heavy_c)::value,
                        decltype(final_c)::value>(
                (OT*)out.data_ptr(), (const T*)x.data_ptr(),
                rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(),
                opt_ptr<float>(deg_dst), ds, row_order, num_rows, D,
                col_base, col_end, accumulate, (size_t)x.numel(),
                kn.team_override, "spmm", stream, sp);
          };
          // the strip-pass variants exist for bf16 -> fp32, no weight only
          // (checked above), so nothing else is instantiated with them
          if constexpr (std::is_same_v<T, unsigned short> &&
                        std::is_same_v<OT, float> && W == Weight::kNone) {
            if (sp.heavy || sp.final_out) {
              dispatch_bool(sp.heavy, [&](auto heavy_c) {
                dispatch_bool(sp.final_out != nullptr,
                              [&](auto final_c) { launch(heavy_c, final_c); });
              });
              return;
            }
          }
          launch(std::false_type{}, std::false_type{});
        };
        auto by_weight = [&](auto un_c) {
          if (ds) go(un_c, std::integral_constant<Weight, Weight::kSrc>{});
          else go(un_c, std::integral_constant<Weight, Weight::kNone>{});
        };
        if (kn.unroll >= 16) by_weight(std::integral_constant<int, 16>{});
        else if (kn.unroll >= 8) by_weight(std::integral_constant<int, 8>{});
        else by_weight(std::integral_constant<int, 4>{});
      }
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

// Per-edge-weighted SpMM (the edge-tensor op):
// out[v,:] (+)= deg_dst[v] * sum_{e in row v} edge_val[e] * x[col_e,:]
// Capability path, not the fused-GCN hot path, so one unroll depth (4),
// OT == T and the whole-matrix window are all it instantiates.
void spmm_edge(torch::Tensor out, torch::Tensor x, torch::Tensor rowptr,
               torch::Tensor colidx, torch::Tensor edge_val,
               c10::optional<torch::Tensor> deg_dst,
               c10::optional<torch::Tensor> row_order, bool accumulate) {
  check_mat_pair(out, "out", x, "x", "spmm_edge");
  ROC_CHECK_DEV_CONT(edge_val);
  TORCH_CHECK(edge_val.scalar_type() == torch::kFloat32,
              "spmm_edge: edge_val must be fp32");
  TORCH_CHECK(edge_val.numel() == colidx.numel(),
              "spmm_edge: edge_val size mismatch");
  TORCH_CHECK(out.scalar_type() == x.scalar_type(),
              "spmm_edge: dtype mismatch");
  const int num_rows = (int)out.size(0);
  const int64_t D = out.size(1);
  check_csr(rowptr, colidx, num_rows, "spmm_edge");
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "spmm_edge", [&](auto xt) {
    using T = typename decltype(xt)::type;
    launch_spmm<T, T, 4, Weight::kEdge>(
        (T*)out.data_ptr(), (const T*)x.data_ptr(),
        rowptr.data_ptr<int64_t>(), colidx.data_ptr<int>(),
        opt_ptr<float>(deg_dst), edge_val.data_ptr<float>(), row_order,
        num_rows, D, 0, D, accumulate, (size_t)x.numel(), 0, "spmm_edge",
        stream);
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void edge_dot(torch::Tensor dw, torch::Tensor dy, torch::Tensor x,
              torch::Tensor rowptr, torch::Tensor colidx) {
  ROC_CHECK_DEV_CONT(dw);
  check_mat_pair(dy, "dy", x, "x", "edge_dot");
  TORCH_CHECK(dw.scalar_type() == torch::kFloat32, "edge_dot: dw must be fp32");
  TORCH_CHECK(dw.numel() == colidx.numel(), "edge_dot: dw size mismatch");
  TORCH_CHECK(dy.scalar_type() == x.scalar_type(), "edge_dot: dtype mismatch");
  const int num_rows = (int)dy.size(0);
  const int64_t D = dy.size(1);
  check_csr(rowptr, colidx, num_rows, "edge_dot");
  auto stream = roc_stream();
  dispatch_elt(dy.scalar_type(), "edge_dot", [&](auto xt) {
    using T = typename decltype(xt)::type;
    launch_edge_dot<T>(dw.data_ptr<float>(), (const T*)dy.data_ptr(),
                       (const T*)x.data_ptr(), rowptr.data_ptr<int64_t>(),
                       colidx.data_ptr<int>(), num_rows, D, stream);
  });
  ROC_HIP_CHECK(hipGetLastError());
}
