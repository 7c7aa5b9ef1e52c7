// FP8 neighbour aggregation for CDNA4: an e4m3 row quantiser with per-row
// power-of-two scales, and the CSR SpMM that gathers those rows.
//
//   quantise  y = x[r] * pre_scale[r]            (one fp32 multiply)
//             s[r] = 2^k, k the smallest integer with max_j |y_j| <= 448 * 2^k
//             q[r, j] = RNE_e4m3(y_j / s[r])     (an exact exponent shift)
//   spmm      out[v, :] = (deg_dst[v] *) sum_{e in row v} s[u_e] * q[u_e, :]
//
// A gathered row is half the bytes of a bf16 row; the price is one 4-B scale
// load per edge. The scales are powers of two so that s * decode(q) is exact
// in fp32: the sum is then the plain ascending fp32 sum of exact terms, and
// the whole path has a bit-exact CPU reference (ops/reference.py).
//
// Rules the tests pin:
//  - the format is OCP e4m3 (bias 7, max 448, no inf, subnormals, -0), as the
//    gfx950 converts implement it and as torch.float8_e4m3fn defines it
//  - k is read off the bits of amax = m * 2^e, m in [0.5, 1): k = e - 9 if
//    m <= 0.875 else e - 8; amax == 0 gives s = 1. k is held at >= kMinExp so
//    that s, 1/s and every product s * decode(q) stay normal fp32 numbers: a
//    row whose amax is below 448 * 2^kMinExp keeps s = 2^kMinExp and rounds
//    towards zero like any small value
//  - y / s is clamped to +-448 before the convert (it never exceeds it)
//  - NaN and +-inf inputs are out of contract
//  - the SpMM accumulates in fp32 in ascending edge order from 0 (or from the
//    fp32 partial of an earlier strip pass), multiplies by deg_dst once and
//    rounds once, at the store; empty rows store 0
//  - D % 16 == 0: every lane's 16-B unit is whole or absent, there is no tail
//    path and no column window
//
// The SpMM kernel is spmm_kernel's frame (spmm.hip) with the fp8 payload: the
// same row team, column tiles, gather engines, row order, and the HEAVY /
// FINAL / PERM strip-pass variants, so it runs every plan _strip_spmm runs
// for whole-row bf16, unchanged. Its ladder rung is its own: the scale of a
// source is on the critical path of every add of its row, so a rung issues
// its N payload gathers and its N scale loads back to back before the first
// use, where Weight::kSrc looks the weight up as the payloads land.

#include "csr_launch.h"
#include "gather.h"

// Every function of this file is built without the packed fp32 ALU forms
// (v_pk_fma_f32 and kin): the 16-wide accumulate is exactly the pattern the
// compiler packs, and the scalar forms are the ones the rest of the library
// is validated on.
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

typedef unsigned char fp8_t;

constexpr int kMaxD = 1024;
constexpr int kMinExp = -100;
constexpr int kQuantGridCap = 2048;

// ---- quantiser ------------------------------------------------------------
// layer_norm's geometry: a RowTeam<TEAM> holds the whole bf16 row in
// registers, UNITS 16-B units per lane (unit k of a lane covers columns
// (k*TEAM + lane)*8 ...), amax goes through the team tree, x is read once and
// q written once, 8 bytes per unit in one store. D % 16 == 0, so a unit is
// whole or past D.
template <int TEAM, int UNITS>
__global__ __launch_bounds__(kBlock) void quantize_rows_fp8_kernel(
    fp8_t* __restrict__ q, float* __restrict__ s,
    const unsigned short* __restrict__ x, const float* __restrict__ pre_scale,
    int num_rows, int D) {
  const RowTeam<TEAM> rt;
  int col0[UNITS];
  bool live[UNITS];
#pragma unroll
  for (int k = 0; k < UNITS; ++k) {
    col0[k] = (k * TEAM + rt.lane) * 8;
    live[k] = col0[k] < D;
  }
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t base = (int64_t)row * D;
    const float p = pre_scale ? pre_scale[row] : 1.f;
    float v[UNITS][8];
    float amax = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      if (live[k]) {
        load_bf16x8(x + base + col0[k], v[k]);
      } else {
#pragma unroll
        for (int j = 0; j < 8; ++j) v[k][j] = 0.f;
      }
#pragma unroll
      for (int j = 0; j < 8; ++j) {
        v[k][j] *= p;
        amax = fmaxf(amax, fabsf(v[k][j]));
      }
    }
    amax = team_reduce_max<TEAM>(amax);

    // amax = 1.f * 2^(E-127) = m * 2^(E-126), m = 1.f / 2 <= 0.875 <=> the
    // fraction is <= .75
    const unsigned bits = __float_as_uint(amax);
    int k2 = (int)(bits >> 23) - 126 - 9 + ((bits & 0x7fffffu) > 0x600000u);
    k2 = k2 < kMinExp ? kMinExp : k2;
    if (amax == 0.f) k2 = 0;
    const float inv = __uint_as_float((unsigned)(127 - k2) << 23);

#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      float z[8];
#pragma unroll
      for (int j = 0; j < 8; ++j)
        z[j] = fminf(fmaxf(v[k][j] * inv, -448.f), 448.f);
      int w0 = __builtin_amdgcn_cvt_pk_fp8_f32(z[0], z[1], 0, false);
      w0 = __builtin_amdgcn_cvt_pk_fp8_f32(z[2], z[3], w0, true);
      int w1 = __builtin_amdgcn_cvt_pk_fp8_f32(z[4], z[5], 0, false);
      w1 = __builtin_amdgcn_cvt_pk_fp8_f32(z[6], z[7], w1, true);
      if (live[k])
        *reinterpret_cast<uint2*>(q + base + col0[k]) =
            make_uint2((unsigned)w0, (unsigned)w1);
    }
    if (rt.lane == 0) s[row] = __uint_as_float((unsigned)(k2 + 127) << 23);
  }
}

// ---- spmm -----------------------------------------------------------------
__device__ __forceinline__ void acc_add_fp8(float* acc, const uint4& r,
                                            float w) {
  float v[16];
  unpack_fp8(v, r);
#pragma unroll
  for (int j = 0; j < 16; ++j) acc[j] += w * v[j];  // the product is exact
}

// One fp8 rung: N indices, then N payload gathers and N scale loads issued
// back to back into statically indexed slots, and only then the first use.
template <int N, typename LD>
__device__ __forceinline__ void fp8_group(
    float* __restrict__ acc, const LD& ld, const int* __restrict__ colidx,
    const float* __restrict__ scale, int64_t e) {
  int u[N];
  uint4 r[N];
  float w[N];
#pragma unroll
  for (int i = 0; i < N; ++i) u[i] = colidx[e + i];
#pragma unroll
  for (int i = 0; i < N; ++i) r[i] = ld.load(u[i]);
#pragma unroll
  for (int i = 0; i < N; ++i) w[i] = scale[u[i]];
#pragma unroll
  for (int i = 0; i < N; ++i) acc_add_fp8(acc, r[i], w[i]);
}

// spmm_kernel's arguments and variants (spmm.hip), for q / scale in place of
// x / weight and whole rows only. OT is bf16 or fp32 (strip partials, or the
// fp32 result of a one-pass launch).
template <typename OT, int TEAM, int UN, bool BUF, bool HEAVY = false,
          bool FINAL = false, bool PERM = false>
__global__ __launch_bounds__(kBlock) void spmm_fp8_kernel(
    OT* __restrict__ out, const fp8_t* __restrict__ q,
    const float* __restrict__ scale, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, const float* __restrict__ deg_dst,
    const int* __restrict__ row_order, int num_rows, int64_t ld,
    bool accumulate, unsigned q_bytes, const int* __restrict__ heavy_rows,
    int num_heavy, int heavy_min, unsigned short* __restrict__ final_out,
    const int* __restrict__ out_rows, int n_out) {
  constexpr int EPU = EltTraits<fp8_t>::kPerVec;
  const RowTeam<TEAM> rt;
  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  if (col0 >= ld) return;  // ld % EPU == 0: a unit is whole or absent

  const auto g = make_gather<fp8_t, BUF>(q, q_bytes, ld, col0);
  // dst: the row of the finished result (== row without PERM)
  auto do_row = [&](int row, int dst, int64_t e0, int64_t e1) {
    float acc[EPU];
    OT* o = out + (int64_t)(FINAL ? row : dst) * ld + col0;
    if (accumulate) {
#pragma unroll
      for (int j = 0; j < EPU; ++j) acc[j] = elt_to_f32(o[j]);
    } else {
#pragma unroll
      for (int j = 0; j < EPU; ++j) acc[j] = 0.f;
    }
    int64_t e = e0;
    ROC_EDGE_LADDER(UN, e, e1,
                    fp8_group<ROC_LADDER_N>(acc, g, colidx, scale, e));
    if (deg_dst) {
      const float s = deg_dst[dst];
#pragma unroll
      for (int j = 0; j < EPU; ++j) acc[j] *= s;
    }
    if constexpr (FINAL) store_vec(final_out + (int64_t)dst * ld + col0, acc);
    else store_vec(o, acc);
  };
  if constexpr (HEAVY) {
    // the heavy list a wave at a time, then the natural sweep past its rows
    constexpr int TPW = 64 / TEAM;
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
      do_row(row, row, e0, e1);
    }
  } else if constexpr (PERM) {
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int dst = out_rows[ri];
      if ((unsigned)dst >= (unsigned)n_out) continue;  // bad entry
      do_row(ri, dst, rowptr[ri], rowptr[ri + 1]);
    }
  } else {
    for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
      const int row = row_order ? row_order[ri] : ri;
      do_row(row, row, rowptr[row], rowptr[row + 1]);
    }
  }
}

struct Fp8Pass {
  const int* heavy_rows = nullptr;
  int num_heavy = 0;
  int heavy_min = 0;
  unsigned short* final_out = nullptr;
  const int* out_rows = nullptr;
  int n_out = 0;
};

template <typename OT, bool HEAVY, bool FINAL, bool PERM>
void launch_spmm_fp8(OT* out, const fp8_t* q, const float* scale,
                     const int64_t* rowptr, const int* colidx,
                     const float* deg_dst,
                     const c10::optional<torch::Tensor>& row_order,
                     int num_rows, int64_t D, bool accumulate, size_t q_elems,
                     hipStream_t stream, const Fp8Pass& sp) {
  constexpr int EPU = EltTraits<fp8_t>::kPerVec;
  const GatherGeom g = gather_geom<fp8_t>(num_rows, D / EPU, 0, q_elems);
  const int* order = row_order_ptr(row_order, num_rows, g.team, "spmm_fp8");
  dispatch_gather(g, [&](auto team_c, auto buf_c) {
    hipLaunchKernelGGL(
        (spmm_fp8_kernel<OT, decltype(team_c)::value, 16,
                         decltype(buf_c)::value, HEAVY, FINAL, PERM>),
        g.grid, dim3(kBlock), 0, stream, out, q, scale, rowptr, colidx,
        deg_dst, order, num_rows, D, accumulate, g.bytes, sp.heavy_rows,
        sp.num_heavy, sp.heavy_min, sp.final_out, sp.out_rows, sp.n_out);
  });
}

void check_scale(const torch::Tensor& s, int64_t n, const char* what) {
  TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                  s.scalar_type() == torch::kFloat32 && s.numel() == n,
              what, " must be a contiguous fp32 GPU tensor, one entry per row");
}

void check_fp8_mat(const torch::Tensor& q, const char* what) {
  check_mat(q, what, "q");
  TORCH_CHECK(q.scalar_type() == torch::kUInt8, what,
              ": q must be uint8 (e4m3 bytes)");
  TORCH_CHECK(q.size(1) % 16 == 0, what,
              ": the feature dim must be a multiple of 16");
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void quantize_rows_fp8(torch::Tensor q, torch::Tensor s, torch::Tensor x,
                       c10::optional<torch::Tensor> pre_scale) {
  check_fp8_mat(q, "quantize_rows_fp8");
  check_mat(x, "quantize_rows_fp8", "x");
  TORCH_CHECK(x.scalar_type() == torch::kBFloat16,
              "quantize_rows_fp8: x must be bf16");
  TORCH_CHECK(q.sizes() == x.sizes(),
              "quantize_rows_fp8: q and x differ in shape");
  const int num_rows = (int)x.size(0);
  const int64_t D = x.size(1);
  TORCH_CHECK(D >= 16 && D <= kMaxD,
              "quantize_rows_fp8: D must be in [16, ", kMaxD, "]");
  check_scale(s, num_rows, "quantize_rows_fp8: s");
  if (pre_scale.has_value())
    check_scale(*pre_scale, num_rows, "quantize_rows_fp8: pre_scale");
  if (num_rows == 0) return;
  const int team = row_team_size(D / 8);
  const dim3 grid(roc_grid_1d(num_rows, kBlock / team, kQuantGridCap));
  auto stream = roc_stream();
  auto launch = [&](auto team_c, auto units_c) {
    hipLaunchKernelGGL(
        (quantize_rows_fp8_kernel<decltype(team_c)::value,
                                  decltype(units_c)::value>),
        grid, dim3(kBlock), 0, stream, (fp8_t*)q.data_ptr(),
        s.data_ptr<float>(), (const unsigned short*)x.data_ptr(),
        pre_scale.has_value() ? pre_scale->data_ptr<float>() : nullptr,
        num_rows, (int)D);
  };
  if (D > 64 * 8)  // two units per lane, team 64 only
    launch(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
  else
    dispatch_team(team, [&](auto team_c) {
      launch(team_c, std::integral_constant<int, 1>{});
    });
  ROC_HIP_CHECK(hipGetLastError());
}

// The arguments after `scale` are spmm's (spmm.hip), less deg_src (fold it
// into the quantiser's pre_scale) and the column window.
void spmm_fp8(torch::Tensor out, torch::Tensor q, torch::Tensor scale,
              torch::Tensor rowptr, torch::Tensor colidx,
              c10::optional<torch::Tensor> deg_dst,
              c10::optional<torch::Tensor> row_order, bool accumulate,
              c10::optional<torch::Tensor> heavy_rows, int64_t heavy_min,
              c10::optional<torch::Tensor> final_out,
              c10::optional<torch::Tensor> out_rows) {
  check_fp8_mat(q, "spmm_fp8");
  check_mat(out, "spmm_fp8", "out");
  TORCH_CHECK(out.size(1) == q.size(1),
              "spmm_fp8: out and q differ in feature dim");
  check_scale(scale, q.size(0), "spmm_fp8: scale");
  const bool f32 = out.scalar_type() == torch::kFloat32;
  TORCH_CHECK(f32 || out.scalar_type() == torch::kBFloat16,
              "spmm_fp8: out must be bf16 or fp32");
  TORCH_CHECK(f32 || !accumulate, "spmm_fp8: accumulate needs an fp32 out");
  Fp8Pass sp;
  if (heavy_rows.has_value()) {
    ROC_CHECK_DEV_CONT(*heavy_rows);
    TORCH_CHECK(f32 && heavy_rows->scalar_type() == torch::kInt32 &&
                    !row_order.has_value() && !out_rows.has_value() &&
                    heavy_min >= 0 && heavy_min <= INT_MAX,
                "spmm_fp8: heavy_rows is an int32 list of an fp32 strip "
                "pass; it excludes row_order and out_rows");
    sp.heavy_rows = heavy_rows->data_ptr<int>();
    sp.num_heavy = (int)heavy_rows->numel();
    sp.heavy_min = (int)heavy_min;
  }
  if (final_out.has_value()) {
    ROC_CHECK_DEV_CONT(*final_out);
    TORCH_CHECK(f32 && final_out->scalar_type() == torch::kBFloat16,
                "spmm_fp8: final_out is the bf16 result of an fp32 pass");
    TORCH_CHECK(out_rows.has_value()
                    ? final_out->dim() == 2 &&
                          final_out->size(1) == out.size(1) &&
                          final_out->size(0) < INT_MAX
                    : final_out->sizes() == out.sizes(),
                "spmm_fp8: final_out shape mismatch");
    sp.final_out = (unsigned short*)final_out->data_ptr();
  }
  const int num_rows =
      out_rows.has_value() ? (int)out_rows->numel() : (int)out.size(0);
  const int64_t D = out.size(1);
  check_csr(rowptr, colidx, num_rows, "spmm_fp8");
  if (out_rows.has_value()) {
    ROC_CHECK_DEV_CONT(*out_rows);
    TORCH_CHECK(out_rows->scalar_type() == torch::kInt32 &&
                    !row_order.has_value() &&
                    (final_out.has_value() || !f32),
                "spmm_fp8: out_rows is an int32 option of the bf16 plain "
                "pass and of the final strip pass; it excludes row_order");
    TORCH_CHECK(!final_out.has_value() || out.size(0) == num_rows,
                "spmm_fp8: out_rows must have one entry per row of the "
                "partials");
    sp.out_rows = out_rows->data_ptr<int>();
    sp.n_out = (int)(final_out.has_value() ? final_out->size(0) : out.size(0));
  }
  if (deg_dst.has_value())
    check_scale(*deg_dst, out_rows.has_value() ? sp.n_out : num_rows,
                "spmm_fp8: deg_dst");
  if (num_rows == 0) return;
  const float* dd = deg_dst.has_value() ? deg_dst->data_ptr<float>() : nullptr;
  auto stream = roc_stream();
  auto launch = [&](auto ot, auto heavy_c, auto final_c, auto perm_c) {
    using OT = typename decltype(ot)::type;
    launch_spmm_fp8<OT, decltype(heavy_c)::value, decltype(final_c)::value,
                    decltype(perm_c)::value>(
        (OT*)out.data_ptr(), (const fp8_t*)q.data_ptr(),
        scale.data_ptr<float>(), rowptr.data_ptr<int64_t>(),
        colidx.data_ptr<int>(), dd, row_order, num_rows, D, accumulate,
        (size_t)q.numel(), stream, sp);
  };
  const std::false_type no{};
  const std::true_type yes{};
  if (!f32) {
    if (sp.out_rows) launch(EltTag<unsigned short>{}, no, no, yes);
    else launch(EltTag<unsigned short>{}, no, no, no);
  } else if (sp.out_rows) {  // checked above: a final pass, no list
    launch(EltTag<float>{}, no, yes, yes);
  } else {
    dispatch_bool(sp.heavy_rows != nullptr, [&](auto heavy_c) {
      dispatch_bool(sp.final_out != nullptr, [&](auto final_c) {
        launch(EltTag<float>{}, heavy_c, final_c, no);
      });
    });
  }
  ROC_HIP_CHECK(hipGetLastError());
}
