// Per-row LayerNorm (+ fused ReLU) for CDNA4, forward and backward.
//
// forward   mean_i = sum_j x[i,j] / D
//           var_i  = sum_j (x[i,j] - mean_i)^2 / D        (centred pass)
//           rstd_i = 1 / sqrt(var_i + eps)
//           y[i,j] = act((x[i,j] - mean_i) * rstd_i * gamma[j] + beta[j])
// backward  xh = (x - mean) * rstd,  g = dy (where xh*gamma+beta > 0 if relu)
//           dx[i,j]   = rstd_i * ((g*gamma - mean_j(g*gamma))
//                                 - xh * mean_j(g*gamma*xh))
//           dgamma[j] = sum_i g*xh,   dbeta[j] = sum_i g
//
// Frame: a RowTeam<TEAM> owns one row at a time and holds the WHOLE row in
// registers, UNITS 16-B units per lane (unit k of a lane covers columns
// (k*TEAM + lane)*EPU ...), so x is read once and y / dx written once.
// TEAM < 64 always has UNITS == 1; UNITS 2 and 4 exist at TEAM == 64 only.
// gamma and beta (fp32 masters) are loaded once per team, before the rows.
//
// Rules the tests pin:
//  - all math is fp32 and every operation rounds on its own (contraction is
//    off below), so the relu mask of the backward is the forward's bit for
//    bit and the kernels agree with a plain fp32 evaluation of the formulas
//  - the variance is the centred second pass, never E[x^2] - mean^2
//  - rstd is 1.0f / sqrtf(.), both correctly rounded; no rsqrt
//  - one rounding to bf16, at the store
//  - lanes and units past D add 0 to every sum and store nothing; the fp32
//    unit that straddles D (D % 4 != 0) loads and stores through guarded
//    scalar accesses on statically indexed registers
//  - dgamma / dbeta use no atomics: per-lane fp32 partials over all the rows
//    a team visits, folded through LDS in team order into one slab row per
//    block, and the slab is folded by a second kernel in a fixed order. The
//    grid depends on (N, D, dtype) only, so the result is bit-reproducible.

#include <climits>

#include "row_team.h"

#pragma clang fp contract(off)

namespace {

constexpr int kMaxD = 1024;
constexpr int kFwdGridCap = 2048;
// the slab is [blocks, 2, D] fp32: 8 MB at most
constexpr int kBwdGridCap = 1024;
// slab fold: kFoldCols columns per block, the blocks of the slab cut into
// kFoldSegs contiguous segments, one thread per (segment, column)
constexpr int kFoldCols = 16;
constexpr int kFoldSegs = kBlock / kFoldCols;

// ---- one unit of a row: full = one 16-B access, straddling = guarded
// scalar accesses, past D = zeros / nothing ---------------------------------
__device__ __forceinline__ void load_unit(float (&v)[4], const float* p,
                                          int nvalid) {
  if (nvalid == 4) {
    load_f32x4(p, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j) v[j] = j < nvalid ? p[j] : 0.f;
  }
}
__device__ __forceinline__ void load_unit(float (&v)[8], const float* p,
                                          int nvalid) {
  if (nvalid == 8) {
    load_f32x4(p, v);
    load_f32x4(p + 4, v + 4);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = j < nvalid ? p[j] : 0.f;
  }
}
// bf16 rows are whole units (D % 8 == 0)
__device__ __forceinline__ void load_unit(float (&v)[8],
                                          const unsigned short* p,
                                          int nvalid) {
  if (nvalid == 8) {
    load_bf16x8(p, v);
  } else {
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = 0.f;
  }
}
__device__ __forceinline__ void store_unit(float* p, const float (&v)[4],
                                           int nvalid) {
  if (nvalid == 4) {
    store_vec(p, v);
  } else {
#pragma unroll
    for (int j = 0; j < 4; ++j)
      if (j < nvalid) p[j] = v[j];
  }
}
__device__ __forceinline__ void store_unit(unsigned short* p,
                                           const float (&v)[8], int nvalid) {
  if (nvalid == 8) store_vec(p, v);
}

// what every kernel keeps per lane for the whole launch
template <typename T, int TEAM, int UNITS>
struct LaneCols {
  static constexpr int EPU = EltTraits<T>::kPerVec;
  int col0[UNITS];
  int nvalid[UNITS];  // 0 .. EPU columns of unit k inside D
  float gamma[UNITS][EPU];
  float beta[UNITS][EPU];
  __device__ __forceinline__ LaneCols(int lane, int D,
                                      const float* __restrict__ g,
                                      const float* __restrict__ b) {
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      col0[k] = (k * TEAM + lane) * EPU;
      const int left = D - col0[k];
      nvalid[k] = left >= EPU ? EPU : (left > 0 ? left : 0);
      load_unit(gamma[k], g + col0[k], nvalid[k]);
      load_unit(beta[k], b + col0[k], nvalid[k]);
    }
  }
};

template <typename T, int TEAM, int UNITS, bool STATS>
__global__ __launch_bounds__(kBlock) void layer_norm_fwd_kernel(
    T* __restrict__ y, float* __restrict__ mean, float* __restrict__ rstd,
    const T* __restrict__ x, const float* __restrict__ gamma,
    const float* __restrict__ beta, int num_rows, int D, float eps,
    bool relu) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const RowTeam<TEAM> rt;
  const LaneCols<T, TEAM, UNITS> lc(rt.lane, D, gamma, beta);
  const float fD = (float)D;

  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t base = (int64_t)row * D;
    float v[UNITS][EPU];
#pragma unroll
    for (int k = 0; k < UNITS; ++k)
      load_unit(v[k], x + base + lc.col0[k], lc.nvalid[k]);

    float s = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k)
#pragma unroll
      for (int j = 0; j < EPU; ++j) s += v[k][j];
    const float m = team_reduce_sum<TEAM>(s) / fD;

    float q = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k)
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        const float d = j < lc.nvalid[k] ? v[k][j] - m : 0.f;
        v[k][j] = d;
        q += d * d;
      }
    const float var = team_reduce_sum<TEAM>(q) / fD;
    const float r = 1.0f / sqrtf(var + eps);

#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        const float o = v[k][j] * r * lc.gamma[k][j] + lc.beta[k][j];
        v[k][j] = relu ? fmaxf(o, 0.f) : o;
      }
      store_unit(y + base + lc.col0[k], v[k], lc.nvalid[k]);  // one rounding
    }
    if constexpr (STATS) {
      if (rt.lane == 0) {
        mean[row] = m;
        rstd[row] = r;
      }
    }
  }
}

template <typename T, int TEAM, int UNITS>
__global__ __launch_bounds__(kBlock) void layer_norm_bwd_kernel(
    T* __restrict__ dx, float* __restrict__ slab, const T* __restrict__ dy,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, int num_rows, int D, bool relu) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  constexpr int NT = kBlock / TEAM;       // teams per block
  constexpr int W = TEAM * UNITS * EPU;   // columns a team covers, >= D
  __shared__ __align__(16) float part[NT][2][W];

  const RowTeam<TEAM> rt;
  const LaneCols<T, TEAM, UNITS> lc(rt.lane, D, gamma, beta);
  const float fD = (float)D;

  float dg[UNITS][EPU], db[UNITS][EPU];
#pragma unroll
  for (int k = 0; k < UNITS; ++k)
#pragma unroll
    for (int j = 0; j < EPU; ++j) dg[k][j] = db[k][j] = 0.f;

  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t base = (int64_t)row * D;
    float xh[UNITS][EPU], a[UNITS][EPU];
#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
      load_unit(xh[k], x + base + lc.col0[k], lc.nvalid[k]);
      load_unit(a[k], dy + base + lc.col0[k], lc.nvalid[k]);
    }
    const float m = mean[row], r = rstd[row];

    // columns past D hold dy = gamma = beta = 0, so g and g*gamma are 0
    // there and they add nothing below, whatever their xh is
    float s1 = 0.f, s2 = 0.f;
#pragma unroll
    for (int k = 0; k < UNITS; ++k)
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        const float h = (xh[k][j] - m) * r;
        float g = a[k][j];
        if (relu) g = h * lc.gamma[k][j] + lc.beta[k][j] > 0.f ? g : 0.f;
        dg[k][j] += g * h;
        db[k][j] += g;
        const float ag = g * lc.gamma[k][j];
        xh[k][j] = h;
        a[k][j] = ag;
        s1 += ag;
        s2 += ag * h;
      }
    const float m1 = team_reduce_sum<TEAM>(s1) / fD;
    const float m2 = team_reduce_sum<TEAM>(s2) / fD;

#pragma unroll
    for (int k = 0; k < UNITS; ++k) {
#pragma unroll
      for (int j = 0; j < EPU; ++j)
        a[k][j] = r * ((a[k][j] - m1) - xh[k][j] * m2);
      store_unit(dx + base + lc.col0[k], a[k], lc.nvalid[k]);  // one rounding
    }
  }

  // the block's teams, in team order, into slab[blockIdx.x] = [2, D]
  const int t = (int)threadIdx.x / TEAM;
#pragma unroll
  for (int k = 0; k < UNITS; ++k)
#pragma unroll
    for (int j = 0; j < EPU; j += 4) {
      store_f32x4(&part[t][0][lc.col0[k] + j], &dg[k][j]);
      store_f32x4(&part[t][1][lc.col0[k] + j], &db[k][j]);
    }
  __syncthreads();
  float* out = slab + (int64_t)blockIdx.x * 2 * D;
  for (int i = threadIdx.x; i < 2 * D; i += kBlock) {
    const int which = i >= D, c = which ? i - D : i;
    float s = 0.f;
#pragma unroll
    for (int u = 0; u < NT; ++u) s += part[u][which][c];
    out[i] = s;
  }
}

// slab [nblocks, 2*D] -> dgamma | dbeta. Column c is summed over each of
// kFoldSegs contiguous segments of blocks in ascending block order, then
// over the segments in ascending order: one fixed order per (nblocks, D).
__global__ __launch_bounds__(kBlock) void layer_norm_fold_kernel(
    float* __restrict__ dgamma, float* __restrict__ dbeta,
    const float* __restrict__ slab, int nblocks, int D) {
  __shared__ float part[kFoldSegs][kFoldCols];
  const int l = (int)threadIdx.x % kFoldCols;
  const int seg = (int)threadIdx.x / kFoldCols;
  const int c = blockIdx.x * kFoldCols + l;
  const int per = (nblocks + kFoldSegs - 1) / kFoldSegs;
  const int b0 = seg * per;
  const int b1 = b0 + per < nblocks ? b0 + per : nblocks;
  float s = 0.f;
  if (c < 2 * D) {
#pragma unroll 8
    for (int b = b0; b < b1; ++b) s += slab[(int64_t)b * 2 * D + c];
  }
  part[seg][l] = s;
  __syncthreads();
  if (seg == 0 && c < 2 * D) {
    float tot = 0.f;
#pragma unroll
    for (int q = 0; q < kFoldSegs; ++q) tot += part[q][l];
    if (c < D) dgamma[c] = tot; else dbeta[c - D] = tot;
  }
}

// geometry: a function of (D, dtype) only
struct LnGeom {
  int team;
  int units;  // 1, 2 or 4 units per lane
};

template <typename T>
LnGeom ln_geom(int64_t D) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const int64_t row_units = (D + EPU - 1) / EPU;
  LnGeom g;
  g.team = row_team_size(row_units);
  const int64_t per_lane = (row_units + g.team - 1) / g.team;
  g.units = per_lane <= 1 ? 1 : (per_lane <= 2 ? 2 : 4);
  return g;
}

// f receives (team, units) as integral constants; units > 1 only at team 64,
// and 4 units of bf16 would be 2048 columns, past kMaxD
template <typename T, typename F>
void dispatch_ln_geom(const LnGeom& g, F&& f) {
  if (g.units == 1) {
    dispatch_team(g.team, [&](auto team_c) {
      f(team_c, std::integral_constant<int, 1>{});
    });
  } else if (g.units == 2) {
    f(std::integral_constant<int, 64>{}, std::integral_constant<int, 2>{});
  } else {
    if constexpr (std::is_same<T, float>::value)
      f(std::integral_constant<int, 64>{}, std::integral_constant<int, 4>{});
    else
      TORCH_CHECK(false, "layer_norm: no bf16 geometry for this width");
  }
}

void check_affine(const torch::Tensor& p, int64_t D, const char* what) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() &&
                  p.scalar_type() == torch::kFloat32 && p.dim() == 1 &&
                  p.size(0) == D,
              what, " must be a contiguous fp32 [D] GPU tensor");
}

void check_rows(const torch::Tensor& a, const torch::Tensor& b,
                const char* op) {
  ROC_CHECK_DEV_CONT(a);
  ROC_CHECK_DEV_CONT(b);
  TORCH_CHECK(a.dim() == 2 && a.sizes() == b.sizes() &&
                  a.scalar_type() == b.scalar_type(),
              op, ": [N, D] tensors of one shape and dtype");
  TORCH_CHECK(a.size(0) < INT_MAX, op, ": too many rows");
  const int64_t D = a.size(1);
  TORCH_CHECK(D >= 1 && D <= kMaxD, op, ": D must be in [1, ", kMaxD, "]");
  TORCH_CHECK(a.scalar_type() != torch::kBFloat16 || D % 8 == 0, op,
              ": bf16 rows must be a multiple of 8 wide");
}

void check_stat(const torch::Tensor& s, int64_t N, const char* what) {
  TORCH_CHECK(s.is_cuda() && s.is_contiguous() &&
                  s.scalar_type() == torch::kFloat32 && s.numel() == N,
              what, " must be a contiguous fp32 [N] GPU tensor");
}

}  // namespace

void layer_norm_fwd(torch::Tensor y, c10::optional<torch::Tensor> mean,
                    c10::optional<torch::Tensor> rstd, torch::Tensor x,
                    torch::Tensor gamma, torch::Tensor beta, double eps,
                    bool relu) {
  check_rows(y, x, "layer_norm_fwd");
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_affine(gamma, D, "layer_norm_fwd: gamma");
  check_affine(beta, D, "layer_norm_fwd: beta");
  TORCH_CHECK(mean.has_value() == rstd.has_value(),
              "layer_norm_fwd: pass both mean and rstd, or neither");
  float* meanp = nullptr;
  float* rstdp = nullptr;
  if (mean.has_value()) {
    check_stat(*mean, num_rows, "layer_norm_fwd: mean");
    check_stat(*rstd, num_rows, "layer_norm_fwd: rstd");
    meanp = mean->data_ptr<float>();
    rstdp = rstd->data_ptr<float>();
  }
  if (num_rows == 0) return;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "layer_norm_fwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const LnGeom g = ln_geom<T>(D);
    const dim3 grid(roc_grid_1d(num_rows, kBlock / g.team, kFwdGridCap));
    dispatch_ln_geom<T>(g, [&](auto team_c, auto units_c) {
      dispatch_bool(meanp != nullptr, [&](auto stats_c) {
        hipLaunchKernelGGL(
            (layer_norm_fwd_kernel<T, decltype(team_c)::value,
                                   decltype(units_c)::value,
                                   decltype(stats_c)::value>),
            grid, dim3(kBlock), 0, stream, (T*)y.data_ptr(), meanp, rstdp,
            (const T*)x.data_ptr(), gamma.data_ptr<float>(),
            beta.data_ptr<float>(), num_rows, D, (float)eps, relu);
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void layer_norm_bwd(torch::Tensor dx, torch::Tensor dgamma,
                    torch::Tensor dbeta, torch::Tensor dy, torch::Tensor x,
                    torch::Tensor mean, torch::Tensor rstd,
                    torch::Tensor gamma, torch::Tensor beta, bool relu) {
  check_rows(dx, x, "layer_norm_bwd");
  check_rows(dy, x, "layer_norm_bwd");
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_affine(gamma, D, "layer_norm_bwd: gamma");
  check_affine(beta, D, "layer_norm_bwd: beta");
  check_affine(dgamma, D, "layer_norm_bwd: dgamma");
  check_affine(dbeta, D, "layer_norm_bwd: dbeta");
  check_stat(mean, num_rows, "layer_norm_bwd: mean");
  check_stat(rstd, num_rows, "layer_norm_bwd: rstd");
  if (num_rows == 0) {
    dgamma.zero_();
    dbeta.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "layer_norm_bwd", [&](auto xt) {
    using T = typename decltype(xt)::type;
    const LnGeom g = ln_geom<T>(D);
    const int nblocks = roc_grid_1d(num_rows, kBlock / g.team, kBwdGridCap);
    // from the torch allocator: capturable, and freed in stream order
    torch::Tensor slab = torch::empty(
        {nblocks, 2, D}, x.options().dtype(torch::kFloat32));
    dispatch_ln_geom<T>(g, [&](auto team_c, auto units_c) {
      hipLaunchKernelGGL(
          (layer_norm_bwd_kernel<T, decltype(team_c)::value,
                                 decltype(units_c)::value>),
          dim3(nblocks), dim3(kBlock), 0, stream, (T*)dx.data_ptr(),
          slab.data_ptr<float>(), (const T*)dy.data_ptr(),
          (const T*)x.data_ptr(), mean.data_ptr<float>(),
          rstd.data_ptr<float>(), gamma.data_ptr<float>(),
          beta.data_ptr<float>(), num_rows, D, relu);
    });
    hipLaunchKernelGGL(layer_norm_fold_kernel,
                       dim3((2 * D + kFoldCols - 1) / kFoldCols),
                       dim3(kBlock), 0, stream, dgamma.data_ptr<float>(),
                       dbeta.data_ptr<float>(), slab.data_ptr<float>(),
                       nblocks, D);
  });
  ROC_HIP_CHECK(hipGetLastError());
}
