// BatchNorm (+ fused ReLU) over the rows of a tall [N, D] for CDNA4: the
// column statistics, the apply pass, and the backward's column sums and dx.
//
// stats     mean_j = sum_i x[i,j] / n,  m2_j = sum_i (x[i,j] - mean_j)^2
// finalize  rstd_j = 1 / sqrt(m2_j / n + eps)           (+ running buffers)
// apply     y[i,j] = act(((x[i,j] - mean_j) * rstd_j) * gamma_j + beta_j)
// backward  xh = (x - mean) * rstd,  g = dy (where xh*gamma+beta > 0 if relu)
//           dgamma_j = sum_i g*xh,   dbeta_j = sum_i g
//           dx[i,j]  = (gamma_j*rstd_j) * ((g - S_g[j]/n) - xh * S_gx[j]/n)
// The statistics of a sharded [N, D] are merged across ranks between stats
// and finalize, and S_g / S_gx between the two backward kernels, by the
// caller (ops/functional.py); n is the global row count then.
//
// Column-reduce frame (stats and bwd_reduce). A block is RG = kBlock / CL
// row-groups of CL contiguous lanes; lane l of every group owns the 16-B
// unit l of the block's column tile (kTileUnits units, blockIdx.y), so one
// row-group reads one row's units coalesced. A block owns a CONTIGUOUS chunk
// of rows; its row-groups take rows chunk0 + rg, + RG, ... and a lane keeps
// fp32 partials for its own EPU columns over all the rows it visits, DEPTH
// rows' loads in flight before the first use. The row-groups then fold
// through LDS in row-group order into slab[blockIdx.x, :, tile columns], and
// a fold kernel reduces the slab over blocks: contiguous segments of blocks in
// ascending order, then the segments ascending. No atomics, and the grid is a
// function of (N, D, dtype) only, so every output is bit-reproducible.
//
// Rules the tests pin:
//  - all math is fp32 over the exact widen, every operation rounds on its own
//    (contraction is off below), one rounding to bf16 at the store; so the
//    relu mask of the backward is the forward's bit for bit
//  - the variance never takes the raw form sum x^2 - (sum x)^2 / n. A block
//    sums d = x - shift and d^2 with shift_j = x[first row of its chunk, j]
//    (one load per lane, shared by all its row-groups, so the in-block fold
//    is a plain ordered sum) and emits (mean_b, M2_b); its row count is known
//    from the geometry. The fold merges blocks pairwise with the parallel
//    update of Chan et al., on means taken relative to block 0's
//  - rstd is 1.0f / sqrtf(.), both correctly rounded; no rsqrt
//  - lanes and units past D add 0 and store nothing; the fp32 unit that
//    straddles D goes through guarded scalar accesses on statically indexed
//    registers (load_unit / store_unit of row_team.h)
//  - no D cap: wide rows are column-tiled over blockIdx.y

#include <climits>

#include "row_team.h"

#pragma clang fp contract(off)

// built without the packed fp32 ALU forms, like spmm_fp8.hip
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kTileUnits = 64;   // 16-B units of one column tile
constexpr int kReduceGridCap = 1024;  // slab [blocks, 2, D] fp32
constexpr int kMinChunkGroups = 4;    // a chunk is >= 4 rows per row-group
constexpr int kRowGridCap = 2048;     // apply / dx: grid-strided rows
constexpr int kFoldCols = 16;
constexpr int kFoldSegs = kBlock / kFoldCols;
// rows in flight per row-group (docs/KERNELS.md has the measurement)
constexpr int kStatsDepth = 4;
constexpr int kReduceDepth = 2;

// a lane's place in the frame: which row-group, which unit of the tile
template <typename T, int CL>
struct ColLane {
  static constexpr int EPU = EltTraits<T>::kPerVec;
  static constexpr int RG = kBlock / CL;
  int lane, rg;
  int col0;    // first column of this lane's unit
  int nvalid;  // 0 .. EPU of them inside D
  __device__ __forceinline__ explicit ColLane(int D)
      : lane((int)threadIdx.x % CL), rg((int)threadIdx.x / CL) {
    col0 = ((int)blockIdx.y * kTileUnits + lane) * EPU;
    const int left = D - col0;
    nvalid = left >= EPU ? EPU : (left > 0 ? left : 0);
  }
};

// the block's row-groups, in row-group order, for column `c` of the tile
template <int RG, int W>
__device__ __forceinline__ float fold_groups(const float (&part)[RG][2][W],
                                             int which, int c) {
  float s = 0.f;
#pragma unroll
  for (int u = 0; u < RG; ++u) s += part[u][which][c];
  return s;
}

template <typename T, int CL, int DEPTH>
__global__ __launch_bounds__(kBlock) void batch_norm_stats_kernel(
    float* __restrict__ slab, const T* __restrict__ x, int num_rows, int D,
    int chunk) {
  using CLn = ColLane<T, CL>;
  constexpr int EPU = CLn::EPU, RG = CLn::RG, W = CL * EPU;
  __shared__ __align__(16) float part[RG][2][W];
  __shared__ __align__(16) float shift_s[W];

  const CLn cl(D);
  const int r0 = (int)blockIdx.x * chunk;
  const int r1 = num_rows - r0 < chunk ? num_rows : r0 + chunk;

  float sh[EPU], s1[EPU], s2[EPU];
  load_unit(sh, x + (int64_t)r0 * D + cl.col0, cl.nvalid);
#pragma unroll
  for (int j = 0; j < EPU; ++j) s1[j] = s2[j] = 0.f;

  for (int row = r0 + cl.rg; row < r1; row += RG * DEPTH) {
    float v[DEPTH][EPU];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      // row - r1 < 0 here, so the sum below cannot wrap
      const bool in = d * RG < r1 - row;
      load_unit(v[d], x + (int64_t)(in ? row + d * RG : row) * D + cl.col0,
                in ? cl.nvalid : 0);
    }
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      if (d * RG < r1 - row) {
#pragma unroll
        for (int j = 0; j < EPU; ++j) {
          const float dv = v[d][j] - sh[j];
          s1[j] += dv;
          s2[j] += dv * dv;
        }
      }
    }
  }

#pragma unroll
  for (int j = 0; j < EPU; j += 4) {
    store_f32x4(&part[cl.rg][0][cl.lane * EPU + j], &s1[j]);
    store_f32x4(&part[cl.rg][1][cl.lane * EPU + j], &s2[j]);
    if (cl.rg == 0) store_f32x4(&shift_s[cl.lane * EPU + j], &sh[j]);
  }
  __syncthreads();
  const float nb = (float)(r1 - r0);
  float* out = slab + (int64_t)blockIdx.x * 2 * D;
  const int tile0 = (int)blockIdx.y * kTileUnits * EPU;
  for (int c = threadIdx.x; c < W && tile0 + c < D; c += kBlock) {
    const float a = fold_groups<RG, W>(part, 0, c);
    const float q = fold_groups<RG, W>(part, 1, c);
    const float ma = a / nb;  // mean of the shifted values
    out[tile0 + c] = shift_s[c] + ma;
    // M2 = q - a^2 / nb cancels up to the shift's distance from the mean,
    // so the epilogue adds no rounding of its own to it: a^2 / nb is
    // p + pe + a * (rem / nb) with the product's and the division's
    // remainders taken exactly by fma
    const float p = a * ma;
    const float pe = fmaf(a, ma, -p);
    const float rem = fmaf(-ma, nb, a);
    out[D + tile0 + c] = fmaxf(((q - p) - pe) - a * (rem / nb), 0.f);
  }
}

template <typename T, int CL, int DEPTH>
__global__ __launch_bounds__(kBlock) void batch_norm_bwd_reduce_kernel(
    float* __restrict__ slab, const T* __restrict__ dy,
    const T* __restrict__ x, const float* __restrict__ mean,
    const float* __restrict__ rstd, const float* __restrict__ gamma,
    const float* __restrict__ beta, int num_rows, int D, int chunk,
    bool relu) {
  using CLn = ColLane<T, CL>;
  constexpr int EPU = CLn::EPU, RG = CLn::RG, W = CL * EPU;
  __shared__ __align__(16) float part[RG][2][W];

  const CLn cl(D);
  const int r0 = (int)blockIdx.x * chunk;
  const int r1 = num_rows - r0 < chunk ? num_rows : r0 + chunk;

  float m[EPU], r[EPU], gam[EPU], bet[EPU], dg[EPU], db[EPU];
  load_unit(m, mean + cl.col0, cl.nvalid);
  load_unit(r, rstd + cl.col0, cl.nvalid);
  load_unit(gam, gamma + cl.col0, cl.nvalid);
  load_unit(bet, beta + cl.col0, cl.nvalid);
#pragma unroll
  for (int j = 0; j < EPU; ++j) dg[j] = db[j] = 0.f;

  for (int row = r0 + cl.rg; row < r1; row += RG * DEPTH) {
    float v[DEPTH][EPU], a[DEPTH][EPU];
#pragma unroll
    for (int d = 0; d < DEPTH; ++d) {
      const bool in = d * RG < r1 - row;
      const int64_t base = (int64_t)(in ? row + d * RG : row) * D + cl.col0;
      load_unit(v[d], x + base, in ? cl.nvalid : 0);
      load_unit(a[d], dy + base, in ? cl.nvalid : 0);
    }
    // rows past the chunk and columns past D hold dy = 0, so g = 0 there
    // and they add nothing, whatever their xh is
#pragma unroll
    for (int d = 0; d < DEPTH; ++d)
#pragma unroll
      for (int j = 0; j < EPU; ++j) {
        const float h = (v[d][j] - m[j]) * r[j];
        float g = a[d][j];
        if (relu) g = h * gam[j] + bet[j] > 0.f ? g : 0.f;
        dg[j] += g * h;
        db[j] += g;
      }
  }

#pragma unroll
  for (int j = 0; j < EPU; j += 4) {
    store_f32x4(&part[cl.rg][0][cl.lane * EPU + j], &dg[j]);
    store_f32x4(&part[cl.rg][1][cl.lane * EPU + j], &db[j]);
  }
  __syncthreads();
  float* out = slab + (int64_t)blockIdx.x * 2 * D;
  const int tile0 = (int)blockIdx.y * kTileUnits * EPU;
  for (int c = threadIdx.x; c < W && tile0 + c < D; c += kBlock) {
    out[tile0 + c] = fold_groups<RG, W>(part, 0, c);
    out[D + tile0 + c] = fold_groups<RG, W>(part, 1, c);
  }
}

// (n, d, m2) <- (n, d, m2) merged with (nb, db, mb): Chan et al.
__device__ __forceinline__ void chan_merge(int& n, float& d, float& m2,
                                           int nb, float db, float mb) {
  if (nb == 0) return;
  const int nn = n + nb;
  const float delta = db - d;
  const float wb = (float)nb / (float)nn;
  d = d + delta * wb;
  m2 = (m2 + mb) + (delta * delta) * ((float)n * wb);
  n = nn;
}

// slab [nblocks, 2, D] -> out0[D], out1[D]. Column c is reduced over each of
// kFoldSegs contiguous segments of blocks in ascending block order, then
// over the segments in ascending order: one fixed order per (nblocks, D).
// CHAN: the slab rows are (mean_b, M2_b) of `chunk` rows each (the last
// block has the rest of num_rows) and merge to (mean, m2); means are carried
// relative to block 0's, so the merge rounds at the size of their spread.
// Otherwise both halves are plain sums.
template <bool CHAN>
__global__ __launch_bounds__(kBlock) void batch_norm_fold_kernel(
    float* __restrict__ out0, float* __restrict__ out1,
    const float* __restrict__ slab, int nblocks, int D, int num_rows,
    int chunk) {
  __shared__ float part[kFoldSegs][2][kFoldCols];
  __shared__ int cnt[kFoldSegs];
  const int l = (int)threadIdx.x % kFoldCols;
  const int seg = (int)threadIdx.x / kFoldCols;
  const int c = blockIdx.x * kFoldCols + l;
  const int per = (nblocks + kFoldSegs - 1) / kFoldSegs;
  const int b0 = seg * per < nblocks ? seg * per : nblocks;
  const int b1 = b0 + per < nblocks ? b0 + per : nblocks;
  const float ref = CHAN && c < D ? slab[c] : 0.f;
  int n = 0;
  float s0 = 0.f, s1 = 0.f;
  if (c < D) {
    for (int b = b0; b < b1; ++b) {
      const float v0 = slab[(int64_t)b * 2 * D + c];
      const float v1 = slab[(int64_t)b * 2 * D + D + c];
      if constexpr (CHAN) {
        const int nb = b == nblocks - 1 ? num_rows - b * chunk : chunk;
        chan_merge(n, s0, s1, nb, v0 - ref, v1);
      } else {
        s0 += v0;
        s1 += v1;
      }
    }
  }
  part[seg][0][l] = s0;
  part[seg][1][l] = s1;
  if (l == 0) cnt[seg] = n;  // column blockIdx.x * kFoldCols is inside D
  __syncthreads();
  if (seg == 0 && c < D) {
    int tn = 0;
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int q = 0; q < kFoldSegs; ++q) {
      if constexpr (CHAN) {
        chan_merge(tn, t0, t1, cnt[q], part[q][0][l], part[q][1][l]);
      } else {
        t0 += part[q][0][l];
        t1 += part[q][1][l];
      }
    }
    out0[c] = CHAN ? ref + t0 : t0;
    out1[c] = t1;
  }
}

__global__ __launch_bounds__(kBlock) void batch_norm_finalize_kernel(
    float* __restrict__ rstd, float* __restrict__ running_mean,
    float* __restrict__ running_var, const float* __restrict__ mean,
    const float* __restrict__ m2, int D, float n, float momentum, float eps) {
  const int c = blockIdx.x * kBlock + threadIdx.x;
  if (c >= D) return;
  const float q = m2[c];
  rstd[c] = 1.0f / sqrtf(q / n + eps);
  if (running_mean != nullptr) {
    const float keep = 1.0f - momentum;
    running_mean[c] = keep * running_mean[c] + momentum * mean[c];
    if (n > 1.0f)  // unbiased; one row has no sample variance
      running_var[c] = keep * running_var[c] + momentum * (q / (n - 1.0f));
  }
}

// apply and dx: the same lanes-by-row-groups block, rows grid-strided
template <typename T, int CL>
__global__ __launch_bounds__(kBlock) void batch_norm_apply_kernel(
    T* __restrict__ y, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    int num_rows, int D, bool relu) {
  using CLn = ColLane<T, CL>;
  constexpr int EPU = CLn::EPU, RG = CLn::RG;
  const CLn cl(D);
  if (cl.nvalid == 0) return;
  float m[EPU], r[EPU], gam[EPU], bet[EPU];
  load_unit(m, mean + cl.col0, cl.nvalid);
  load_unit(r, rstd + cl.col0, cl.nvalid);
  load_unit(gam, gamma + cl.col0, cl.nvalid);
  load_unit(bet, beta + cl.col0, cl.nvalid);
  const int stride = (int)gridDim.x * RG;
  for (int64_t row = (int)blockIdx.x * RG + cl.rg; row < num_rows;
       row += stride) {
    float v[EPU];
    load_unit(v, x + row * D + cl.col0, cl.nvalid);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float o = ((v[j] - m[j]) * r[j]) * gam[j] + bet[j];
      v[j] = relu ? fmaxf(o, 0.f) : o;
    }
    store_unit(y + row * D + cl.col0, v, cl.nvalid);  // one rounding
  }
}

template <typename T, int CL>
__global__ __launch_bounds__(kBlock) void batch_norm_bwd_dx_kernel(
    T* __restrict__ dx, const T* __restrict__ dy, const T* __restrict__ x,
    const float* __restrict__ mean, const float* __restrict__ rstd,
    const float* __restrict__ gamma, const float* __restrict__ beta,
    const float* __restrict__ s_g, const float* __restrict__ s_gx,
    int num_rows, int D, float n, bool relu) {
  using CLn = ColLane<T, CL>;
  constexpr int EPU = CLn::EPU, RG = CLn::RG;
  const CLn cl(D);
  if (cl.nvalid == 0) return;
  float m[EPU], r[EPU], gam[EPU], bet[EPU], mg[EPU], mgx[EPU], k[EPU];
  load_unit(m, mean + cl.col0, cl.nvalid);
  load_unit(r, rstd + cl.col0, cl.nvalid);
  load_unit(gam, gamma + cl.col0, cl.nvalid);
  load_unit(bet, beta + cl.col0, cl.nvalid);
  load_unit(mg, s_g + cl.col0, cl.nvalid);
  load_unit(mgx, s_gx + cl.col0, cl.nvalid);
#pragma unroll
  for (int j = 0; j < EPU; ++j) {
    mg[j] = mg[j] / n;
    mgx[j] = mgx[j] / n;
    k[j] = gam[j] * r[j];
  }
  const int stride = (int)gridDim.x * RG;
  for (int64_t row = (int)blockIdx.x * RG + cl.rg; row < num_rows;
       row += stride) {
    float v[EPU], a[EPU];
    load_unit(v, x + row * D + cl.col0, cl.nvalid);
    load_unit(a, dy + row * D + cl.col0, cl.nvalid);
#pragma unroll
    for (int j = 0; j < EPU; ++j) {
      const float h = (v[j] - m[j]) * r[j];
      float g = a[j];
      if (relu) g = h * gam[j] + bet[j] > 0.f ? g : 0.f;
      a[j] = k[j] * ((g - mg[j]) - h * mgx[j]);
    }
    store_unit(dx + row * D + cl.col0, a, cl.nvalid);  // one rounding
  }
}

// geometry: a function of (N, D, dtype) only
struct BnGeom {
  int cl;      // column lanes
  int tiles;   // column tiles (gridDim.y)
  int chunk;   // rows of one reduce block
  int blocks;  // reduce blocks (gridDim.x); every one has rows
};

template <typename T>
BnGeom bn_geom(int64_t num_rows, int64_t D) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  const int64_t units = (D + EPU - 1) / EPU;
  BnGeom g;
  g.tiles = (int)((units + kTileUnits - 1) / kTileUnits);
  g.cl = row_team_size(g.tiles > 1 ? kTileUnits : units);
  const int min_chunk = kMinChunkGroups * (kBlock / g.cl);
  const int want = roc_grid_1d(num_rows, min_chunk, kReduceGridCap);
  g.chunk = (int)((num_rows + want - 1) / want);
  g.blocks = (int)((num_rows + g.chunk - 1) / g.chunk);
  return g;
}

template <typename F>
void dispatch_depth(int64_t depth, int dflt, const char* op, F&& f) {
  switch (depth ? depth : dflt) {
    case 2: f(std::integral_constant<int, 2>{}); break;
    case 4: f(std::integral_constant<int, 4>{}); break;
    case 8: f(std::integral_constant<int, 8>{}); break;
    default: TORCH_CHECK(false, op, ": depth must be 0 (default), 2, 4 or 8");
  }
}

void check_cols(const torch::Tensor& p, int64_t D, const char* op,
                const char* what) {
  TORCH_CHECK(p.is_cuda() && p.is_contiguous() &&
                  p.scalar_type() == torch::kFloat32 && p.dim() == 1 &&
                  p.size(0) == D,
              op, ": ", what, " must be a contiguous fp32 [D] GPU tensor");
}

void check_rows(const torch::Tensor& x, const char* op) {
  ROC_CHECK_DEV_CONT(x);
  TORCH_CHECK(x.dim() == 2 && x.size(1) >= 1, op, ": x must be [N, D >= 1]");
  // gridDim.y and the int column arithmetic: far past any feature width
  TORCH_CHECK(x.size(0) < INT_MAX && x.size(1) <= (1 << 22), op,
              ": too many rows or columns");
  TORCH_CHECK(x.scalar_type() != torch::kBFloat16 || x.size(1) % 8 == 0, op,
              ": bf16 rows must be a multiple of 8 wide");
}

void check_same(const torch::Tensor& a, const torch::Tensor& x,
                const char* op) {
  ROC_CHECK_DEV_CONT(a);
  TORCH_CHECK(a.sizes() == x.sizes() && a.scalar_type() == x.scalar_type(),
              op, ": [N, D] tensors of one shape and dtype");
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void batch_norm_stats(torch::Tensor mean, torch::Tensor m2, torch::Tensor x,
                      int64_t depth) {
  const char* op = "batch_norm_stats";
  check_rows(x, op);
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_cols(mean, D, op, "mean");
  check_cols(m2, D, op, "m2");
  if (num_rows == 0) {
    mean.zero_();
    m2.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), op, [&](auto xt) {
    using T = typename decltype(xt)::type;
    const BnGeom g = bn_geom<T>(num_rows, D);
    // from the torch allocator: capturable, and freed in stream order
    torch::Tensor slab =
        torch::empty({g.blocks, 2, D}, x.options().dtype(torch::kFloat32));
    dispatch_team(g.cl, [&](auto cl_c) {
      dispatch_depth(depth, kStatsDepth, op, [&](auto depth_c) {
        hipLaunchKernelGGL(
            (batch_norm_stats_kernel<T, decltype(cl_c)::value,
                                     decltype(depth_c)::value>),
            dim3(g.blocks, g.tiles), dim3(kBlock), 0, stream,
            slab.data_ptr<float>(), (const T*)x.data_ptr(), num_rows, D,
            g.chunk);
      });
    });
    hipLaunchKernelGGL(batch_norm_fold_kernel<true>,
                       dim3((D + kFoldCols - 1) / kFoldCols), dim3(kBlock), 0,
                       stream, mean.data_ptr<float>(), m2.data_ptr<float>(),
                       slab.data_ptr<float>(), g.blocks, D, num_rows, g.chunk);
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void batch_norm_finalize(torch::Tensor rstd, torch::Tensor mean,
                         torch::Tensor m2,
                         c10::optional<torch::Tensor> running_mean,
                         c10::optional<torch::Tensor> running_var, double n,
                         double momentum, double eps) {
  const char* op = "batch_norm_finalize";
  TORCH_CHECK(rstd.dim() == 1 && rstd.size(0) >= 1, op, ": rstd must be [D]");
  const int64_t D = rstd.size(0);
  check_cols(rstd, D, op, "rstd");
  check_cols(mean, D, op, "mean");
  check_cols(m2, D, op, "m2");
  TORCH_CHECK(running_mean.has_value() == running_var.has_value(), op,
              ": pass both running buffers, or neither");
  TORCH_CHECK(n >= 1.0, op, ": n must be the global row count, >= 1");
  float* rm = nullptr;
  float* rv = nullptr;
  if (running_mean.has_value()) {
    check_cols(*running_mean, D, op, "running_mean");
    check_cols(*running_var, D, op, "running_var");
    rm = running_mean->data_ptr<float>();
    rv = running_var->data_ptr<float>();
  }
  hipLaunchKernelGGL(batch_norm_finalize_kernel,
                     dim3((unsigned)((D + kBlock - 1) / kBlock)), dim3(kBlock),
                     0, roc_stream(), rstd.data_ptr<float>(), rm, rv,
                     mean.data_ptr<float>(), m2.data_ptr<float>(), (int)D,
                     (float)n, (float)momentum, (float)eps);
  ROC_HIP_CHECK(hipGetLastError());
}

void batch_norm_apply(torch::Tensor y, torch::Tensor x, torch::Tensor mean,
                      torch::Tensor rstd, torch::Tensor gamma,
                      torch::Tensor beta, bool relu) {
  const char* op = "batch_norm_apply";
  check_rows(x, op);
  check_same(y, x, op);
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_cols(mean, D, op, "mean");
  check_cols(rstd, D, op, "rstd");
  check_cols(gamma, D, op, "gamma");
  check_cols(beta, D, op, "beta");
  if (num_rows == 0) return;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), op, [&](auto xt) {
    using T = typename decltype(xt)::type;
    const BnGeom g = bn_geom<T>(num_rows, D);
    const dim3 grid(roc_grid_1d(num_rows, kBlock / g.cl, kRowGridCap),
                    g.tiles);
    dispatch_team(g.cl, [&](auto cl_c) {
      hipLaunchKernelGGL(
          (batch_norm_apply_kernel<T, decltype(cl_c)::value>), grid,
          dim3(kBlock), 0, stream, (T*)y.data_ptr(), (const T*)x.data_ptr(),
          mean.data_ptr<float>(), rstd.data_ptr<float>(),
          gamma.data_ptr<float>(), beta.data_ptr<float>(), num_rows, D, relu);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void batch_norm_bwd_reduce(torch::Tensor dgamma, torch::Tensor dbeta,
                           torch::Tensor dy, torch::Tensor x,
                           torch::Tensor mean, torch::Tensor rstd,
                           torch::Tensor gamma, torch::Tensor beta, bool relu,
                           int64_t depth) {
  const char* op = "batch_norm_bwd_reduce";
  check_rows(x, op);
  check_same(dy, x, op);
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_cols(dgamma, D, op, "dgamma");
  check_cols(dbeta, D, op, "dbeta");
  check_cols(mean, D, op, "mean");
  check_cols(rstd, D, op, "rstd");
  check_cols(gamma, D, op, "gamma");
  check_cols(beta, D, op, "beta");
  if (num_rows == 0) {
    dgamma.zero_();
    dbeta.zero_();
    return;
  }
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), op, [&](auto xt) {
    using T = typename decltype(xt)::type;
    const BnGeom g = bn_geom<T>(num_rows, D);
    torch::Tensor slab =
        torch::empty({g.blocks, 2, D}, x.options().dtype(torch::kFloat32));
    dispatch_team(g.cl, [&](auto cl_c) {
      dispatch_depth(depth, kReduceDepth, op, [&](auto depth_c) {
        hipLaunchKernelGGL(
            (batch_norm_bwd_reduce_kernel<T, decltype(cl_c)::value,
                                          decltype(depth_c)::value>),
            dim3(g.blocks, g.tiles), dim3(kBlock), 0, stream,
            slab.data_ptr<float>(), (const T*)dy.data_ptr(),
            (const T*)x.data_ptr(), mean.data_ptr<float>(),
            rstd.data_ptr<float>(), gamma.data_ptr<float>(),
            beta.data_ptr<float>(), num_rows, D, g.chunk, relu);
      });
    });
    hipLaunchKernelGGL(batch_norm_fold_kernel<false>,
                       dim3((D + kFoldCols - 1) / kFoldCols), dim3(kBlock), 0,
                       stream, dgamma.data_ptr<float>(),
                       dbeta.data_ptr<float>(), slab.data_ptr<float>(),
                       g.blocks, D, num_rows, g.chunk);
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void batch_norm_bwd_dx(torch::Tensor dx, torch::Tensor dy, torch::Tensor x,
                       torch::Tensor mean, torch::Tensor rstd,
                       torch::Tensor gamma, torch::Tensor beta,
                       torch::Tensor s_g, torch::Tensor s_gx, double n,
                       bool relu) {
  const char* op = "batch_norm_bwd_dx";
  check_rows(x, op);
  check_same(dy, x, op);
  check_same(dx, x, op);
  const int num_rows = (int)x.size(0);
  const int D = (int)x.size(1);
  check_cols(mean, D, op, "mean");
  check_cols(rstd, D, op, "rstd");
  check_cols(gamma, D, op, "gamma");
  check_cols(beta, D, op, "beta");
  check_cols(s_g, D, op, "s_g");
  check_cols(s_gx, D, op, "s_gx");
  TORCH_CHECK(n >= 1.0, op, ": n must be the global row count, >= 1");
  if (num_rows == 0) return;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), op, [&](auto xt) {
    using T = typename decltype(xt)::type;
    const BnGeom g = bn_geom<T>(num_rows, D);
    const dim3 grid(roc_grid_1d(num_rows, kBlock / g.cl, kRowGridCap),
                    g.tiles);
    dispatch_team(g.cl, [&](auto cl_c) {
      hipLaunchKernelGGL(
          (batch_norm_bwd_dx_kernel<T, decltype(cl_c)::value>), grid,
          dim3(kBlock), 0, stream, (T*)dx.data_ptr(), (const T*)dy.data_ptr(),
          (const T*)x.data_ptr(), mean.data_ptr<float>(),
          rstd.data_ptr<float>(), gamma.data_ptr<float>(),
          beta.data_ptr<float>(), s_g.data_ptr<float>(),
          s_gx.data_ptr<float>(), num_rows, D, (float)n, relu);
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}
