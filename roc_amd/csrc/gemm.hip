// Hand-written MFMA GEMMs for the linear op (CDNA4 / gfx950).
//
//  gemm_rr : C[M,N] = A[M,K] @ B[K,N]   (+ fused ReLU / rowwise scale)
//            A row-major, B passed PRE-TRANSPOSED as Bt[N,K] so both LDS
//            stages are direct coalesced copies (no transpose writes).
//            Replaces reference cublasSgemm fwd/dX (`linear_kernel.cu:76,227`).
//  gemm_atb: C[Ka,N] += A[R,Ka]^T @ B[R,N]   (fp32 out, ordered split-K)
//            the weight-gradient GEMM (reference `linear_kernel.cu:220`,
//            beta=1 accumulate); reduction dim R is the node count (~10^5-6),
//            so blocks split R into fp32 partial slabs, reduced in a
//            fixed order (bit-reproducible).
//
// Element types: bf16 (mfma_f32_16x16x32_bf16, the flagship path) and
// exact fp32 (mfma_f32_16x16x4f32 at the f32 vector rate — gfx950 has no
// xf32; this keeps the reference's fp32-only mode available on GPU).
// Shapes are tall-skinny (M ~ nodes, K/N ~ 41..640): 128-row M-tiles,
// K-step 32, fp32 accumulation, zero-filled staging for every edge tail,
// double-buffered LDS with the T14 split (loads issued before the
// previous tile's MFMAs, LDS writes after).

#include "common.h"

typedef __attribute__((ext_vector_type(8))) short short8;
typedef __attribute__((ext_vector_type(4))) float f32x4;

namespace {

constexpr int BM = 128;   // M rows per block
constexpr int BK = 32;    // K per step
constexpr int PADK = 40;  // LDS row stride in ELEMENTS (16-B aligned)

template <typename ET>
struct GemmTraits;
template <>
struct GemmTraits<unsigned short> {  // bf16 storage
  static constexpr int kEPS = 8;     // elements per 16-B segment
  using Seg = short8;
  static __device__ __forceinline__ Seg zero() {
    return Seg{0, 0, 0, 0, 0, 0, 0, 0};
  }
};
template <>
struct GemmTraits<float> {
  static constexpr int kEPS = 4;
  using Seg = float4;
  static __device__ __forceinline__ Seg zero() {
    return make_float4(0.f, 0.f, 0.f, 0.f);
  }
};

// ---- staging: LOAD half (global -> regs) + WRITE half (regs -> LDS) ----
template <typename ET, int ROWS, bool ALIGNED>
__device__ __forceinline__ void stage_load(
    typename GemmTraits<ET>::Seg (
        &regs)[ROWS * (BK / GemmTraits<ET>::kEPS) / kBlock],
    const ET* __restrict__ g, int row0, int nrows, int64_t ld, int k0,
    int K) {
  constexpr int EPS = GemmTraits<ET>::kEPS;
  constexpr int SPR = BK / EPS;               // segments per row
  constexpr int ROWS_PER_PASS = kBlock / SPR;
  const int seg = threadIdx.x % SPR;
  const int r_in = threadIdx.x / SPR;
#pragma unroll
  for (int pass = 0; pass < ROWS / ROWS_PER_PASS; ++pass) {
    const int gr = row0 + pass * ROWS_PER_PASS + r_in;
    const int gk = k0 + seg * EPS;
    auto v = GemmTraits<ET>::zero();
    if (gr < nrows) {
      const ET* p = g + (int64_t)gr * ld + gk;
      if (ALIGNED && gk + EPS <= K) {
        v = *reinterpret_cast<const typename GemmTraits<ET>::Seg*>(p);
      } else {
        const int nv = min(EPS, K - gk);
        for (int j = 0; j < nv; ++j) v[j] = p[j];
      }
    }
    regs[pass] = v;
  }
}

template <typename ET, int ROWS>
__device__ __forceinline__ void stage_write(
    ET* __restrict__ lds,
    const typename GemmTraits<ET>::Seg (
        &regs)[ROWS * (BK / GemmTraits<ET>::kEPS) / kBlock]) {
  constexpr int EPS = GemmTraits<ET>::kEPS;
  constexpr int SPR = BK / EPS;
  constexpr int ROWS_PER_PASS = kBlock / SPR;
  const int seg = threadIdx.x % SPR;
  const int r_in = threadIdx.x / SPR;
#pragma unroll
  for (int pass = 0; pass < ROWS / ROWS_PER_PASS; ++pass) {
    const int r = pass * ROWS_PER_PASS + r_in;
    *reinterpret_cast<typename GemmTraits<ET>::Seg*>(
        &lds[r * PADK + seg * EPS]) = regs[pass];
  }
}

// one 16x16 output fragment's worth of MFMAs for a BK=32 K-step.
// bf16: a single mfma_f32_16x16x32_bf16; fp32: 8 x mfma_f32_16x16x4f32.
template <typename ET>
__device__ __forceinline__ f32x4 frag_mfma(const ET* a_lds, const ET* b_lds,
                                           int mrow, int nrow, int khalf,
                                           f32x4 acc) {
  if constexpr (sizeof(ET) == 2) {
    const short8 af = *reinterpret_cast<const short8*>(
        &a_lds[mrow * PADK + khalf * 8]);
    const short8 bf = *reinterpret_cast<const short8*>(
        &b_lds[nrow * PADK + khalf * 8]);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
  } else {
#pragma unroll
    for (int kk = 0; kk < BK / 4; ++kk) {
      const float af = a_lds[mrow * PADK + kk * 4 + khalf];
      const float bf = b_lds[nrow * PADK + kk * 4 + khalf];
      acc = __builtin_amdgcn_mfma_f32_16x16x4f32(af, bf, acc, 0, 0, 0);
    }
    return acc;
  }
}

// ---------------------------------------------------------------------------
// gemm_rr
// ---------------------------------------------------------------------------

template <typename ET, int BN, bool RELU, bool ALIGNED_A, bool ALIGNED_B>
__global__ __launch_bounds__(kBlock) void gemm_rr_kernel(
    ET* __restrict__ C, const ET* __restrict__ A, const ET* __restrict__ Bt,
    const float* __restrict__ row_scale, int M, int N, int K) {
  constexpr int NFRAG = BN / 16;
  __shared__ ET a_lds[2][BM * PADK];
  __shared__ ET b_lds[2][BN * PADK];

  const int m_blk = blockIdx.x * BM;
  const int n_blk = blockIdx.y * BN;
  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15;
  const int khalf = lane >> 4;
  const int m_wave = wave * 32;

  f32x4 acc[2][NFRAG];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < NFRAG; ++j) acc[i][j] = {0.f, 0.f, 0.f, 0.f};

  typename GemmTraits<ET>::Seg ra[BM * (BK / GemmTraits<ET>::kEPS) / kBlock];
  typename GemmTraits<ET>::Seg rb[BN * (BK / GemmTraits<ET>::kEPS) / kBlock];
  const int nk = (K + BK - 1) / BK;
  stage_load<ET, BM, ALIGNED_A>(ra, A, m_blk, M, K, 0, K);
  stage_load<ET, BN, ALIGNED_B>(rb, Bt, n_blk, N, K, 0, K);
  stage_write<ET, BM>(a_lds[0], ra);
  stage_write<ET, BN>(b_lds[0], rb);
  __syncthreads();
  int cur = 0;
  for (int kt = 0; kt < nk; ++kt) {
    if (kt + 1 < nk) {  // issue next tile's loads before the MFMAs (T14)
      stage_load<ET, BM, ALIGNED_A>(ra, A, m_blk, M, K, (kt + 1) * BK, K);
      stage_load<ET, BN, ALIGNED_B>(rb, Bt, n_blk, N, K, (kt + 1) * BK, K);
    }
#pragma unroll
    for (int mi = 0; mi < 2; ++mi) {
      const int mrow = m_wave + mi * 16 + l15;
#pragma unroll
      for (int ni = 0; ni < NFRAG; ++ni) {
        acc[mi][ni] = frag_mfma<ET>(a_lds[cur], b_lds[cur], mrow,
                                    ni * 16 + l15, khalf, acc[mi][ni]);
      }
    }
    if (kt + 1 < nk) {
      stage_write<ET, BM>(a_lds[cur ^ 1], ra);
      stage_write<ET, BN>(b_lds[cur ^ 1], rb);
      __syncthreads();
      cur ^= 1;
    }
  }

  // epilogue: C[row][col], row = m_frag + (lane>>4)*4 + j, col = n_frag + l15
#pragma unroll
  for (int mi = 0; mi < 2; ++mi) {
#pragma unroll
    for (int ni = 0; ni < NFRAG; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int row = m_blk + m_wave + mi * 16 + khalf * 4 + j;
        const int col = n_blk + ni * 16 + l15;
        if (row < M && col < N) {
          float v = acc[mi][ni][j];
          if (row_scale) v *= row_scale[row];  // fused rowwise scale
          if (RELU) v = v > 0.f ? v : 0.f;
          f32_to_elt(v, &C[(int64_t)row * N + col]);
        }
      }
    }
  }
}

template <typename ET, int BN>
void launch_rr(ET* C, const ET* A, const ET* Bt, const float* row_scale,
               int M, int N, int K, bool relu, hipStream_t s) {
  dim3 grid((M + BM - 1) / BM, (N + BN - 1) / BN);
  const bool al = (K % GemmTraits<ET>::kEPS) == 0;  // row stride = K
  dispatch_bool(relu, [&](auto relu_c) {
    dispatch_bool(al, [&](auto al_c) {
      constexpr bool AL = decltype(al_c)::value;
      hipLaunchKernelGGL(
          (gemm_rr_kernel<ET, BN, decltype(relu_c)::value, AL, AL>), grid,
          dim3(kBlock), 0, s, C, A, Bt, row_scale, M, N, K);
    });
  });
}

// ---------------------------------------------------------------------------
// gemm_atb (split-K weight-grad GEMM, fp32 slabs reduced in a fixed order)
// ---------------------------------------------------------------------------

constexpr int BKA = 64;  // Ka tile (output rows)
constexpr int BNW = 64;  // N tile (output cols)
constexpr int RB = 32;   // reduction rows per step

// stage a [RB x 64] tile TRANSPOSED into LDS[64][PADK] (lds[c][r]).
//
// bf16 swizzle: the plain [c][r] image puts every lane of a half-wave
// on the same bank pair (column stride 64*PADK bytes for a fixed r is
// 0 mod the 32 write banks), measured at 22% of the 128x128 tile's wave
// cycles in SQ_LDS_BANK_CONFLICT (profiles/r29). Storing row
// r ^ ((cseg&3)<<3) spreads the 8 column-segment lanes over 4 bank
// groups while keeping each khalf-read's 8 elements contiguous; the
// reader compensates with khalf ^ ((c>>3)&3) (frag_mfma_tswz).
// LOAD half: globals -> regs (issue-only; the s_waitcnt lands in the
// WRITE half, so callers can put a full MFMA phase between the two —
// the T14 split; the fused version had zero latency hiding)
template <typename ET, bool ALIGNED>
__device__ __forceinline__ void stage_loadT(
    typename GemmTraits<ET>::Seg (&regs)[RB * 64 / kBlock /
                                         GemmTraits<ET>::kEPS],
    const ET* __restrict__ g, int r0, int nrows, int64_t ld, int c0,
    int ncols) {
  constexpr int EPS = GemmTraits<ET>::kEPS;
  constexpr int SPR = 64 / EPS;           // segments per row of 64 cols
  constexpr int RPP = kBlock / SPR;       // rows per pass
  const int cseg = threadIdx.x % SPR;
  const int r_in = threadIdx.x / SPR;
#pragma unroll
  for (int pass = 0; pass < RB / RPP; ++pass) {
    const int r = pass * RPP + r_in;
    const int gr = r0 + r;
    auto v = GemmTraits<ET>::zero();
    if (gr < nrows) {
      const ET* p = g + (int64_t)gr * ld + c0 + cseg * EPS;
      const int nv = min(EPS, ncols - (c0 + cseg * EPS));
      if (ALIGNED && nv >= EPS) {
        v = *reinterpret_cast<const typename GemmTraits<ET>::Seg*>(p);
      } else {
        for (int j = 0; j < max(nv, 0); ++j) v[j] = p[j];
      }
    }
    regs[pass] = v;
  }
}

// WRITE half: regs -> transposed (bf16: bank-swizzled) LDS image
template <typename ET>
__device__ __forceinline__ void stage_writeT(
    ET* __restrict__ lds,
    const typename GemmTraits<ET>::Seg (&regs)[RB * 64 / kBlock /
                                               GemmTraits<ET>::kEPS]) {
  constexpr int EPS = GemmTraits<ET>::kEPS;
  constexpr int SPR = 64 / EPS;
  constexpr int RPP = kBlock / SPR;
  const int cseg = threadIdx.x % SPR;
  const int r_in = threadIdx.x / SPR;
#pragma unroll
  for (int pass = 0; pass < RB / RPP; ++pass) {
    const int r = pass * RPP + r_in;
    const int rs = (sizeof(ET) == 2) ? (r ^ ((cseg & 3) << 3)) : r;
#pragma unroll
    for (int j = 0; j < EPS; ++j)
      lds[(cseg * EPS + j) * PADK + rs] = (ET)regs[pass][j];
  }
}

template <typename ET, bool ALIGNED>
__device__ __forceinline__ void stage_tile_T(
    ET* __restrict__ lds, const ET* __restrict__ g, int r0, int nrows,
    int64_t ld, int c0, int ncols) {
  typename GemmTraits<ET>::Seg regs[RB * 64 / kBlock /
                                    GemmTraits<ET>::kEPS];
  stage_loadT<ET, ALIGNED>(regs, g, r0, nrows, ld, c0, ncols);
  stage_writeT<ET>(lds, regs);
}

// fragment reader for the swizzled transposed images (bf16; the fp32
// image is stored unswizzled and read by the generic frag_mfma)
template <typename ET>
__device__ __forceinline__ f32x4 frag_mfma_tswz(
    const ET* a_lds, const ET* b_lds, int mrow, int nrow, int khalf,
    f32x4 acc) {
  if constexpr (sizeof(ET) == 2) {
    const int ka = (khalf ^ ((mrow >> 3) & 3)) * 8;
    const int kb = (khalf ^ ((nrow >> 3) & 3)) * 8;
    const short8 af =
        *reinterpret_cast<const short8*>(&a_lds[mrow * PADK + ka]);
    const short8 bf =
        *reinterpret_cast<const short8*>(&b_lds[nrow * PADK + kb]);
    return __builtin_amdgcn_mfma_f32_16x16x32_bf16(af, bf, acc, 0, 0, 0);
  } else {
    return frag_mfma<ET>(a_lds, b_lds, mrow, nrow, khalf, acc);
  }
}

// Split-K epilogue. With one split the block owns its C elements and
// accumulates in place. With several, each split stores its partial tile
// into its own [Ka*N] slab of `part` (every in-range element, zeros
// included: the slab is uninitialised) and atb_reduce_kernel folds the
// slabs into C in a fixed order, so dW is bit-identical from run to run
// (fp32 atomics into C summed in arrival order, and Adam's normalised
// step blew that rounding noise up to percents of the weights).
__device__ __forceinline__ void atb_emit(float* __restrict__ C,
                                         float* __restrict__ part,
                                         int64_t idx, int64_t slab,
                                         float v) {
  if (part != nullptr) part[(int64_t)blockIdx.z * slab + idx] = v;
  else if (v != 0.f) atomicAdd(&C[idx], v);  // sole writer of C[idx]
}

// C[e] += sum_z part[z][e], fixed order: 4 strided z-lanes, then a tree.
constexpr int kRedE = 64, kRedZ = 4;
__global__ __launch_bounds__(kRedE * kRedZ) void atb_reduce_kernel(
    float* __restrict__ C, const float* __restrict__ part, int64_t slab,
    int splitk) {
  __shared__ float red[kRedZ][kRedE];
  const int64_t e = (int64_t)blockIdx.x * kRedE + threadIdx.x;
  float s = 0.f;
  if (e < slab)
    for (int z = threadIdx.y; z < splitk; z += kRedZ)
      s += part[(int64_t)z * slab + e];
  red[threadIdx.y][threadIdx.x] = s;
  __syncthreads();
  if (threadIdx.y == 0 && e < slab)
    C[e] += (red[0][threadIdx.x] + red[1][threadIdx.x]) +
            (red[2][threadIdx.x] + red[3][threadIdx.x]);
}

// One block owns a (TW*64) x (TW*64) output tile, TW in {1, 2}; each wave
// owns TW Ka row-groups (mi) x 4*TW N fragments (ni). The 128x128 tile
// (TW = 2) re-reads A and B across tiles 4x less than the 64x64 one (A is
// re-read per N-tile, B per Ka-tile — at [608,256] that is 2.3 GB/call vs
// 1.16 GB; measured r2c20).
template <typename ET, int TW, bool ALIGNED_A, bool ALIGNED_B>
__global__ __launch_bounds__(kBlock) void gemm_atb_kernel(
    float* __restrict__ C, const ET* __restrict__ A, const ET* __restrict__ B,
    int R, int Ka, int N, int rows_per_split, float* __restrict__ part) {
  __shared__ ET at_lds[TW * BKA * PADK];
  __shared__ ET bt_lds[TW * BNW * PADK];

  const int i_blk = blockIdx.x * (TW * BKA);
  const int n_blk = blockIdx.y * (TW * BNW);
  const int r_begin = blockIdx.z * rows_per_split;
  const int r_end = min(R, r_begin + rows_per_split);

  const int wave = threadIdx.x / 64;
  const int lane = threadIdx.x & 63;
  const int l15 = lane & 15;
  const int khalf = lane >> 4;
  const int i_wave = wave * 16;  // 16 Ka rows per wave and row-group

  f32x4 acc[TW][4 * TW];
#pragma unroll
  for (int mi = 0; mi < TW; ++mi)
#pragma unroll
    for (int ni = 0; ni < 4 * TW; ++ni) acc[mi][ni] = {0.f, 0.f, 0.f, 0.f};

  // T14 split pipeline: chunk r0+RB's global loads (2*TW tile loads) are
  // issued right after the barrier, a full MFMA phase before their
  // s_waitcnt in stage_writeT (the fused stage had zero latency hiding)
  typename GemmTraits<ET>::Seg ra[TW][RB * 64 / kBlock / GemmTraits<ET>::kEPS];
  typename GemmTraits<ET>::Seg rb[TW][RB * 64 / kBlock / GemmTraits<ET>::kEPS];
  auto load_chunk = [&](int r0) {
#pragma unroll
    for (int t = 0; t < TW; ++t)
      stage_loadT<ET, ALIGNED_A>(ra[t], A, r0, r_end, Ka, i_blk + t * BKA, Ka);
#pragma unroll
    for (int t = 0; t < TW; ++t)
      stage_loadT<ET, ALIGNED_B>(rb[t], B, r0, r_end, N, n_blk + t * BNW, N);
  };
  load_chunk(r_begin);
  for (int r0 = r_begin; r0 < r_end; r0 += RB) {
#pragma unroll
    for (int t = 0; t < TW; ++t)
      stage_writeT<ET>(at_lds + t * BKA * PADK, ra[t]);
#pragma unroll
    for (int t = 0; t < TW; ++t)
      stage_writeT<ET>(bt_lds + t * BNW * PADK, rb[t]);
    __syncthreads();
    if (r0 + RB < r_end) load_chunk(r0 + RB);
    const int irow = i_wave + l15;
#pragma unroll
    for (int mi = 0; mi < TW; ++mi) {
#pragma unroll
      for (int ni = 0; ni < 4 * TW; ++ni) {
        acc[mi][ni] = frag_mfma_tswz<ET>(at_lds + mi * BKA * PADK, bt_lds,
                                         irow, ni * 16 + l15, khalf,
                                         acc[mi][ni]);
      }
    }
    __syncthreads();
  }

#pragma unroll
  for (int mi = 0; mi < TW; ++mi) {
#pragma unroll
    for (int ni = 0; ni < 4 * TW; ++ni) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int i = i_blk + mi * BKA + i_wave + khalf * 4 + j;
        const int n = n_blk + ni * 16 + l15;
        if (i < Ka && n < N)
          atb_emit(C, part, (int64_t)i * N + n, (int64_t)Ka * N,
                   acc[mi][ni][j]);
      }
    }
  }
}

template <typename ET>
void launch_atb(float* c, const ET* a, const ET* b, int R, int Ka, int N,
                hipStream_t s, const torch::TensorOptions& c_opts) {
  const bool wide = Ka >= 2 * BKA && N >= 2 * BNW;
  const int tw = wide ? 2 : 1;
  const int tiles = ((Ka + tw * BKA - 1) / (tw * BKA)) *
                    ((N + tw * BNW - 1) / (tw * BNW));
  // split-K count trades fill (tiles*splitk workgroups) against the
  // partial-slab volume (Ka*N*splitk stores + loads); pinned once at first
  // launch (same hipGraph-capture rule as the SpMM knobs)
  static const int splitk_env = [] {
    const char* e = getenv("ROC_ATB_SPLITK");
    return e ? atoi(e) : 0;
  }();
  int splitk = splitk_env > 0 ? splitk_env : 2048 / max(tiles, 1);
  splitk = max(1, min(splitk, (R + RB - 1) / RB));
  const char* det = getenv("ROC_DETERMINISTIC");
  if (det && det[0] == '1') splitk = 1;  // single-pass dW (slower)
  int rows_per_split = ((R + splitk - 1) / splitk + RB - 1) / RB * RB;
  splitk = (R + rows_per_split - 1) / rows_per_split;
  // one [Ka*N] slab per split; from torch's stream-ordered allocator, so
  // it is safe on side streams and under hipGraph capture
  const int64_t slab = (int64_t)Ka * N;
  torch::Tensor part_t;
  float* part = nullptr;
  if (splitk > 1) {
    part_t = torch::empty({(int64_t)splitk * slab}, c_opts);
    part = part_t.data_ptr<float>();
  }
  dim3 grid((Ka + tw * BKA - 1) / (tw * BKA),
            (N + tw * BNW - 1) / (tw * BNW), splitk);
  const bool ala = (Ka % GemmTraits<ET>::kEPS) == 0;
  const bool alb = (N % GemmTraits<ET>::kEPS) == 0;
  dispatch_bool(wide, [&](auto wide_c) {
    dispatch_bool(ala, [&](auto ala_c) {
      dispatch_bool(alb, [&](auto alb_c) {
        hipLaunchKernelGGL(
            (gemm_atb_kernel<ET, decltype(wide_c)::value ? 2 : 1,
                             decltype(ala_c)::value, decltype(alb_c)::value>),
            grid, dim3(kBlock), 0, s, c, a, b, R, Ka, N, rows_per_split,
            part);
      });
    });
  });
  if (part != nullptr) {
    hipLaunchKernelGGL(atb_reduce_kernel,
                       dim3((unsigned)((slab + kRedE - 1) / kRedE)),
                       dim3(kRedE, kRedZ), 0, s, c, part, slab, splitk);
  }
}

}  // namespace

void gemm_rr(torch::Tensor C, torch::Tensor A, torch::Tensor Bt, bool relu,
             c10::optional<torch::Tensor> row_scale) {
  ROC_CHECK_DEV_CONT(C);
  ROC_CHECK_DEV_CONT(A);
  ROC_CHECK_DEV_CONT(Bt);
  TORCH_CHECK(A.scalar_type() == Bt.scalar_type() &&
                  A.scalar_type() == C.scalar_type(),
              "gemm_rr: mixed dtypes");
  const int M = (int)A.size(0), K = (int)A.size(1);
  const int N = (int)Bt.size(0);
  TORCH_CHECK(Bt.size(1) == K, "gemm_rr: Bt must be [N,K]");
  TORCH_CHECK(C.size(0) == M && C.size(1) == N, "gemm_rr: C shape");
  if (M == 0 || N == 0) return;  // empty partition
  if (K == 0) { C.zero_(); return; }
  auto s = roc_stream();
  const float* rs = nullptr;
  if (row_scale.has_value()) {
    TORCH_CHECK(row_scale->scalar_type() == torch::kFloat32 &&
                    row_scale->numel() == M,
                "row_scale must be fp32 [M]");
    rs = row_scale->data_ptr<float>();
  }
  dispatch_elt(A.scalar_type(), "gemm_rr", [&](auto et) {
    using ET = typename decltype(et)::type;
    auto* c = (ET*)C.data_ptr();
    auto* a = (const ET*)A.data_ptr();
    auto* b = (const ET*)Bt.data_ptr();
    if (N > 64) launch_rr<ET, 128>(c, a, b, rs, M, N, K, relu, s);
    else        launch_rr<ET, 64>(c, a, b, rs, M, N, K, relu, s);
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void gemm_atb(torch::Tensor C, torch::Tensor A, torch::Tensor B) {
  ROC_CHECK_DEV_CONT(C);
  ROC_CHECK_DEV_CONT(A);
  ROC_CHECK_DEV_CONT(B);
  TORCH_CHECK(A.scalar_type() == B.scalar_type(), "gemm_atb: mixed dtypes");
  TORCH_CHECK(C.scalar_type() == torch::kFloat32, "gemm_atb: fp32 out");
  const int R = (int)A.size(0), Ka = (int)A.size(1);
  const int N = (int)B.size(1);
  TORCH_CHECK(B.size(0) == R, "gemm_atb: row mismatch");
  TORCH_CHECK(C.size(0) == Ka && C.size(1) == N, "gemm_atb: C shape");
  if (R == 0 || Ka == 0 || N == 0) return;  // empty partition: C += 0
  auto s = roc_stream();
  dispatch_elt(A.scalar_type(), "gemm_atb", [&](auto et) {
    using ET = typename decltype(et)::type;
    launch_atb<ET>(C.data_ptr<float>(), (const ET*)A.data_ptr(),
                   (const ET*)B.data_ptr(), R, Ka, N, s, C.options());
  });
  ROC_HIP_CHECK(hipGetLastError());
}
