// DropEdge neighbour aggregation for CDNA4: the CSR SpMM that decides, per
// edge and inside the gather kernel, whether the edge exists this epoch. A
// dropped edge costs its 4-B index and one Philox draw, and no gather.
//
//   out[v, :] = row_scale[v] * 1/(1-p) * sum_{kept e of row v} x[u_e, :]
//
// The mask (shared with ops/reference.py, bit for bit):
//   edge (v <- u) is kept  iff  philox4x32_10(idx, off, seed).x >= thresh
//   idx    = (uint64(v) << 32) | uint32(u), v the destination row and u the
//            (halo-extended) source id, both in the FORWARD orientation
//   thresh = min(floor(p * 2^32), 2^32 - 1), computed on the host in double;
//            the kernel compares integers
//   off    = counter ? *counter * 65536 + offset : offset  (dropout.hip's rule)
//   the Philox stream word is kPhiloxEdgeStream, so the edge mask and the
//   feature mask of one (seed, offset) are independent
// It follows that
//  - the mask needs no edge id and no edge permutation: the transpose CSR
//    evaluates the same function with the roles of row and column swapped
//    (TRANSPOSED), so the backward is this kernel over (t_rowptr, t_colidx)
//  - duplicate (u, v) edges share one fate
//  - the key is the shard's local ids: another partitioning draws another,
//    equally valid, mask
//
// The kernel is spmm_kernel's row-team frame (row_team.h, gather.h,
// csr_launch.h): a team of TEAM lanes per row, column tiles on blockIdx.y,
// both gather engines, row_order with its cut-off, a cold scalar path for a
// unit that straddles D. What is its own is how the indices reach the ladder:
//  - a team takes its row in windows of 64 edges; its lanes load the window's
//    colidx coalesced, 64/TEAM statically indexed loads per lane (the plain
//    kernel has every lane of the team re-read the same index)
//  - each lane draws the mask of its own edges: one Philox per lane serves 64
//    decisions per wave pass
//  - the team's slice of the wave ballot, and a popcount of the bits below the
//    lane, rank the kept edges; the kept sources go in rank order - ascending
//    edge order - into the team's ring in LDS
//  - gather_group runs over the ring in whole groups of 16, so 16 kept gathers
//    are in flight however the drops fall; fewer than 16 left over are carried
//    into the next window, and only the row's last window drains down the
//    8 / 4 / 1 ladder. The ring holds 80 entries (at most 15 carried + 64
//    new); a group of 16 starts at a multiple of 16 and never wraps
//  - one team adds a row's kept edges in ascending edge order, so the result
//    does not depend on grid, engine or row order
// Teams of a wave run different trip counts, so nothing in the row or window
// loops is a workgroup barrier: ring writes and reads of a team are ordered by
// wavefront-scope fences around a wave barrier (one wave issues its LDS
// operations in order).
// Rows with no edges, and rows whose edges are all dropped, store zeros.

#include "csr_launch.h"
#include "gather.h"
#include "philox.h"

// built without the packed fp32 ALU forms, like spmm_fp8.hip
#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute push(__attribute__((target("no-packed-fp32-ops"))), \
                             apply_to = function)
#endif

namespace {

constexpr int kWin = 64;      // edges of one window
constexpr int kGroup = 16;    // gathers in flight
constexpr int kRing = 80;     // kGroup - 1 carried + kWin new, rounded up
constexpr int kRingLd = 84;   // ring stride: teams of a wave on distinct banks

template <bool TRANSPOSED>
__device__ __forceinline__ bool edge_kept(int row, int col, unsigned off,
                                          unsigned long long seed,
                                          unsigned thresh) {
  const unsigned v = (unsigned)(TRANSPOSED ? col : row);
  const unsigned u = (unsigned)(TRANSPOSED ? row : col);
  const unsigned long long idx = ((unsigned long long)v << 32) | u;
  return philox4x32_10(idx, off, seed, kPhiloxEdgeStream).x >= thresh;
}

__device__ __forceinline__ void acc_add(float* acc, const uint4& r) {
  float v[8];
  unpack(v, r);
#pragma unroll
  for (int j = 0; j < 8; ++j) acc[j] += v[j];
}
__device__ __forceinline__ void acc_add(float* acc, const float4& r) {
  acc[0] += r.x; acc[1] += r.y; acc[2] += r.z; acc[3] += r.w;
}

// acc += x[ring[c + i], unit] for N consecutive ring entries
template <int N, typename T, typename LD>
__device__ __forceinline__ void ring_group(float* __restrict__ acc,
                                           const LD& ld, const int* ring,
                                           int c) {
  gather_group<N, T>(ld, ring, c,
                     [&](int, int, const typename RawVec<T>::type& r) {
    acc_add(acc, r);
  });
}

// ring writes of a team before, ring reads after (and the reverse)
__device__ __forceinline__ void team_lds_order() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

template <typename T, int TEAM, bool BUF, bool TRANSPOSED>
__global__ __launch_bounds__(kBlock) void spmm_drop_kernel(
    T* __restrict__ out, const T* __restrict__ x,
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const float* __restrict__ row_scale, const int* __restrict__ row_order,
    int num_rows, int64_t D, unsigned x_bytes, unsigned thresh,
    float inv_keep, unsigned long long seed, unsigned offset,
    const long long* __restrict__ counter) {
  constexpr int EPU = EltTraits<T>::kPerVec;
  constexpr int PER = kWin / TEAM;  // index loads of one lane per window
  __shared__ __attribute__((aligned(16))) int rings[(kBlock / TEAM) * kRingLd];
  const RowTeam<TEAM> rt;
  int* ring = rings + ((int)threadIdx.x / TEAM) * kRingLd;
  const unsigned off = philox_call_offset(counter, offset);

  const int64_t col0 = ((int64_t)blockIdx.y * TEAM + rt.lane) * EPU;
  const bool full = col0 + EPU <= D;
  const int nvalid = full ? EPU : (col0 < D ? (int)(D - col0) : 0);
  const auto g = make_gather<T, BUF>(x, x_bytes, D, col0);

  // this team's bits of a wave ballot, and the bits below this lane
  const int tshift = ((int)threadIdx.x & 63) & ~(TEAM - 1);
  const unsigned long long tmask = TEAM == 64 ? ~0ull : (1ull << TEAM) - 1;
  const unsigned long long below = (1ull << rt.lane) - 1;

  for (int ri = rt.team; ri < num_rows; ri += rt.nteams) {
    const int row = row_order ? row_order[ri] : ri;
    const int64_t e0 = rowptr[row];
    const int64_t e1 = rowptr[row + 1];
    float acc[EPU];
#pragma unroll
    for (int j = 0; j < EPU; ++j) acc[j] = 0.f;

    // head, avail and every trip count below are uniform over the team
    int head = 0;   // ring position of the oldest entry, a multiple of 16
    int avail = 0;  // entries queued
    for (int64_t w = e0; w < e1; w += kWin) {
      int u[PER];
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const int64_t e = w + i * TEAM + rt.lane;
        u[i] = e < e1 ? colidx[e] : -1;
      }
#pragma unroll
      for (int i = 0; i < PER; ++i) {
        const bool keep = u[i] >= 0 &&
                          edge_kept<TRANSPOSED>(row, u[i], off, seed, thresh);
        const unsigned long long b = (__ballot(keep) >> tshift) & tmask;
        if (keep) {
          int pos = head + avail + __popcll(b & below);
          if (pos >= kRing) pos -= kRing;
          ring[pos] = u[i];
        }
        avail += __popcll(b);
      }
      team_lds_order();

      const bool last = w + kWin >= e1;
      const int groups = avail / kGroup;
      const int rest = last ? avail % kGroup : 0;  // drained now
      if (full) {
        int c = head;
        for (int k = 0; k < groups; ++k) {
          ring_group<kGroup, T>(acc, g, ring, c);
          c = c + kGroup == kRing ? 0 : c + kGroup;
        }
        const int c1 = c + rest;  // c <= 64 and rest < 16: no wrap
        ROC_EDGE_LADDER(8, c, c1, ring_group<ROC_LADDER_N, T>(acc, g, ring, c));
      } else if (nvalid > 0) {
        // cold path: the unit straddles D (D % EPU != 0), scalar loads
        const int n = groups * kGroup + rest;
        for (int k = 0; k < n; ++k) {
          const int c = head + k;
          const T* r = x + (int64_t)ring[c >= kRing ? c - kRing : c] * D + col0;
#pragma unroll
          for (int j = 0; j < EPU; ++j)
            if (j < nvalid) acc[j] += elt_to_f32(r[j]);
        }
      }
      head = (head + groups * kGroup) % kRing;
      avail -= groups * kGroup + rest;
      team_lds_order();
    }

    const float s = (row_scale ? row_scale[row] : 1.f) * inv_keep;
    T* o = out + (int64_t)row * D + col0;
    if (full) {
#pragma unroll
      for (int j = 0; j < EPU; ++j) acc[j] *= s;
      store_vec(o, acc);
    } else if (nvalid > 0) {
#pragma unroll
      for (int j = 0; j < EPU; ++j)
        if (j < nvalid) f32_to_elt(acc[j] * s, o + j);
    }
  }
}

// out[e] = 1 if edge e of the CSR is kept, else 0: a wave per row
template <bool TRANSPOSED>
__global__ __launch_bounds__(kBlock) void drop_edge_mask_kernel(
    unsigned char* __restrict__ out, const int64_t* __restrict__ rowptr,
    const int* __restrict__ colidx, int num_rows, unsigned thresh,
    unsigned long long seed, unsigned offset,
    const long long* __restrict__ counter) {
  const RowTeam<64> rt;
  const unsigned off = philox_call_offset(counter, offset);
  for (int row = rt.team; row < num_rows; row += rt.nteams) {
    const int64_t e1 = rowptr[row + 1];
    for (int64_t e = rowptr[row] + rt.lane; e < e1; e += 64)
      out[e] = edge_kept<TRANSPOSED>(row, colidx[e], off, seed, thresh);
  }
}

// the integer the kernels compare a draw with
unsigned drop_thresh(double p, const char* what) {
  TORCH_CHECK(p >= 0.0 && p < 1.0, what, ": p must be in [0, 1)");
  const double t = std::floor(p * 4294967296.0);
  return t >= 4294967295.0 ? 0xFFFFFFFFu : (unsigned)t;
}

const long long* counter_ptr(const c10::optional<torch::Tensor>& counter,
                             const char* what) {
  if (!counter.has_value()) return nullptr;
  TORCH_CHECK(counter->is_cuda() && counter->scalar_type() == torch::kInt64 &&
                  counter->numel() == 1,
              what, ": counter must be a GPU int64[1] tensor");
  return (const long long*)counter->data_ptr<int64_t>();
}

}  // namespace

#if defined(__HIP_DEVICE_COMPILE__)
#pragma clang attribute pop
#endif

void spmm_drop(torch::Tensor out, torch::Tensor x, torch::Tensor rowptr,
               torch::Tensor colidx, double p, int64_t seed, int64_t offset,
               c10::optional<torch::Tensor> counter,
               c10::optional<torch::Tensor> row_scale,
               c10::optional<torch::Tensor> row_order, bool transposed) {
  check_mat_pair(out, "out", x, "x", "spmm_drop");
  TORCH_CHECK(out.scalar_type() == x.scalar_type(),
              "spmm_drop: dtype mismatch");
  const int num_rows = (int)out.size(0);
  const int64_t D = out.size(1);
  check_csr(rowptr, colidx, num_rows, "spmm_drop");
  const unsigned thresh = drop_thresh(p, "spmm_drop");
  const long long* cnt = counter_ptr(counter, "spmm_drop");
  if (row_scale.has_value())
    TORCH_CHECK(row_scale->is_cuda() && row_scale->is_contiguous() &&
                    row_scale->scalar_type() == torch::kFloat32 &&
                    row_scale->numel() == num_rows,
                "spmm_drop: row_scale must be a contiguous fp32 GPU tensor, "
                "one entry per row");
  if (num_rows == 0 || D == 0) return;
  if (colidx.numel() == 0 || x.size(0) == 0) {  // nothing to gather
    out.zero_();
    return;
  }
  const float inv_keep = (float)(1.0 / (1.0 - p));
  const float* rs = row_scale.has_value() ? row_scale->data_ptr<float>()
                                          : nullptr;
  auto stream = roc_stream();
  dispatch_elt(x.scalar_type(), "spmm_drop", [&](auto xt) {
    using T = typename decltype(xt)::type;
    constexpr int EPU = EltTraits<T>::kPerVec;
    const GatherGeom g =
        gather_geom<T>(num_rows, (D + EPU - 1) / EPU, 0, (size_t)x.numel());
    const int* order = row_order_ptr(row_order, num_rows, g.team, "spmm_drop");
    dispatch_gather(g, [&](auto team_c, auto buf_c) {
      dispatch_bool(transposed, [&](auto tr_c) {
        hipLaunchKernelGGL(
            (spmm_drop_kernel<T, decltype(team_c)::value,
                              decltype(buf_c)::value, decltype(tr_c)::value>),
            g.grid, dim3(kBlock), 0, stream, (T*)out.data_ptr(),
            (const T*)x.data_ptr(), rowptr.data_ptr<int64_t>(),
            colidx.data_ptr<int>(), rs, order, num_rows, D, g.bytes, thresh,
            inv_keep, (unsigned long long)seed, (unsigned)offset, cnt);
      });
    });
  });
  ROC_HIP_CHECK(hipGetLastError());
}

void drop_edge_mask(torch::Tensor out, torch::Tensor rowptr,
                    torch::Tensor colidx, double p, int64_t seed,
                    int64_t offset, c10::optional<torch::Tensor> counter,
                    bool transposed) {
  ROC_CHECK_DEV_CONT(out);
  TORCH_CHECK(out.scalar_type() == torch::kUInt8 &&
                  out.numel() == colidx.numel(),
              "drop_edge_mask: out must be uint8, one entry per edge");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.numel() >= 1 &&
                  rowptr.numel() - 1 < INT_MAX,
              "drop_edge_mask: bad rowptr");
  const int num_rows = (int)rowptr.numel() - 1;
  check_csr(rowptr, colidx, num_rows, "drop_edge_mask");
  const unsigned thresh = drop_thresh(p, "drop_edge_mask");
  const long long* cnt = counter_ptr(counter, "drop_edge_mask");
  if (num_rows == 0 || colidx.numel() == 0) return;
  auto stream = roc_stream();
  dispatch_bool(transposed, [&](auto tr_c) {
    hipLaunchKernelGGL((drop_edge_mask_kernel<decltype(tr_c)::value>),
                       row_team_grid(num_rows, 64), dim3(kBlock), 0, stream,
                       out.data_ptr<uint8_t>(), rowptr.data_ptr<int64_t>(),
                       colidx.data_ptr<int>(), num_rows, thresh,
                       (unsigned long long)seed, (unsigned)offset, cnt);
  });
  ROC_HIP_CHECK(hipGetLastError());
}
