// Device-side neighbour sampling for the mini-batch tier (CDNA4, wave64).
//
// One hop = the bit-exact device twin of graph_cpu.cpp sample_hop plus
// csr_transpose: the same per-row splitmix64 stream, the same Floyd
// selection order, the same first-appearance local ids, the same stable
// transpose. Stages, all on the current stream:
//
//   count   cnt[i] = min(fanout, deg(targets[i])), inv_deg; scan -> rowptr_s
//   pick    a TEAM of T lanes per row; Floyd's k selected offsets live in
//           the team's registers (R per lane, slot q in lane q % T,
//           register q / T); membership = R compares + one team ballot
//   relabel mark / claim (atomicMin) / own / scan / assign / relabel over a
//           persistent two-array workspace (slot, first) of the graph's N
//           nodes: no hash table, no sort; release restores it in O(n_src)
//   transp  one stable torch::sort of the local ids gives the edge
//           permutation; kernels here gather the rows and count per source
//
// The exclusive scan is three launches (block sums, one block over the
// sums, add-back): no kernel waits on another workgroup. Every atomic is an
// integer atomicMin / atomicAdd on global memory, so no result depends on
// the schedule. Also here: gather_rows_cast, the input-row gather that
// replaces the host index + copy + cast when the features are HBM-resident.

#include <climits>
#include <vector>

#include "common.h"

namespace {

constexpr int kScanItems = 4;                     // per thread
constexpr int kScanTile = kBlock * kScanItems;    // per block

__device__ __forceinline__ unsigned long long splitmix64(
    unsigned long long x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

// ---------------------------------------------------------------------------
// exclusive scan: int32 in, int32 / int64 out, out[n] = total
// ---------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ T wave_scan_incl(T v) {
  const int lane = threadIdx.x & 63;
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const T o = __shfl_up(v, d);
    if (lane >= d) v += o;
  }
  return v;
}

// inclusive scan over the block's kBlock values; total = their sum
template <typename T>
__device__ __forceinline__ T block_scan_incl(T v, T* lds, T& total) {
  const int w = threadIdx.x >> 6;
  v = wave_scan_incl(v);
  if ((threadIdx.x & 63) == 63) lds[w] = v;
  __syncthreads();
  T off = 0, sum = 0;
#pragma unroll
  for (int q = 0; q < kBlock / 64; ++q) {
    if (q < w) off += lds[q];
    sum += lds[q];
  }
  total = sum;
  __syncthreads();
  return v + off;
}

template <typename TOut>
__device__ __forceinline__ TOut scan_load(const int* __restrict__ in,
                                          int64_t n, int (&v)[kScanItems]) {
  const int64_t i0 =
      (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
  TOut s = 0;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    v[j] = (i0 + j < n) ? in[i0 + j] : 0;
    s += (TOut)v[j];
  }
  return s;
}

template <typename TOut>
__global__ __launch_bounds__(kBlock) void scan_block_sums_kernel(
    const int* __restrict__ in, TOut* __restrict__ partial, int64_t n) {
  __shared__ TOut lds[kBlock / 64];
  int v[kScanItems];
  TOut total;
  block_scan_incl(scan_load<TOut>(in, n, v), lds, total);
  if (threadIdx.x == 0) partial[blockIdx.x] = total;
}

// one block: partial[] -> its exclusive scan, in chunks with a carry
template <typename TOut>
__global__ __launch_bounds__(kBlock) void scan_partials_kernel(
    TOut* __restrict__ partial, int nb) {
  __shared__ TOut lds[kBlock / 64];
  TOut carry = 0;
  for (int base = 0; base < nb; base += kBlock) {
    const int i = base + (int)threadIdx.x;
    const TOut v = i < nb ? partial[i] : (TOut)0;
    TOut total;
    const TOut incl = block_scan_incl(v, lds, total);
    if (i < nb) partial[i] = carry + incl - v;
    carry += total;
  }
}

template <typename TOut>
__global__ __launch_bounds__(kBlock) void scan_add_back_kernel(
    const int* __restrict__ in, const TOut* __restrict__ partial,
    TOut* __restrict__ out, int64_t n) {
  __shared__ TOut lds[kBlock / 64];
  int v[kScanItems];
  const TOut s = scan_load<TOut>(in, n, v);
  TOut total;
  TOut run = partial[blockIdx.x] + block_scan_incl(s, lds, total) - s;
  const int64_t i0 =
      (int64_t)blockIdx.x * kScanTile + (int64_t)threadIdx.x * kScanItems;
#pragma unroll
  for (int j = 0; j < kScanItems; ++j) {
    if (i0 + j < n) {
      out[i0 + j] = run;
      run += (TOut)v[j];
      if (i0 + j == n - 1) out[n] = run;
    }
  }
}

// out: [n + 1]. n == 0 leaves out[0] to the caller (allocated zeroed).
template <typename TOut>
void exclusive_scan(const int* in, TOut* out, int64_t n,
                    torch::ScalarType st, const torch::Device& dev,
                    hipStream_t s) {
  if (n <= 0) return;
  const int nb = (int)((n + kScanTile - 1) / kScanTile);
  auto partial = torch::empty({nb}, torch::dtype(st).device(dev));
  TOut* pp = (TOut*)partial.data_ptr();
  hipLaunchKernelGGL((scan_block_sums_kernel<TOut>), dim3(nb), dim3(kBlock),
                     0, s, in, pp, n);
  hipLaunchKernelGGL((scan_partials_kernel<TOut>), dim3(1), dim3(kBlock), 0,
                     s, pp, nb);
  hipLaunchKernelGGL((scan_add_back_kernel<TOut>), dim3(nb), dim3(kBlock), 0,
                     s, in, (const TOut*)pp, out, n);
}

// ---------------------------------------------------------------------------
// count: cnt, inv_deg; a target outside [0, N) counts 0 and raises *bad
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sample_count_kernel(
    const int64_t* __restrict__ rowptr, const int64_t* __restrict__ targets,
    int* __restrict__ cnt, float* __restrict__ inv_deg,
    int64_t* __restrict__ bad, int64_t n_dst, int64_t N, int fanout) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_dst) return;
  const int64_t v = targets[i];
  int c = 0;
  if (v < 0 || v >= N) {
    *bad = 1;  // every writer stores the same value
  } else {
    const int64_t deg = rowptr[v + 1] - rowptr[v];
    c = (int)(deg < (int64_t)fanout ? deg : (int64_t)fanout);
  }
  cnt[i] = c;
  inv_deg[i] = __fdiv_rn(1.0f, (float)(c > 1 ? c : 1));
}

// ---------------------------------------------------------------------------
// pick: T lanes per row, adjacent teams take adjacent rows. Rows with
// deg <= fanout copy their edges in order. The others run Floyd's
// algorithm: the loop over j is the same for every lane of the team (each
// lane steps the row's splitmix64 stream itself: no broadcast, no LDS), and
// its trip count, fanout, is the same for every team, so the whole wave
// walks it together and the ballot below always sees all 64 lanes.
// ---------------------------------------------------------------------------
template <int T, int R>
__global__ __launch_bounds__(kBlock) void sample_pick_kernel(
    const int64_t* __restrict__ rowptr, const int* __restrict__ colidx,
    const int64_t* __restrict__ targets, const int64_t* __restrict__ rowptr_s,
    int* __restrict__ picked, int* __restrict__ erow, int64_t n_dst,
    int fanout, unsigned long long seed) {
  static_assert(64 % T == 0, "a team never straddles a wave");
  const int64_t row = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / T;
  const int tl = threadIdx.x % T;
  const int tbase = (threadIdx.x & 63) & ~(T - 1);
  const unsigned long long tmask =
      T == 64 ? ~0ull : ((1ull << (T & 63)) - 1ull);
  int64_t v = 0, lo = 0, base = 0;
  int deg = 0;
  if (row < n_dst) {
    v = targets[row];
    base = rowptr_s[row];
    // a row the count kernel refused (bad target) has no edges
    if (rowptr_s[row + 1] > base) {
      lo = rowptr[v];
      deg = (int)(rowptr[v + 1] - lo);
    }
  }
  const bool sampled = deg > fanout;
  if (!sampled) {
    for (int k = tl; k < deg; k += T) {
      picked[base + k] = colidx[lo + k];
      erow[base + k] = (int)row;
    }
  }
  if (__ballot(sampled) == 0ull) return;  // wave-uniform

  int sel[R];
#pragma unroll
  for (int r = 0; r < R; ++r) sel[r] = -1;
  unsigned long long st = splitmix64((seed << 20) ^ (unsigned long long)v);
  const int j0 = deg - fanout;
  for (int k = 0; k < fanout; ++k) {
    st = splitmix64(st);
    const int j = j0 + k;
    // a team that only copies rides along with a harmless divisor
    const unsigned long long d = sampled ? (unsigned long long)(j + 1) : 1ull;
    const int t = (int)(st % d);
    bool hit = false;
#pragma unroll
    for (int r = 0; r < R; ++r) hit |= (sel[r] == t);
    const bool seen = ((__ballot(hit) >> tbase) & tmask) != 0ull;
    const int val = seen ? j : t;
    const int kr = k / T;  // wave-uniform
    if (tl == k % T) {
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (r == kr) sel[r] = val;
    }
  }
  if (sampled) {
#pragma unroll
    for (int r = 0; r < R; ++r) {
      const int k = r * T + tl;
      if (k < fanout) {
        picked[base + k] = colidx[lo + sel[r]];
        erow[base + k] = (int)row;
      }
    }
  }
}

// ---------------------------------------------------------------------------
// relabel over the (slot, first) workspace
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kBlock) void sample_mark_kernel(
    const int64_t* __restrict__ targets, int* __restrict__ slot,
    int64_t n_dst, int64_t N) {
  const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (i >= n_dst) return;
  const int64_t v = targets[i];
  if (v >= 0 && v < N) slot[v] = (int)i;
}

__global__ __launch_bounds__(kBlock) void sample_claim_kernel(
    const int* __restrict__ picked, const int* __restrict__ slot,
    int* __restrict__ first, int64_t ne) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= ne) return;
  const int u = picked[e];
  if (slot[u] < 0) atomicMin(&first[u], (int)e);
}

__global__ __launch_bounds__(kBlock) void sample_own_kernel(
    const int* __restrict__ picked, const int* __restrict__ slot,
    const int* __restrict__ first, int* __restrict__ flag, int64_t ne) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= ne) return;
  const int u = picked[e];
  flag[e] = (slot[u] < 0 && first[u] == (int)e) ? 1 : 0;
}

// threads [0, ne): owners publish their id; threads [0, n_dst): the
// targets are the first n_dst sources
__global__ __launch_bounds__(kBlock) void sample_assign_kernel(
    const int* __restrict__ picked, const int* __restrict__ flag,
    const int* __restrict__ rank, const int64_t* __restrict__ targets,
    int* __restrict__ slot, int64_t* __restrict__ src_ids, int64_t ne,
    int64_t n_dst) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e < n_dst) src_ids[e] = targets[e];
  if (e < ne && flag[e]) {
    const int u = picked[e];
    const int64_t id = n_dst + rank[e];
    slot[u] = (int)id;
    src_ids[id] = u;
  }
}

__global__ __launch_bounds__(kBlock) void sample_relabel_kernel(
    const int* __restrict__ picked, const int* __restrict__ slot,
    int* __restrict__ colidx_local, int* __restrict__ t_cnt, int64_t ne) {
  const int64_t e = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (e >= ne) return;
  const int id = slot[picked[e]];
  colidx_local[e] = id;
  atomicAdd(&t_cnt[id], 1);
}

// restore slot = -1, first = INT_MAX at the listed nodes
template <typename TI>
__global__ __launch_bounds__(kBlock) void sample_release_kernel(
    const TI* __restrict__ ids, int* __restrict__ slot,
    int* __restrict__ first, int64_t n, int64_t N) {
  const int64_t j = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (j >= n) return;
  const int64_t u = (int64_t)ids[j];
  if (u < 0 || u >= N) return;
  slot[u] = -1;
  first[u] = INT_MAX;
}

// transposed edge q came from forward edge perm[q]
__global__ __launch_bounds__(kBlock) void sample_transpose_kernel(
    const int64_t* __restrict__ perm, const int* __restrict__ erow,
    int* __restrict__ t_eperm, int* __restrict__ t_colidx, int64_t ne) {
  const int64_t q = (int64_t)blockIdx.x * kBlock + threadIdx.x;
  if (q >= ne) return;
  const int64_t e = perm[q];
  t_eperm[q] = (int)e;
  t_colidx[q] = erow[e];
}

// ---------------------------------------------------------------------------
// gather_rows_cast: out[j, :] = in[ids[j], :]. A team of T lanes per row,
// the row index loaded by the team's first lane and shuffled. With
// D % 8 == 0 every row starts 16-B aligned in both types and moves in
// 8-element units (16-B lane loads and stores); otherwise row starts are
// not aligned and the row moves element by element (lanes still walk
// consecutive addresses).
// ---------------------------------------------------------------------------
__device__ __forceinline__ void load_unit8(const float* p, float (&a)[8]) {
  load_f32x4(p, a);
  load_f32x4(p + 4, a + 4);
}
__device__ __forceinline__ void load_unit8(const unsigned short* p,
                                           float (&a)[8]) {
  load_bf16x8(p, a);
}

template <typename TIn, typename TOut>
__global__ __launch_bounds__(kBlock) void gather_rows_cast_kernel(
    TOut* __restrict__ out, const TIn* __restrict__ in,
    const int64_t* __restrict__ ids, int64_t n, int64_t n_in, int D, int T) {
  const int64_t team = ((int64_t)blockIdx.x * kBlock + threadIdx.x) / T;
  const int64_t nteams = (int64_t)gridDim.x * kBlock / T;
  const int tl = threadIdx.x % T;
  const int dv = (D % 8 == 0) ? D : 0;  // the part moved in 16-B units
  for (int64_t row = team; row < n; row += nteams) {
    long long id = tl == 0 ? (long long)ids[row] : 0ll;
    id = __shfl(id, 0, T);
    if (id < 0 || id >= n_in) continue;  // never read outside `in`
    const TIn* src = in + id * (int64_t)D;
    TOut* dst = out + row * (int64_t)D;
    for (int c = tl * 8; c < dv; c += T * 8) {
      float a[8];
      load_unit8(src + c, a);
      store_vec(dst + c, a);
    }
    for (int c = dv + tl; c < D; c += T)
      f32_to_elt(elt_to_f32(src[c]), dst + c);
  }
}

inline dim3 grid_for(int64_t n) {
  return dim3((unsigned)((n + kBlock - 1) / kBlock));
}

template <int T, int R>
void launch_pick(const int64_t* rowptr, const int* colidx,
                 const int64_t* targets, const int64_t* rowptr_s, int* picked,
                 int* erow, int64_t n_dst, int fanout,
                 unsigned long long seed, hipStream_t s) {
  hipLaunchKernelGGL((sample_pick_kernel<T, R>), grid_for(n_dst * T),
                     dim3(kBlock), 0, s, rowptr, colidx, targets, rowptr_s,
                     picked, erow, n_dst, fanout, seed);
}

}  // namespace

// One sampled hop on the device. slot / first: the sampler's persistent
// int32 [N] workspace (-1 / INT_MAX everywhere on entry, and again on every
// exit). Returns {rowptr_s i64 [n_dst+1], colidx_local i32 [E_s],
// src_ids i64 [n_src], t_rowptr i64 [n_src+1], t_colidx i32 [E_s],
// t_edge_perm i32 [E_s], inv_deg f32 [n_dst]}. Two host reads: E_s (with
// the bad-target flag) and n_src.
std::vector<torch::Tensor> sample_hop_device(torch::Tensor rowptr,
                                             torch::Tensor colidx,
                                             torch::Tensor targets,
                                             int64_t fanout, int64_t seed,
                                             torch::Tensor slot,
                                             torch::Tensor first) {
  ROC_CHECK_DEV_CONT(rowptr);
  ROC_CHECK_DEV_CONT(colidx);
  ROC_CHECK_DEV_CONT(targets);
  ROC_CHECK_DEV_CONT(slot);
  ROC_CHECK_DEV_CONT(first);
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64, "rowptr must be int64");
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32, "colidx must be int32");
  TORCH_CHECK(targets.scalar_type() == torch::kInt64,
              "targets must be int64");
  TORCH_CHECK(slot.scalar_type() == torch::kInt32 &&
                  first.scalar_type() == torch::kInt32,
              "workspace must be int32");
  TORCH_CHECK(targets.dim() == 1 && rowptr.dim() == 1 && rowptr.numel() >= 1);
  TORCH_CHECK(rowptr.device() == colidx.device() &&
                  rowptr.device() == targets.device() &&
                  rowptr.device() == slot.device() &&
                  rowptr.device() == first.device(),
              "sample_hop_device: all tensors must share one device");
  TORCH_CHECK(fanout >= 1, "fanout must be positive");
  TORCH_CHECK(fanout <= 512, "sample_hop_device: fanout ", fanout,
              " is above the sampler's limit of 512");
  const int64_t N = rowptr.numel() - 1;
  const int64_t n_dst = targets.numel();
  TORCH_CHECK(N < (1ll << 31), "sample_hop_device: N must be below 2^31");
  TORCH_CHECK(slot.numel() == N && first.numel() == N,
              "workspace must have one entry per graph node");
  TORCH_CHECK(n_dst * fanout < (1ll << 31),
              "sample_hop_device: n_dst * fanout must be below 2^31");

  const auto dev = rowptr.device();
  const auto i32 = torch::dtype(torch::kInt32).device(dev);
  const auto i64 = torch::dtype(torch::kInt64).device(dev);
  auto s = roc_stream();
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();
  const int64_t* tg = targets.data_ptr<int64_t>();
  int* slot_p = slot.data_ptr<int>();
  int* first_p = first.data_ptr<int>();
  const int fo = (int)fanout;

  // [rowptr_s | bad-target flag]: one copy brings E_s and the flag back
  auto head = torch::zeros({n_dst + 2}, i64);
  auto rowptr_s = head.narrow(0, 0, n_dst + 1);
  auto inv_deg = torch::empty({n_dst}, torch::dtype(torch::kFloat32).device(dev));
  int64_t ne = 0;
  if (n_dst > 0) {
    auto cnt = torch::empty({n_dst}, i32);
    hipLaunchKernelGGL(sample_count_kernel, grid_for(n_dst), dim3(kBlock), 0,
                       s, rp, tg, cnt.data_ptr<int>(),
                       inv_deg.data_ptr<float>(),
                       head.data_ptr<int64_t>() + n_dst + 1, n_dst, N, fo);
    exclusive_scan<int64_t>(cnt.data_ptr<int>(), head.data_ptr<int64_t>(),
                            n_dst, torch::kInt64, dev, s);
    ROC_HIP_CHECK(hipGetLastError());
    auto tail = head.narrow(0, n_dst, 2).cpu();  // host read 1
    ne = tail.data_ptr<int64_t>()[0];
    TORCH_CHECK(tail.data_ptr<int64_t>()[1] == 0,
                "sample_hop_device: a target id is outside [0, N)");
  }

  auto colidx_local = torch::empty({ne}, i32);
  auto t_colidx = torch::empty({ne}, i32);
  auto t_eperm = torch::empty({ne}, i32);
  torch::Tensor src_ids, t_rowptr;
  if (ne == 0) {
    src_ids = targets.clone();
    t_rowptr = torch::zeros({n_dst + 1}, i64);
    return {rowptr_s, colidx_local, src_ids, t_rowptr, t_colidx, t_eperm,
            inv_deg};
  }

  auto picked = torch::empty({ne}, i32);
  auto erow = torch::empty({ne}, i32);
  int* pk = picked.data_ptr<int>();
  const int64_t* rps = rowptr_s.data_ptr<int64_t>();
  const unsigned long long useed = (unsigned long long)seed;
  if (fo <= 8) launch_pick<8, 1>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  else if (fo <= 16) launch_pick<8, 2>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  else if (fo <= 32) launch_pick<8, 4>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  else if (fo <= 64) launch_pick<16, 4>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  else if (fo <= 128) launch_pick<32, 4>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  else launch_pick<64, 8>(rp, ci, tg, rps, pk, erow.data_ptr<int>(), n_dst, fo, useed, s);
  ROC_HIP_CHECK(hipGetLastError());

  // From the mark on, the workspace is dirty. If anything below throws
  // before src_ids is complete, every touched node is a target or a picked
  // id, so releasing those two lists restores it.
  bool dirty = true;
  auto release_touched = [&]() {
    hipLaunchKernelGGL((sample_release_kernel<int64_t>), grid_for(n_dst),
                       dim3(kBlock), 0, s, tg, slot_p, first_p, n_dst, N);
    hipLaunchKernelGGL((sample_release_kernel<int>), grid_for(ne),
                       dim3(kBlock), 0, s, (const int*)pk, slot_p, first_p,
                       ne, N);
  };
  try {
    hipLaunchKernelGGL(sample_mark_kernel, grid_for(n_dst), dim3(kBlock), 0,
                       s, tg, slot_p, n_dst, N);
    hipLaunchKernelGGL(sample_claim_kernel, grid_for(ne), dim3(kBlock), 0, s,
                       (const int*)pk, (const int*)slot_p, first_p, ne);
    auto flag = torch::empty({ne}, i32);
    auto rank = torch::empty({ne + 1}, i32);
    hipLaunchKernelGGL(sample_own_kernel, grid_for(ne), dim3(kBlock), 0, s,
                       (const int*)pk, (const int*)slot_p,
                       (const int*)first_p, flag.data_ptr<int>(), ne);
    exclusive_scan<int>(flag.data_ptr<int>(), rank.data_ptr<int>(), ne,
                        torch::kInt32, dev, s);
    ROC_HIP_CHECK(hipGetLastError());
    const int64_t n_src =
        n_dst + (int64_t)rank.narrow(0, ne, 1).cpu().data_ptr<int>()[0];  // host read 2

    src_ids = torch::empty({n_src}, i64);
    auto t_cnt = torch::zeros({n_src}, i32);
    t_rowptr = torch::zeros({n_src + 1}, i64);
    hipLaunchKernelGGL(sample_assign_kernel,
                       grid_for(ne > n_dst ? ne : n_dst), dim3(kBlock), 0, s,
                       (const int*)pk, (const int*)flag.data_ptr<int>(),
                       (const int*)rank.data_ptr<int>(), tg, slot_p,
                       src_ids.data_ptr<int64_t>(), ne, n_dst);
    hipLaunchKernelGGL(sample_relabel_kernel, grid_for(ne), dim3(kBlock), 0,
                       s, (const int*)pk, (const int*)slot_p,
                       colidx_local.data_ptr<int>(), t_cnt.data_ptr<int>(),
                       ne);
    hipLaunchKernelGGL((sample_release_kernel<int64_t>), grid_for(n_src),
                       dim3(kBlock), 0, s,
                       (const int64_t*)src_ids.data_ptr<int64_t>(), slot_p,
                       first_p, n_src, N);
    dirty = false;
    ROC_HIP_CHECK(hipGetLastError());

    exclusive_scan<int64_t>(t_cnt.data_ptr<int>(),
                            t_rowptr.data_ptr<int64_t>(), n_src, torch::kInt64,
                            dev, s);
    auto sorted = torch::sort(colidx_local, /*stable=*/true, 0, false);
    auto perm = std::get<1>(sorted).contiguous();
    hipLaunchKernelGGL(sample_transpose_kernel, grid_for(ne), dim3(kBlock),
                       0, s, (const int64_t*)perm.data_ptr<int64_t>(),
                       (const int*)erow.data_ptr<int>(),
                       t_eperm.data_ptr<int>(), t_colidx.data_ptr<int>(), ne);
    ROC_HIP_CHECK(hipGetLastError());
  } catch (...) {
    if (dirty) release_touched();
    throw;
  }
  return {rowptr_s, colidx_local, src_ids, t_rowptr, t_colidx, t_eperm,
          inv_deg};
}

// out[j, :] = feats[ids[j], :] cast to out's dtype (f32 -> f32 / bf16,
// bf16 -> bf16).
void gather_rows_cast(torch::Tensor out, torch::Tensor feats,
                      torch::Tensor ids) {
  ROC_CHECK_DEV_CONT(out);
  ROC_CHECK_DEV_CONT(feats);
  ROC_CHECK_DEV_CONT(ids);
  TORCH_CHECK(ids.scalar_type() == torch::kInt64 && ids.dim() == 1,
              "gather_rows_cast: ids must be int64 [n]");
  TORCH_CHECK(feats.dim() == 2 && out.dim() == 2 &&
                  out.size(0) == ids.numel() && out.size(1) == feats.size(1),
              "gather_rows_cast: out must be [len(ids), feats.shape[1]]");
  TORCH_CHECK(out.device() == feats.device() && ids.device() == feats.device(),
              "gather_rows_cast: all tensors must share one device");
  const int64_t n = ids.numel(), n_in = feats.size(0);
  const int64_t D64 = feats.size(1);
  TORCH_CHECK(D64 < (1ll << 31) - 512, "gather_rows_cast: row too long");
  const int D = (int)D64;
  if (n == 0 || D == 0) return;
  const bool f_in = feats.scalar_type() == torch::kFloat32;
  const bool f_out = out.scalar_type() == torch::kFloat32;
  TORCH_CHECK((f_in || feats.scalar_type() == torch::kBFloat16) &&
                  (f_out || out.scalar_type() == torch::kBFloat16) &&
                  (f_in || !f_out),
              "gather_rows_cast: f32->f32, f32->bf16 or bf16->bf16 only");
  TORCH_CHECK(((uintptr_t)feats.data_ptr() | (uintptr_t)out.data_ptr()) % 16
                  == 0, "gather_rows_cast: tensors must be 16-B aligned");
  const int items = D % 8 == 0 ? D / 8 : D;  // a row's units of work
  int T = 1;
  while (T < 64 && T < items) T <<= 1;
  const int grid = roc_grid_1d(n * T, kBlock, 1 << 16);
  auto s = roc_stream();
  const int64_t* ip = ids.data_ptr<int64_t>();
  if (f_in && f_out)
    hipLaunchKernelGGL((gather_rows_cast_kernel<float, float>), dim3(grid),
                       dim3(kBlock), 0, s, out.data_ptr<float>(),
                       (const float*)feats.data_ptr<float>(), ip, n, n_in, D,
                       T);
  else if (f_in)
    hipLaunchKernelGGL((gather_rows_cast_kernel<float, unsigned short>),
                       dim3(grid), dim3(kBlock), 0, s,
                       (unsigned short*)out.data_ptr(),
                       (const float*)feats.data_ptr<float>(), ip, n, n_in, D,
                       T);
  else
    hipLaunchKernelGGL(
        (gather_rows_cast_kernel<unsigned short, unsigned short>), dim3(grid),
        dim3(kBlock), 0, s, (unsigned short*)out.data_ptr(),
        (const unsigned short*)feats.data_ptr(), ip, n, n_in, D, T);
  ROC_HIP_CHECK(hipGetLastError());
}
