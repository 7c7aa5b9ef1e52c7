// Native graph machinery (CPU, OpenMP): CSR transpose, row sorting,
// degree counting. Replaces the numpy paths for the 10^8-edge graphs
// (counting sort is O(E) vs argsort's O(E log E)); the reference's
// equivalents are the C++ loader/partition code in `gnn.cc:751-872`.
#include <torch/extension.h>

#include <atomic>
#include <cstdint>
#include <cstring>
#include <unordered_map>
#include <vector>

#ifdef _OPENMP
#include <omp.h>
#endif

// transpose of a (possibly rectangular) CSR: rows -> num_cols rows.
std::vector<torch::Tensor> csr_transpose(int64_t num_cols,
                                         torch::Tensor rowptr,
                                         torch::Tensor colidx) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu());
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64);
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32);
  rowptr = rowptr.contiguous();
  colidx = colidx.contiguous();
  const int64_t nr = rowptr.numel() - 1;
  const int64_t ne = colidx.numel();
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();

  auto t_rowptr = torch::zeros({num_cols + 1}, torch::kInt64);
  auto t_colidx = torch::empty({ne}, torch::kInt32);
  int64_t* trp = t_rowptr.data_ptr<int64_t>();
  int* tci = t_colidx.data_ptr<int>();

  // 1) count in-degree of each column
  {
    std::vector<std::atomic<int64_t>> cnt(num_cols);
    for (int64_t i = 0; i < num_cols; ++i)
      cnt[i].store(0, std::memory_order_relaxed);
#pragma omp parallel for schedule(static)
    for (int64_t e = 0; e < ne; ++e)
      cnt[ci[e]].fetch_add(1, std::memory_order_relaxed);
    int64_t run = 0;
    for (int64_t c = 0; c < num_cols; ++c) {
      trp[c] = run;
      run += cnt[c].load(std::memory_order_relaxed);
    }
    trp[num_cols] = run;
  }
  // 2) scatter destinations. Serial pass: keeps the result DETERMINISTIC
  //    (stable by source row within each column), which keeps reduction
  //    order — and therefore training — reproducible across runs.
  {
    std::vector<int64_t> cursor(num_cols);
    std::memcpy(cursor.data(), trp, num_cols * sizeof(int64_t));
    for (int64_t v = 0; v < nr; ++v) {
      for (int64_t e = rp[v]; e < rp[v + 1]; ++e)
        tci[cursor[ci[e]]++] = (int)v;
    }
  }
  return {t_rowptr, t_colidx};
}

// Reverse Cuthill-McKee ordering on the symmetrized adjacency (in-CSR +
// its transpose, both passed in so the O(E) counting-sort transpose is
// reused). Classic RCM: BFS from a minimum-degree seed per component,
// neighbors enqueued degree-ascending, final order reversed. Returns an
// int64 permutation for `reorder_graph` (a locality preprocessing the
// reference lacks; its partitioner `gnn.cc:806-829` cuts contiguous
// ranges of whatever order the dataset shipped).
torch::Tensor rcm_order(torch::Tensor rowptr, torch::Tensor colidx,
                        torch::Tensor t_rowptr, torch::Tensor t_colidx) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu());
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64);
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32);
  rowptr = rowptr.contiguous();
  colidx = colidx.contiguous();
  t_rowptr = t_rowptr.contiguous();
  t_colidx = t_colidx.contiguous();
  const int64_t n = rowptr.numel() - 1;
  TORCH_CHECK(t_rowptr.numel() - 1 == n, "transpose must be square");
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();
  const int64_t* trp = t_rowptr.data_ptr<int64_t>();
  const int* tci = t_colidx.data_ptr<int>();

  std::vector<int64_t> deg(n);
#pragma omp parallel for schedule(static)
  for (int64_t v = 0; v < n; ++v)
    deg[v] = (rp[v + 1] - rp[v]) + (trp[v + 1] - trp[v]);

  // seeds: degree-ascending so each component starts at a pseudo-peripheral
  // low-degree vertex (counting sort — degrees are bounded by 2E)
  std::vector<int64_t> seeds(n);
  {
    std::vector<int64_t> idx(n);
    for (int64_t v = 0; v < n; ++v) idx[v] = v;
    std::stable_sort(idx.begin(), idx.end(),
                     [&](int64_t a, int64_t b) { return deg[a] < deg[b]; });
    seeds.swap(idx);
  }

  auto out = torch::empty({n}, torch::kInt64);
  int64_t* order = out.data_ptr<int64_t>();  // doubles as the BFS queue
  std::vector<uint8_t> visited(n, 0);
  std::vector<int64_t> nbr;
  int64_t head = 0, tail = 0;
  size_t seed_i = 0;
  while (tail < n) {
    while (seed_i < seeds.size() && visited[seeds[seed_i]]) ++seed_i;
    const int64_t s = seeds[seed_i];
    visited[s] = 1;
    order[tail++] = s;
    while (head < tail) {
      const int64_t v = order[head++];
      nbr.clear();
      for (int64_t e = rp[v]; e < rp[v + 1]; ++e) {
        const int64_t u = ci[e];
        if (!visited[u]) { visited[u] = 1; nbr.push_back(u); }
      }
      for (int64_t e = trp[v]; e < trp[v + 1]; ++e) {
        const int64_t u = tci[e];
        if (!visited[u]) { visited[u] = 1; nbr.push_back(u); }
      }
      std::sort(nbr.begin(), nbr.end(),
                [&](int64_t a, int64_t b) {
                  return deg[a] != deg[b] ? deg[a] < deg[b] : a < b;
                });
      for (const int64_t u : nbr) order[tail++] = u;
    }
  }
  std::reverse(order, order + n);
  return out;
}

// Label-propagation clustering order: T synchronous rounds where each
// vertex adopts the most frequent label among its in-neighbors (the CSR
// row, which includes the self-edge), then a stable sort by final
// label. On community-structured graphs this packs each community
// contiguously — far better gather locality than RCM, whose BFS fronts
// explode through the long-range edges. In-edges-only measurably beats
// symmetrized counting here (hub out-fans otherwise smear labels).
// Deterministic: ties break toward the smaller label.
torch::Tensor lp_cluster_order(torch::Tensor rowptr, torch::Tensor colidx,
                               int64_t iters) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu());
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64);
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32);
  rowptr = rowptr.contiguous();
  colidx = colidx.contiguous();
  const int64_t n = rowptr.numel() - 1;
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();

  std::vector<int64_t> lab(n), next(n);
  for (int64_t v = 0; v < n; ++v) lab[v] = v;
  std::atomic<int64_t> changed{0};
  for (int64_t it = 0; it < iters; ++it) {
    changed.store(0, std::memory_order_relaxed);
#pragma omp parallel
    {
      std::vector<int64_t> buf;
#pragma omp for schedule(dynamic, 2048)
      for (int64_t v = 0; v < n; ++v) {
        buf.clear();
        for (int64_t e = rp[v]; e < rp[v + 1]; ++e) buf.push_back(lab[ci[e]]);
        if (buf.empty()) { next[v] = lab[v]; continue; }
        std::sort(buf.begin(), buf.end());
        int64_t best = buf[0], best_cnt = 1, cur = buf[0], cur_cnt = 1;
        for (size_t i = 1; i < buf.size(); ++i) {
          if (buf[i] == cur) {
            ++cur_cnt;
          } else {
            if (cur_cnt > best_cnt) { best = cur; best_cnt = cur_cnt; }
            cur = buf[i];
            cur_cnt = 1;
          }
        }
        if (cur_cnt > best_cnt) { best = cur; best_cnt = cur_cnt; }
        next[v] = best;
        if (best != lab[v]) changed.fetch_add(1, std::memory_order_relaxed);
      }
    }
    lab.swap(next);
    // converged-enough: a vanishing tail of flips no longer moves the
    // ordering (matters at 10^9-edge scale where each round is minutes)
    if (changed.load(std::memory_order_relaxed) <= n / 4096) break;
  }

  auto out = torch::empty({n}, torch::kInt64);
  int64_t* order = out.data_ptr<int64_t>();
  for (int64_t v = 0; v < n; ++v) order[v] = v;
  std::stable_sort(order, order + n,
                   [&](int64_t a, int64_t b) { return lab[a] < lab[b]; });
  return out;
}

// Relabel a CSR by a permutation (new_id = position of old_id in perm):
// rows permuted, columns rewritten through the inverse map, columns
// sorted within each row. O(E), OpenMP over destination rows, no
// edge-sized temporaries beyond the output — the numpy path in
// graph.py allocates ~3 edge-sized int64 transients, which matters at
// 10^9 edges (the offline reorder_dataset.py use case).
std::vector<torch::Tensor> csr_permute(torch::Tensor rowptr,
                                       torch::Tensor colidx,
                                       torch::Tensor perm) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu() &&
              perm.device().is_cpu());
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64);
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32);
  TORCH_CHECK(perm.scalar_type() == torch::kInt64);
  rowptr = rowptr.contiguous();
  colidx = colidx.contiguous();
  perm = perm.contiguous();
  const int64_t n = rowptr.numel() - 1;
  TORCH_CHECK(perm.numel() == n, "perm must have one entry per node");
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();
  const int64_t* pm = perm.data_ptr<int64_t>();

  std::vector<int64_t> inv(n);
  for (int64_t i = 0; i < n; ++i) {
    TORCH_CHECK(pm[i] >= 0 && pm[i] < n, "perm out of range");
    inv[pm[i]] = i;
  }
  auto new_rowptr = torch::empty({n + 1}, torch::kInt64);
  int64_t* nrp = new_rowptr.data_ptr<int64_t>();
  nrp[0] = 0;
  for (int64_t v = 0; v < n; ++v) {
    const int64_t old_v = pm[v];
    nrp[v + 1] = nrp[v] + (rp[old_v + 1] - rp[old_v]);
  }
  const int64_t ne = nrp[n];
  TORCH_CHECK(ne == colidx.numel());
  auto new_colidx = torch::empty({ne}, torch::kInt32);
  int* nci = new_colidx.data_ptr<int>();
#pragma omp parallel for schedule(dynamic, 1024)
  for (int64_t v = 0; v < n; ++v) {
    const int64_t old_v = pm[v];
    int64_t w = nrp[v];
    for (int64_t e = rp[old_v]; e < rp[old_v + 1]; ++e)
      nci[w++] = (int)inv[ci[e]];
    std::sort(nci + nrp[v], nci + w);
  }
  return {new_rowptr, new_colidx};
}

// sort column ids within each row (in place)
void csr_sort_rows(torch::Tensor rowptr, torch::Tensor colidx) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu());
  const int64_t nr = rowptr.numel() - 1;
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  int* ci = colidx.data_ptr<int>();
#pragma omp parallel for schedule(dynamic, 1024)
  for (int64_t v = 0; v < nr; ++v) std::sort(ci + rp[v], ci + rp[v + 1]);
}


// ---------------------------------------------------------------------------
// Neighbor sampling (one hop of the mini-batch tier, roc_amd/sampling.py).
// For each target row: keep min(fanout, deg) DISTINCT in-neighbor edges
// (without replacement, Floyd's algorithm, per-row splitmix64 stream so
// the result is deterministic in (seed, node) and independent of thread
// schedule). Sources get local ids with the targets occupying [0, n_dst).
// Returns {rowptr_s int64[n_dst+1], colidx_local int32[E_s],
//          src_ids int64[n_src]}.
// ---------------------------------------------------------------------------

static inline uint64_t splitmix64(uint64_t x) {
  x += 0x9e3779b97f4a7c15ull;
  x = (x ^ (x >> 30)) * 0xbf58476d1ce4e5b9ull;
  x = (x ^ (x >> 27)) * 0x94d049bb133111ebull;
  return x ^ (x >> 31);
}

std::vector<torch::Tensor> sample_hop(torch::Tensor rowptr,
                                      torch::Tensor colidx,
                                      torch::Tensor targets, int64_t fanout,
                                      int64_t seed) {
  TORCH_CHECK(rowptr.device().is_cpu() && colidx.device().is_cpu() &&
              targets.device().is_cpu());
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64);
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32);
  TORCH_CHECK(targets.scalar_type() == torch::kInt64);
  TORCH_CHECK(fanout > 0, "fanout must be positive");
  rowptr = rowptr.contiguous();
  colidx = colidx.contiguous();
  targets = targets.contiguous();
  const int64_t* rp = rowptr.data_ptr<int64_t>();
  const int* ci = colidx.data_ptr<int>();
  const int64_t* tg = targets.data_ptr<int64_t>();
  const int64_t n_dst = targets.numel();

  auto rowptr_s = torch::zeros({n_dst + 1}, torch::kInt64);
  int64_t* rps = rowptr_s.data_ptr<int64_t>();
  // phase 1 (parallel): pick GLOBAL neighbor ids into a padded buffer
  std::vector<int> picked((size_t)n_dst * fanout);
#pragma omp parallel for schedule(dynamic, 256)
  for (int64_t i = 0; i < n_dst; ++i) {
    const int64_t v = tg[i];
    const int64_t lo = rp[v], deg = rp[v + 1] - lo;
    int* out = picked.data() + (size_t)i * fanout;
    if (deg <= fanout) {
      for (int64_t e = 0; e < deg; ++e) out[e] = ci[lo + e];
      rps[i + 1] = deg;
    } else {
      // Floyd: k distinct offsets in [0, deg)
      int64_t sel[512];  // fanout is clamped to <= 512 by the wrapper
      int k = 0;
      uint64_t st = splitmix64(((uint64_t)seed << 20) ^ (uint64_t)v);
      for (int64_t j = deg - fanout; j < deg; ++j) {
        st = splitmix64(st);
        int64_t t = (int64_t)(st % (uint64_t)(j + 1));
        bool seen = false;
        for (int q = 0; q < k; ++q)
          if (sel[q] == t) { seen = true; break; }
        sel[k++] = seen ? j : t;
      }
      for (int q = 0; q < k; ++q) out[q] = ci[lo + sel[q]];
      rps[i + 1] = fanout;
    }
  }
  for (int64_t i = 0; i < n_dst; ++i) rps[i + 1] += rps[i];
  const int64_t ne = rps[n_dst];

  // phase 2 (serial, deterministic): local-id mapping, targets first
  auto colidx_local = torch::empty({ne}, torch::kInt32);
  int* cl = colidx_local.data_ptr<int>();
  std::unordered_map<int64_t, int> local;
  local.reserve((size_t)(n_dst + ne));
  std::vector<int64_t> src_ids_v(tg, tg + n_dst);
  src_ids_v.reserve((size_t)(n_dst + ne));
  for (int64_t i = 0; i < n_dst; ++i) local.emplace(tg[i], (int)i);
  for (int64_t i = 0; i < n_dst; ++i) {
    const int* out = picked.data() + (size_t)i * fanout;
    const int64_t cnt = rps[i + 1] - rps[i];
    for (int64_t q = 0; q < cnt; ++q) {
      const int64_t u = out[q];
      auto it = local.find(u);
      int j;
      if (it == local.end()) {
        j = (int)src_ids_v.size();
        local.emplace(u, j);
        src_ids_v.push_back(u);
      } else {
        j = it->second;
      }
      cl[rps[i] + q] = j;
    }
  }
  auto src_ids = torch::empty({(int64_t)src_ids_v.size()}, torch::kInt64);
  std::memcpy(src_ids.data_ptr<int64_t>(), src_ids_v.data(),
              src_ids_v.size() * sizeof(int64_t));
  return {rowptr_s, colidx_local, src_ids};
}

void register_graph_cpu(pybind11::module_& m) {
  m.def("csr_transpose", &csr_transpose,
        "counting-sort CSR transpose (CPU, OpenMP)");
  m.def("csr_sort_rows", &csr_sort_rows, "sort column ids within rows");
  m.def("rcm_order", &rcm_order,
        "reverse Cuthill-McKee permutation over CSR + transpose");
  m.def("lp_cluster_order", &lp_cluster_order,
        "label-propagation clustering permutation (OpenMP)");
  m.def("csr_permute", &csr_permute,
        "relabel CSR by a permutation (rows + columns, sorted)");
  m.def("sample_hop", &sample_hop,
        "one neighbor-sampling hop (distinct, deterministic, OpenMP)");
}
