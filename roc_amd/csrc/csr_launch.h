// Host side of the row-team CSR gather frame (spmm.hip, seg_max.hip,
// seg_stats.hip, graph_attn.hip): argument checks, launch geometry, and the lift of
// (team, gather engine) to template constants. docs/KERNELS.md, "The
// row-team gather frame", describes the whole frame.
#pragma once

#include <climits>

#include "row_team.h"

// `what` is the op's name: every message here starts with it.
inline void check_csr(const torch::Tensor& rowptr, const torch::Tensor& colidx,
                      int64_t num_rows, const char* what) {
  ROC_CHECK_DEV_CONT(rowptr);
  ROC_CHECK_DEV_CONT(colidx);
  TORCH_CHECK(rowptr.scalar_type() == torch::kInt64, what,
              ": rowptr must be int64");
  TORCH_CHECK(colidx.scalar_type() == torch::kInt32, what,
              ": colidx must be int32");
  TORCH_CHECK(rowptr.dim() == 1 && rowptr.size(0) == num_rows + 1, what,
              ": rowptr size mismatch");
}

// for the ops whose arg and t_eperm carry edge indices as int32
// (seg_max.hip, seg_stats.hip)
inline void check_csr_i32(const torch::Tensor& rowptr,
                          const torch::Tensor& colidx, int64_t num_rows,
                          const char* what) {
  check_csr(rowptr, colidx, num_rows, what);
  TORCH_CHECK(colidx.numel() < ((int64_t)1 << 31), what,
              ": 2^31 or more edges do not fit the int32 edge index");
}

// a feature matrix: 2-D, and its row count fits the kernels' int
inline void check_mat(const torch::Tensor& t, const char* what,
                      const char* name) {
  ROC_CHECK_DEV_CONT(t);
  TORCH_CHECK(t.dim() == 2, what, ": ", name, " must be 2-D");
  TORCH_CHECK(t.size(0) < INT_MAX, what, ": ", name, " has too many rows");
}

// the row-major matrix of one op and the matrix it gathers from, under the
// names the op gives them: same feature dim
inline void check_mat_pair(const torch::Tensor& a, const char* a_name,
                           const torch::Tensor& b, const char* b_name,
                           const char* what) {
  check_mat(a, what, a_name);
  check_mat(b, what, b_name);
  TORCH_CHECK(a.size(1) == b.size(1), what, ": ", a_name, " and ", b_name,
              " differ in feature dim");
}

inline void check_like(const torch::Tensor& t, const torch::Tensor& ref,
                       const char* what, const char* name) {
  ROC_CHECK_DEV_CONT(t);
  TORCH_CHECK(t.scalar_type() == ref.scalar_type() && t.sizes() == ref.sizes(),
              what, ": ", name, " must have the shape and dtype of its input");
}

// The row visiting order of a launch, or null for the natural sweep. The
// kernels index it with every ri < n, so it is checked here.
// Measured (scripts/bench_spmm.py, Reddit shape): degree-descending
// scheduling wins for wide rows (D=256: -13%) but loses for narrow
// ones (D=48: +10% — the indirection costs more than the skew tail),
// so a team below 16 drops the order.
inline const int* row_order_ptr(const c10::optional<torch::Tensor>& order,
                                int64_t n, int team, const char* what) {
  if (!order.has_value()) return nullptr;
  TORCH_CHECK(order->is_cuda() && order->is_contiguous() &&
                  order->scalar_type() == torch::kInt32 && order->numel() == n,
              what, ": row_order must be a contiguous int32 GPU tensor "
              "[num_rows]");
  return team < 16 ? nullptr : order->data_ptr<int>();
}

// Geometry of one launch: the team by the row's width in 16-B units, the
// grid over rows x column tiles, the gather engine by the byte size of the
// gathered matrix (the buffer engine's 32-bit offsets cover 4 GB).
struct GatherGeom {
  int team;
  dim3 grid;
  bool buf;
  unsigned bytes;  // of the gathered matrix; 0 with the global engine
};

// col_tiles == 0 tiles the units over the team; team_override == 0 picks
// the team by width.
template <typename T>
GatherGeom gather_geom(int num_rows, int64_t units, int col_tiles,
                       size_t gathered_elems, bool allow_buffer = true,
                       int team_override = 0) {
  GatherGeom g;
  g.team = team_override ? team_override : row_team_size(units);
  if (col_tiles == 0) col_tiles = (int)((units + g.team - 1) / g.team);
  g.grid = row_team_grid(num_rows, g.team, col_tiles);
  const size_t b = gathered_elems * sizeof(T);
  g.buf = allow_buffer && b < (size_t)UINT_MAX;
  g.bytes = (unsigned)(g.buf ? b : 0);
  return g;
}

// f receives (team_c, buf_c): std::integral_constant<int, TEAM> and
// std::true_type / std::false_type
template <typename F>
void dispatch_gather(const GatherGeom& g, F&& f) {
  dispatch_team(g.team, [&](auto team_c) {
    dispatch_bool(g.buf, [&](auto buf_c) { f(team_c, buf_c); });
  });
}
