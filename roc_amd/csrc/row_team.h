// Row-team frame shared by the CSR kernels (spmm.hip, seg_max.hip,
// seg_stats.hip, graph_attn.hip, edge_softmax.hip) and by the row kernels of
// layer_norm.hip. gather.h adds the device side of the feature-row
// gathers, csr_launch.h the host side of their launches.
//
// A team of TEAM contiguous lanes (a power of two <= 64, so a team never
// straddles a wave64) owns one CSR row at a time; teams grid-stride over
// the rows. The shfl_xor trees below therefore never cross a team.
#pragma once

#include <type_traits>

#include "common.h"

template <int TEAM>
struct RowTeam {
  int team;    // global team index = first row this team visits
  int lane;    // lane within the team
  int nteams;  // row stride
  __device__ __forceinline__ RowTeam()
      : team(blockIdx.x * (kBlock / TEAM) + (int)threadIdx.x / TEAM),
        lane((int)threadIdx.x % TEAM),
        nteams(gridDim.x * (kBlock / TEAM)) {}
};

template <int TEAM>
__device__ __forceinline__ float team_reduce_sum(float v) {
#pragma unroll
  for (int off = TEAM / 2; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
  return v;
}

template <int TEAM>
__device__ __forceinline__ float team_reduce_max(float v) {
#pragma unroll
  for (int off = TEAM / 2; off > 0; off >>= 1)
    v = fmaxf(v, __shfl_xor(v, off, 64));
  return v;
}

// smallest team in {8,16,32,64} that covers `units` 16-B units per row
inline int row_team_size(int64_t units) {
  int team = 8;
  while (team < units && team < 64) team *= 2;
  return team;
}

inline dim3 row_team_grid(int num_rows, int team, int col_tiles = 1) {
  return dim3(roc_grid_1d(num_rows, kBlock / team, 8192), col_tiles);
}

// runtime -> compile-time dispatch: f receives a std::integral_constant
template <typename F>
void dispatch_team(int team, F&& f) {
  switch (team) {
    case 8:  f(std::integral_constant<int, 8>{});  break;
    case 16: f(std::integral_constant<int, 16>{}); break;
    case 32: f(std::integral_constant<int, 32>{}); break;
    default: f(std::integral_constant<int, 64>{});
  }
}
