// pareto.h — Pareto front, domination counts and non-dominated-sorting layers of a scored grid
// (mpct_pareto_device / mpct_pareto, include/mpct.h).  Kernels in pareto.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr int kParetoMaxObj = 16;          // MPCT_PARETO_MAX_OBJ
constexpr long long kParetoMaxC = 1 << 20; // MPCT_PARETO_MAX_C
constexpr int kParetoMaxLayers = 64;       // MPCT_PARETO_MAX_LAYERS
constexpr int kParetoBlock = 256;          // threads of a workgroup: one dominated candidate b per lane
constexpr int kParetoTile = 256;           // T: competitors a per LDS tile [K][T]
constexpr int kParetoTargetBlocks = 8192;  // the a-range is split until the grid holds about this many workgroups
constexpr int kParetoUnassigned = 0x7fffffff;  // layer sentinel: valid, no layer yet (INT_MAX)

// Counting kernel.  Lane = candidate b (its k costs in K registers, columns k..K-1 padded with +0.0),
// blockIdx.y = one chunk of `chunk` competitors a, staged tile by tile into LDS as [K][T] and read at a
// wave-uniform address.  Adds to cnt[b] the number of a in the chunk with lay[a] >= pass that dominate
// b, for every b with lay[b] == kParetoUnassigned.  Leaves at once when *remaining == 0.
template <int K, int T>
__global__ void __launch_bounds__(kParetoBlock) pareto_count_kernel(const double* __restrict__ costs, int C, int k, int chunk, int pass,
                                    const int* __restrict__ lay, const int* __restrict__ remaining,
                                    int* __restrict__ cnt);
// lay[c] <- kParetoUnassigned (no NaN among the k costs) or -1; cnt[c] <- 0; *remaining += valid rows
__global__ void __launch_bounds__(kParetoBlock) pareto_init_kernel(const double* __restrict__ costs, int C, int k, int* __restrict__ lay,
                                   int* __restrict__ cnt, int* __restrict__ remaining);
// after pass `pass`: an unassigned c with cnt[c] == 0 gets lay[c] = pass; pass 0 keeps cnt as domc;
// cnt[c] <- 0; *remaining -= newly assigned
__global__ void __launch_bounds__(kParetoBlock) pareto_assign_kernel(int C, int pass, int* __restrict__ lay, int* __restrict__ cnt,
                                     int* __restrict__ domc, int* __restrict__ remaining);
// dom_count / layer in the contract's encoding (-1 invalid, max_layers = beyond); flag[c] = on the front
__global__ void __launch_bounds__(kParetoBlock) pareto_finish_kernel(int C, int max_layers, const int* __restrict__ lay,
                                     const int* __restrict__ domc, int* __restrict__ dom_count,
                                     int* __restrict__ layer, int* __restrict__ flag);
// pos = exclusive prefix sum of flag[0..C]: front[pos[c]] = c where flagged, -1 from pos[C] on
__global__ void __launch_bounds__(kParetoBlock) pareto_front_kernel(int C, const int* __restrict__ flag, const int* __restrict__ pos,
                                    int* __restrict__ front, int* __restrict__ n_front);

struct ParetoOut {
  int* dom_count;
  int* layer;
  int* front;
  int* n_front;
};

// workgroups along the a-range (grid.y) and competitors per chunk (a multiple of the tile) for C
// candidates; split_override > 0 forces the requested number of chunks (some may then be empty)
void pareto_grid(long long C, int tile, int split_override, int* split, int* chunk);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked.
// tile 0 / split 0: the defaults (kParetoTile, pareto_grid); others for the A/B of tools/pareto_bench.py
int pareto_device(const double* costs, long long C, int k, int max_layers, const ParetoOut& out, hipStream_t stream,
                  std::string* err, int tile = 0, int split = 0);

}  // namespace mpct
