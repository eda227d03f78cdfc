// hypervolume.h — Monte-Carlo hypervolume of a set of cost vectors inside a box and every member's
// exclusive contribution (mpct_hypervolume_device / mpct_hypervolume, include/mpct.h).
// Kernels in hypervolume.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "hv_points.h"

namespace mpct {

constexpr long long kHvMaxSamples = 1LL << 30;  // MPCT_HV_MAX_SAMPLES
constexpr int kHvTile = 128;                    // T: members per LDS tile [K][T]; 256 is the other instance
constexpr int kHvGridCap = 1 << 20;             // workgroups at most; beyond, they stride over the sample blocks
constexpr int kHvBins = 8;                      // depth_hist: 0, 1, .., 6 and >= 7

// Counting kernel.  Lane = sample point i (its k coordinates in K registers, generated from (seed, i),
// columns k..K-1 padded with +0.0); the members stream through LDS in tiles [K][T], gathered through
// `members` (NULL: entry m is candidate m) and read at a wave-uniform address.  An entry that is -1 or
// outside [0, C) is staged as NaN and covers nothing, as does a row with a NaN cost.  Adds to
// counts[0] the points covered at all, to counts[1 + b] the points of depth bin b, and to excl[m] the
// points that entry m alone covers (excl may be NULL).  The workgroups stride over the blocks of 256 points.
template <int K, int T>
__global__ void __launch_bounds__(kHvBlock)
    hv_count_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                    const double* __restrict__ lo, const double* __restrict__ ref, long long N,
                    unsigned long long seed, unsigned long long* __restrict__ counts,
                    unsigned long long* __restrict__ excl);
// one thread: n_covered, depth_hist and hv from counts (each output may be NULL); hv is NaN for a box
// that is not finite with lo < ref
__global__ void hv_finish_kernel(const unsigned long long* __restrict__ counts, int k, const double* __restrict__ lo,
                                 const double* __restrict__ ref, long long N, long long* __restrict__ n_covered,
                                 long long* __restrict__ depth_hist, double* __restrict__ hv);

struct HvOut {
  long long* n_covered;   // [1]
  long long* excl;        // [M]
  long long* depth_hist;  // [kHvBins]
  double* hv;             // [1]
};

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked.
// tile 0 / max_blocks 0: the defaults (kHvTile, kHvGridCap); tile 128 or 256 and a smaller grid for the tests
// and tools/hv_bench.py
int hypervolume_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                       const double* ref, long long N, unsigned long long seed, const HvOut& out, hipStream_t stream,
                       std::string* err, int tile = 0, int max_blocks = 0);

}  // namespace mpct
