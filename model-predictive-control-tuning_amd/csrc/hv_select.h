// hv_select.h — greedy hypervolume subset selection: the n members that carry a front
// (mpct_hv_select_device / mpct_hv_select, include/mpct.h).  Kernels in hv_select.hip; the
// sample points and the tile staging are hv_points.h's, shared with hypervolume.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "hv_points.h"

namespace mpct {

constexpr int kHvselMaxPicks = 1024;  // MPCT_HVSEL_MAX_PICKS
constexpr int kHvselTile = 128;       // T: members per LDS tile [K][T], hypervolume.hip's default; 256 is the other instance
constexpr int kHvselGridCap = 2048;   // workgroups at most, 8 per CU of 256; 6 to 3 per CU are resident at once (DESIGN §18 resources); they stride over the point blocks

// The record the rounds hand on, in device memory.  The pick kernel of round r writes it, the gain kernel
// of round r + 1 and the finish kernel read it: a kernel boundary lies between every writer and reader.
struct HvselState {
  int done;                          // the largest gain was 0: the selection has ended
  int n_picked;                      // rounds that picked a member
  unsigned long long covered;        // gain[0] + .. + gain[n_picked - 1]
  unsigned long long n_covered_all;  // points covered by any entry (round 0 counts them)
  double row[16];                    // the last pick's costs, columns k .. 15 padded with +0.0
};

// Gain kernel, one launch per round.  Lane = sample point i, generated in registers; wave w of point block
// blk owns word 4 blk + w of `alive` (bit l: point 256 blk + 64 w + l is still uncovered), reads it at a
// wave-uniform address and writes it back from lane 0.  Round 0 starts from "every point below N", counts
// the points any entry covers into st->n_covered_all and clears the others; round r > 0 first clears the
// points st->row covers.  Then gains[m] += the live points entry m covers.  Leaves at once when st->done.
template <int K, int T>
__global__ void __launch_bounds__(kHvBlock)
    hvsel_gain_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                      const double* __restrict__ lo, const double* __restrict__ ref, long long N,
                      unsigned long long seed, int round, unsigned long long* __restrict__ alive,
                      unsigned long long* __restrict__ gains, HvselState* __restrict__ st);

struct HvSelOut {
  long long* n_picked;       // [1]
  int* pos;                  // [n_pick]
  int* index;                // [n_pick]
  long long* gain;           // [n_pick]
  long long* covered;        // [n_pick]
  double* hv;                // [n_pick]
  int* ties;                 // [n_pick]
  long long* n_covered_all;  // [1]
};

// Pick kernel, one workgroup per round: argmax of gains[M] on (gain descending, m ascending) and the number
// of entries that hold the maximum, in integers; writes slot `round` of the outputs, the picked row and the
// running totals into *st, sets st->done when the maximum is 0, and zeroes gains for the next round.
__global__ void __launch_bounds__(kHvBlock)
    hvsel_pick_kernel(const double* __restrict__ costs, int k, const int* __restrict__ members, int M,
                      const double* __restrict__ lo, const double* __restrict__ ref, long long N, int round,
                      unsigned long long* __restrict__ gains, HvselState* __restrict__ st, HvSelOut out);
// after the last round: n_picked, n_covered_all and the end-of-selection fill of the slots n_picked .. n_pick - 1
__global__ void __launch_bounds__(kHvBlock)
    hvsel_finish_kernel(int k, const double* __restrict__ lo, const double* __restrict__ ref, long long N, int n_pick,
                        const HvselState* __restrict__ st, HvSelOut out);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked.
// tile 0 / max_blocks 0: the defaults (kHvselTile, kHvselGridCap).  round_ms (host, [n_pick]; NULL: off) is
// the tools' mode: events round every round, and the call then waits for the stream to read them.
int hv_select_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                     const double* ref, long long N, unsigned long long seed, int n_pick, const HvSelOut& out,
                     hipStream_t stream, std::string* err, int tile = 0, int max_blocks = 0, float* round_ms = nullptr);

}  // namespace mpct
