// hypervolume.hip — Monte-Carlo hypervolume of M cost vectors inside a box and every member's exclusive
// contribution (see hypervolume.h, include/mpct.h).
//
// N sample points x M members x k column tests, all integer results: pareto_count_kernel with the roles
// swapped.  A lane owns one sample point, generated in registers from (seed, i) by the counter-based
// generator of the contract; the members stream through LDS as [K][T] tiles that every lane reads at the
// same address (a broadcast: no bank conflict).  Per member a:
//   le = AND_j (a_j <= p_j),  depth += le,  last = le ? m : last.
// A NaN in a makes le false, so a skipped entry (-1, or outside [0, C)) is staged as NaN and the inner
// loop has no branch; a lane past N holds a NaN point, is covered by nothing and is left out of every
// count.  The member range is never split: the same lane sees all M members, so depth == 1 names its one
// covering entry in `last`.  The counts meet in integer atomic adds (order-independent, so a repeated
// call is bitwise identical and the launch geometry does not matter).  Every loop bound is a function of
// N, M, k and the grid; nothing waits on another workgroup.
//
// Every product is rounded before it is added: contraction is off for this unit (the pragma below and the
// unit's flags, __graft_entry__.UNIT_FLAGS), so the sample points are restatable in numpy bit for bit.  The
// point generation and the tile staging are hv_points.h's, shared with hv_select.hip.
#include "hypervolume.h"

#pragma clang fp contract(off)

namespace mpct {

template <int K, int T>
__global__ void __launch_bounds__(kHvBlock)
    hv_count_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                    const double* __restrict__ lo, const double* __restrict__ ref, long long N,
                    unsigned long long seed, unsigned long long* __restrict__ counts,
                    unsigned long long* __restrict__ excl) {
  __shared__ __attribute__((aligned(16))) double sA[K * T];
  const int tid = threadIdx.x;
  hv_tile_pad<K, T>(sA, k, tid);
  unsigned long long h[kHvBins];  // this wave's points per depth bin: the same value in every lane
#pragma unroll
  for (int b = 0; b < kHvBins; ++b) h[b] = 0;
  const long long nblocks = (N + kHvBlock - 1) / kHvBlock;
  for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long long i = blk * kHvBlock + tid;
    const bool active = i < N;
    double p[K];
    hv_point<K>(p, k, lo, ref, seed, i, active);
    int depth = 0, last = 0;
    for (int t0 = 0; t0 < M; t0 += T) {
      hv_stage_tile<T>(sA, costs, C, k, members, M, t0, tid);
      __syncthreads();
#pragma unroll 4
      for (int t = 0; t < T; ++t) {
        bool le = true;
#pragma unroll
        for (int j = 0; j < K; ++j) le &= sA[j * T + t] <= p[j];
        depth += le ? 1 : 0;
        last = le ? t0 + t : last;
      }
      __syncthreads();
    }
    if (excl && active && depth == 1) atomicAdd(&excl[last], 1ull);
    const int bin = depth < kHvBins - 1 ? depth : kHvBins - 1;
#pragma unroll
    for (int b = 0; b < kHvBins; ++b) h[b] += (unsigned long long)__popcll(__ballot(active && bin == b));
  }
  if ((tid & 63) == 0) {
    unsigned long long covered = 0;
#pragma unroll
    for (int b = 0; b < kHvBins; ++b) {
      if (b) covered += h[b];
      if (h[b]) atomicAdd(&counts[1 + b], h[b]);
    }
    if (covered) atomicAdd(&counts[0], covered);
  }
}

__global__ void hv_finish_kernel(const unsigned long long* __restrict__ counts, int k, const double* __restrict__ lo,
                                 const double* __restrict__ ref, long long N, long long* __restrict__ n_covered,
                                 long long* __restrict__ depth_hist, double* __restrict__ hv) {
  if (blockIdx.x != 0 || threadIdx.x != 0) return;
  if (n_covered) n_covered[0] = (long long)counts[0];
  if (depth_hist)
    for (int b = 0; b < kHvBins; ++b) depth_hist[b] = (long long)counts[1 + b];
  if (hv) {
    bool box = true;
    const double vol = hv_box_volume(k, lo, ref, &box);
    hv[0] = box ? ((double)counts[0] / (double)N) * vol : __longlong_as_double(0x7ff8000000000000ll);
  }
}

template <int T>
static void launch_count(int K, unsigned grid, hipStream_t stream, const double* costs, int C, int k, const int* members,
                         int M, const double* lo, const double* ref, long long N, unsigned long long seed,
                         unsigned long long* counts, unsigned long long* excl) {
  const dim3 g(grid), blk(kHvBlock);
  switch (K) {
    case 2: hipLaunchKernelGGL((hv_count_kernel<2, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, counts, excl); break;
    case 4: hipLaunchKernelGGL((hv_count_kernel<4, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, counts, excl); break;
    case 8: hipLaunchKernelGGL((hv_count_kernel<8, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, counts, excl); break;
    default: hipLaunchKernelGGL((hv_count_kernel<16, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, counts, excl); break;
  }
}

int hypervolume_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                       const double* ref, long long N, unsigned long long seed, const HvOut& out, hipStream_t stream,
                       std::string* err, int tile, int max_blocks) {
  if (tile != 128 && tile != 256) tile = kHvTile;
  const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
  const long long nblocks = (N + kHvBlock - 1) / kHvBlock;
  const long long cap = max_blocks > 0 && max_blocks < kHvGridCap ? max_blocks : kHvGridCap;
  const unsigned grid = (unsigned)(nblocks < cap ? nblocks : cap);
  unsigned long long* counts = nullptr;  // [0] covered, [1 .. 8] the depth bins
  const size_t bytes = (1 + kHvBins) * sizeof(unsigned long long);
  if (hipMallocAsync(reinterpret_cast<void**>(&counts), bytes, stream) != hipSuccess) {
    *err = "hipMallocAsync failed (hypervolume counts)";
    return -2;
  }
  int rc = 0;
  do {
    if (hipMemsetAsync(counts, 0, bytes, stream) != hipSuccess ||
        (out.excl && M > 0 && hipMemsetAsync(out.excl, 0, (size_t)M * sizeof(long long), stream) != hipSuccess)) {
      *err = "hipMemsetAsync failed (hypervolume counts)";
      rc = -3;
      break;
    }
    unsigned long long* excl = reinterpret_cast<unsigned long long*>(out.excl);
    if (tile == 128)
      launch_count<128>(K, grid, stream, costs, (int)C, k, members, (int)M, lo, ref, N, seed, counts, excl);
    else
      launch_count<256>(K, grid, stream, costs, (int)C, k, members, (int)M, lo, ref, N, seed, counts, excl);
    if (hipGetLastError() != hipSuccess) {
      *err = "hv_count_kernel launch failed";
      rc = -3;
      break;
    }
    if (out.n_covered || out.depth_hist || out.hv) {
      hipLaunchKernelGGL(hv_finish_kernel, dim3(1), dim3(1), 0, stream, (const unsigned long long*)counts, k, lo, ref, N,
                         out.n_covered, out.depth_hist, out.hv);
      if (hipGetLastError() != hipSuccess) {
        *err = "hv_finish_kernel launch failed";
        rc = -3;
      }
    }
  } while (false);
  (void)hipFreeAsync(counts, stream);
  return rc;
}

}  // namespace mpct
