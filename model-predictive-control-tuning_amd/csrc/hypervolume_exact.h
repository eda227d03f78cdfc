// hypervolume_exact.h — exact hypervolume of a set of cost vectors inside a box and every member's
// exclusive contribution, for at most three objectives (mpct_hypervolume_exact_device /
// mpct_hypervolume_exact, include/mpct.h).  Kernels in hypervolume_exact.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr int kHvxMaxObj = 3;     // MPCT_HVX_MAX_OBJ
constexpr int kHvxMaxM = 65536;   // MPCT_HVX_MAX_M
constexpr int kHvxGroups = 256;   // G: slab groups, one wave each; a constant of the design (it fixes the summation order)
constexpr int kHvxBlock = 256;    // threads of a workgroup of the stage, rank and finish kernels

// Entry m gathered through `members` (NULL: entry m is candidate m), clipped to the box and padded to
// three axes (a missing axis is lo = 0, ref = 1, coordinate 0): b[0][m], b[1][m], b[2][m].  An inactive
// entry (-1, outside [0, C), a NaN cost, a clipped coordinate on or past ref, or a bad box) is +INF in
// every axis.  -0.0 is stored as +0.0.
__global__ void __launch_bounds__(kHvxBlock)
    hvx_stage_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                     const double* __restrict__ lo, const double* __restrict__ ref, double* __restrict__ b);
// Ranks by counting: the position of every active entry in the order (x, y, z, m) and in the order
// (z, x, y, m), both total, so the sorted sequences are a function of the clipped vectors alone.  Writes
// the x values, the y values, the entry and its z rank in x order, the z values in z order, and n.
__global__ void __launch_bounds__(kHvxBlock)
    hvx_rank_kernel(const double* __restrict__ b, int M, double* __restrict__ xs, double* __restrict__ yx,
                    double* __restrict__ zs, int* __restrict__ idx, int* __restrict__ zrx, int* __restrict__ nact);
// The sweep: workgroup g (one wave) walks the slabs s = g, g + G, .. in ascending order, each over the
// columns in x order in chunks of 64, and adds into phv[g] and, where pe is not NULL, pe[g][M].
__global__ void __launch_bounds__(64)
    hvx_sweep_kernel(const double* __restrict__ xs, const double* __restrict__ yx, const double* __restrict__ zs,
                     const int* __restrict__ idx, const int* __restrict__ zrx, const int* __restrict__ nact, int k,
                     const double* __restrict__ lo, const double* __restrict__ ref, int M, double* __restrict__ phv,
                     double* __restrict__ pe);
// The sums over g in ascending order; NaN for a bad box.  Each output may be NULL.
__global__ void __launch_bounds__(kHvxBlock)
    hvx_finish_kernel(const double* __restrict__ phv, const double* __restrict__ pe, const int* __restrict__ nact, int k,
                      const double* __restrict__ lo, const double* __restrict__ ref, int M, double* __restrict__ hv,
                      double* __restrict__ excl, long long* __restrict__ n_active);

struct HvxOut {
  double* hv;           // [1]
  double* excl;         // [M]
  long long* n_active;  // [1]
};

// bytes of scratch of one call (hipMallocAsync on the call's stream)
size_t hvx_scratch_bytes(long long M, bool want_excl);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked, M >= 1.
int hypervolume_exact_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                             const double* ref, const HvxOut& out, hipStream_t stream, std::string* err);

}  // namespace mpct
