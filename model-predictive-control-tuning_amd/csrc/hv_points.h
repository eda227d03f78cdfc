// hv_points.h — what hypervolume.hip and hv_select.hip share: the counter-based sample points of the
// hypervolume contract (include/mpct.h) and the staging of a tile of members into LDS as [K][T].  Inline
// device functions; a unit that includes this is built without contraction (its flags in
// __graft_entry__.UNIT_FLAGS and the pragma below), so the points are restatable in numpy bit for bit.
#pragma once
#include <hip/hip_runtime.h>

#pragma clang fp contract(off)

namespace mpct {

constexpr int kHvBlock = 256;  // threads of a workgroup: one sample point per lane

// coordinate j of sample point i in [0, 1): splitmix64's finaliser over the counter 16 i + j + 1
__device__ __forceinline__ double hv_unit(unsigned long long seed, unsigned long long i, int j) {
  unsigned long long x = seed + 0x9E3779B97F4A7C15ull * (16ull * i + (unsigned long long)j + 1ull);
  x ^= x >> 30;
  x *= 0xBF58476D1CE4E5B9ull;
  x ^= x >> 27;
  x *= 0x94D049BB133111EBull;
  x ^= x >> 31;
  return (double)(x >> 11) * 0x1.0p-53;
}

// sample point i in K registers: columns k .. K-1 padded with +0.0; a lane that is not `active` (past N)
// holds NaN, which nothing covers
template <int K>
__device__ __forceinline__ void hv_point(double (&p)[K], int k, const double* __restrict__ lo,
                                         const double* __restrict__ ref, unsigned long long seed, long long i,
                                         bool active) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
#pragma unroll
  for (int j = 0; j < K; ++j) {
    p[j] = 0.0;
    if (j < k) {
      const double w = ref[j] - lo[j];
      const double s = hv_unit(seed, (unsigned long long)i, j) * w;
      p[j] = active ? lo[j] + s : nan;
    }
  }
}

// the padded columns k .. K-1 of the tile, once per kernel: +0.0 <= every padded point coordinate
template <int K, int T>
__device__ __forceinline__ void hv_tile_pad(double* __restrict__ sA, int k, int tid) {
  for (int e = k * T + tid; e < K * T; e += kHvBlock) sA[e] = 0.0;
}

// entries [t0, t0 + T) gathered through `members` (NULL: entry m is candidate m) and transposed into
// [k][T]; an entry past M, -1 or outside [0, C) is staged as NaN.  The caller puts the barriers round it
template <int T>
__device__ __forceinline__ void hv_stage_tile(double* __restrict__ sA, const double* __restrict__ costs, int C, int k,
                                              const int* __restrict__ members, int M, int t0, int tid) {
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  for (int e = tid; e < T * k; e += kHvBlock) {
    const int t = e / k, j = e - t * k, m = t0 + t;
    double v = nan;
    if (m < M) {
      const int c = members ? members[m] : m;
      if (c >= 0 && c < C) v = costs[(size_t)c * k + j];
    }
    sA[j * T + t] = v;
  }
}

// vol of the contract: the product over ascending j of (ref_j - lo_j) from 1.0; *box is false for a box
// that is not finite with lo < ref
__device__ __forceinline__ double hv_box_volume(int k, const double* __restrict__ lo, const double* __restrict__ ref,
                                                bool* box) {
  double vol = 1.0;
  bool ok = true;
  for (int j = 0; j < k; ++j) {
    const double l = lo[j], r = ref[j];
    ok = ok && l - l == 0.0 && r - r == 0.0 && l < r;  // finite and not empty
    vol *= r - l;
  }
  *box = ok;
  return vol;
}

}  // namespace mpct
