// draw_stats.hip — statistics of a [C][D][m] table over its draw axis (include/mpct.h, "Robust index
// statistics"): per column (c, i) the survivor count, the mean, the smallest and the largest
// surviving value with their draws, and type-1 quantiles / tail means at up to 8 levels.
//
// One wave owns one column, NW = draw_stats_waves(D) consecutive columns share a workgroup.  A column's LDS
// slice is the one of robust_tail.h, 12 B per draw: Js[D] the staged values (NaN for a draw that does not
// survive: no comparison with it is true) and idx[D], the draws in rank order.
//
//   * staging: the whole workgroup loads its NW columns.  Consecutive columns of one candidate are
//     consecutive in memory, so with m > 1 thread q reads draw q / NW of column q % NW: runs of NW adjacent
//     values at a stride of m values, and the neighbouring workgroups read the rest of the same lines.  With
//     m = 1 a column is contiguous and thread q reads draw q % D of column q / D.  A workgroup barrier
//     publishes the slices to their waves.
//   * one pass over Js in ascending draw order, every lane the same wave-uniform LDS reads: n, the mean's
//     single accumulator from 0.0, and lo / hi with the lowest draw on ties (a strict comparison replaces
//     the extreme; -0.0 == +0.0, so the first of them keeps its bits).
//   * with levels: the ranking, the scatter into rank order and the tail walks of lanes j < nlev are
//     robust_tail's, statement for statement; inside a wave lds_sync() is the hand-off, because no other
//     wave touches the slice between the two barriers of an item.
//
// The workgroups stride over the groups of NW columns; every wave of a workgroup makes the same number of
// trips, so the barriers are uniform.  Every loop bound is a function of D, m, NW and nlev alone.  No
// products are added anywhere (the unit is built without contraction all the same, __graft_entry__.UNIT_FLAGS).
#include <hip/hip_runtime.h>
#include <math.h>

#include "draw_stats.h"
#include "mpct_dev.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

// one column from its staged slice; o: the column's output element
__device__ __forceinline__ void column_stats(int lane, int D, int nlev, const TailLevels& lv, const DrawStatsOut& out,
                                             long long o, const double* Js, int* idx) {
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  int n = 0, lod = -1, hid = -1;
  double sum = 0.0, lo = kNaN, hi = kNaN;
  for (int k = 0; k < D; ++k) {
    const double v = Js[k];  // the same address in every lane
    if (v == v) {
      sum += v;
      if (n == 0 || v < lo) lo = v, lod = k;
      if (n == 0 || v > hi) hi = v, hid = k;
      ++n;
    }
  }
  if (lane == 0) {
    if (out.n) out.n[o] = n;
    if (out.mean) out.mean[o] = n ? sum / (double)n : kNaN;
    if (out.lo) out.lo[o] = lo;
    if (out.lo_draw) out.lo_draw[o] = lod;
    if (out.hi) out.hi[o] = hi;
    if (out.hi_draw) out.hi_draw[o] = hid;
  }
  if (nlev == 0 || !out.any_level()) return;  // wave-uniform
  if (n > 0) {
    for (int k0 = 0; k0 < D; k0 += kWave) {
      const int k = k0 + lane;
      const double Jk = k < D ? Js[k] : kNaN;
      int rank = 0;
      for (int j = 0; j < D; ++j) {
        const double Jj = Js[j];  // the same address in every lane
        rank += (Jj < Jk || (Jj == Jk && j > k)) ? 1 : 0;
      }
      if (Jk == Jk) idx[rank] = k;  // the survivors' ranks are a permutation of 0 .. n-1
    }
    lds_sync();
  }
  if (lane < nlev) {
    double a = lv.a[0];
#pragma unroll
    for (int q = 1; q < kTailMaxLevels; ++q) a = lane == q ? lv.a[q] : a;
    double qv = kNaN, cv = kNaN;
    int qd = -1;
    if (n > 0) {
      const double x = ceil(a * (double)n);
      const int mr = x < 1.0 ? 1 : (x > (double)n ? n : (int)x);
      qd = idx[mr - 1];
      qv = Js[qd];
      double acc = 0.0;
      for (int r = mr - 1; r < n; ++r) acc += Js[idx[r]];
      cv = acc / (double)(n - mr + 1);
    }
    if (out.quantile) out.quantile[o * nlev + lane] = qv;
    if (out.cvar) out.cvar[o * nlev + lane] = cv;
    if (out.q_draw) out.q_draw[o * nlev + lane] = qd;
  }
}

// ncols = C * m columns; blockDim.x = 64 NW; dynamic LDS = NW slices of robust_tail_lds_bytes(D)
template <bool I32>
__global__ void __launch_bounds__(kWave* kStatMaxWaves)
    draw_stats_kernel(const void* __restrict__ xv, const int* __restrict__ alive, long long ncols, int D, int m, int nlev,
                      const TailLevels lv, const DrawStatsOut out, int ldo, int off) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x, lane = tid & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int NW = blockDim.x >> 6;
  const int sl = (int)(robust_tail_lds_bytes(D) / 8);  // doubles of one slice
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* Js = lds + wave * sl;
  int* idx = reinterpret_cast<int*>(Js + D);
  const long long ngroups = (ncols + NW - 1) / NW;
  for (long long g = blockIdx.x; g < ngroups; g += gridDim.x) {
    const long long col0 = g * NW;
    for (int q = tid; q < NW * D; q += NW * kWave) {
      int j, k;
      if (m == 1) {
        j = q / D;
        k = q - j * D;
      } else {
        k = q / NW;
        j = q - k * NW;
      }
      const long long col = col0 + j;
      if (col < ncols) {
        const long long c = col / m;
        const int i = (int)(col - c * m);
        const long long s = c * D + k;
        double v;
        if (I32) {
          const int iv = static_cast<const int*>(xv)[s * m + i];
          v = iv >= 0 ? (double)iv : kNaN;
        } else {
          v = static_cast<const double*>(xv)[s * m + i];
          if (!isfinite(v)) v = kNaN;
        }
        if (alive && alive[s] == 0) v = kNaN;
        lds[j * sl + k] = v;
      }
    }
    __syncthreads();  // the slices, staged by every wave, to their owners
    const long long col = col0 + wave;
    if (col < ncols) {  // wave-uniform
      const long long c = col / m;
      column_stats(lane, D, nlev, lv, out, c * ldo + off + (col - c * m), Js, idx);
    }
    __syncthreads();  // every slice is read out before the next item's staging rewrites it
  }
}

// alive [C][D] from the per-simulation costs and statuses: one wave per candidate
__global__ void __launch_bounds__(kWave* kStatMaxWaves)
    draw_alive_kernel(long long C, int D, int my, double j_bound, const double* __restrict__ J1,
                      const int* __restrict__ status, int* __restrict__ alive) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long c = (long long)blockIdx.x * kStatMaxWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (c >= C) return;  // wave-uniform
  const int* s = status + c * D;
  const double* j = J1 + c * D * my;
  int never = 0;
  for (int k0 = 0; k0 < D; k0 += kWave) {
    const int k = k0 + lane;
    if (k < D) never |= s[k] & (MPCT_ST_SKIPPED_ | MPCT_ST_BADHORIZON_);
  }
  const bool dead = __ballot(never != 0) != 0;  // never simulated: no live draw
  for (int k0 = 0; k0 < D; k0 += kWave) {
    const int k = k0 + lane;
    if (k < D) {
      double J = 0.0;
      for (int q = 0; q < my; ++q) J += j[(long long)k * my + q];
      alive[c * D + k] = (!dead && s[k] == 0 && isfinite(J) && J <= j_bound) ? 1 : 0;
    }
  }
}

}  // namespace mpct

// ------------------------------------------------------------------------------------------
// host-side launches
namespace mpct {

static int launched(std::string* err) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

int launch_draw_stats(const void* x, int x_type, const int* alive, long long C, int D, int m, int nlev,
                      const double* levels, const DrawStatsOut& out, int ldo, int off, int grid_cap, hipStream_t stream,
                      std::string* err) {
  if (C == 0) return 0;
  TailLevels lv;
  for (int q = 0; q < kTailMaxLevels; ++q) lv.a[q] = q < nlev ? levels[q] : 1.0;
  const int NW = draw_stats_waves(D);
  const long long ncols = C * m, ngroups = (ncols + NW - 1) / NW;
  const long long cap = grid_cap > 0 ? grid_cap : kStatGridCap;
  const unsigned grid = (unsigned)(ngroups < cap ? ngroups : cap);
  const size_t lds = (size_t)NW * robust_tail_lds_bytes(D);
  if (x_type == kStatI32)
    hipLaunchKernelGGL(draw_stats_kernel<true>, dim3(grid), dim3(kWave * NW), lds, stream, x, alive, ncols, D, m, nlev, lv,
                       out, ldo, off);
  else
    hipLaunchKernelGGL(draw_stats_kernel<false>, dim3(grid), dim3(kWave * NW), lds, stream, x, alive, ncols, D, m, nlev, lv,
                       out, ldo, off);
  return launched(err);
}

int launch_draw_alive(long long C, int D, int my, double j_bound, const double* J1, const int* status, int* alive,
                      hipStream_t stream, std::string* err) {
  if (C == 0) return 0;
  const unsigned grid = (unsigned)((C + kStatMaxWaves - 1) / kStatMaxWaves);
  hipLaunchKernelGGL(draw_alive_kernel, dim3(grid), dim3(kWave * kStatMaxWaves), 0, stream, C, D, my, j_bound, J1, status,
                     alive);
  return launched(err);
}

}  // namespace mpct
