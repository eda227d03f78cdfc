// traj_indices.hip — closed-loop performance indices of stored trajectories (include/mpct.h, "Closed-loop
// performance indices"): IAE, ISE, ITAE, peak error and its time, overshoot, final error and
// settling time per output row; total variation, sum of squared moves, peak move and range per input row.
//
// One 64-lane wave per row, kIndexWaves rows per workgroup, no LDS.  A wave walks its row in blocks of 64
// samples from t0: lane l reads sample t0 + 64 b + l, so every block is one coalesced 512-byte load per
// signal, and lane l accumulates exactly the samples with (t - t0) mod 64 = l in ascending t from 0.0 (the
// contract's summation order).  r(nit-1) and y(t0) are read once per row at a wave-uniform address.  The
// previous input sample of a lane comes from its neighbour (lane_prev), lane 0 takes the last sample of
// the block before (a carry), so u is read once.  The 64 partial sums are combined by wave_sum64
// (wave_ops.h): a pairwise tree in lane order, ((p0 + p1) + (p2 + p3)) + .. up to (p0..31) + (p32..63).
// Maxima, minima, the first time of the peak error (the smallest t among the lanes holding the maximum,
// wave_argmin64 on the negated value) and the settling time are exact integers / selections.
//
// Every product is rounded before it is added: contraction is off for this unit (the pragma below and the
// unit's flags in __graft_entry__.UNIT_FLAGS), so no fused multiply-add appears in ise, itae, du2 or band.
// Every loop bound is a function of nit and t0 alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "traj_indices.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {
__device__ __forceinline__ double wave_min64(double v) { return pair_min<true>(pair_min<false>(row_min(v))); }
__device__ __forceinline__ double wave_max64(double v) { return -wave_min64(-v); }
__device__ __forceinline__ int wave_max64_i(int v) { return -pair_min_i<true>(pair_min_i<false>(row_min_i(-v))); }
__device__ __forceinline__ bool finite2(double a, double b) { return isfinite(a) && isfinite(b); }
}  // namespace

__global__ void __launch_bounds__(64 * kIndexWaves)
    traj_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                        long long ny, long long nrows, int nref, int my, int nu, int nit, IndexParams p, IndexOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long row = (long long)blockIdx.x * kIndexWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= nrows) return;  // wave-uniform
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const int t0 = p.t0, n = nit - t0;
  if (row < ny) {
    // ---- output row (s, i): row = s * my + i
    const long long s = row / my;
    const int i = (int)(row - s * my);
    const double* yr = y + (size_t)row * nit;
    const double* rr = r + ((size_t)(s % nref) * my + i) * nit;
    const double rf = rr[nit - 1], y0 = yr[t0];
    const double d = rf - y0;
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    const double band = p.band_rel * fabs(d) + p.band_abs;
    double iae = 0.0, ise = 0.0, itae = 0.0, m = -1.0, om = -INFINITY;
    int tm = 0x7fffffff, lastv = t0 - 1;
    bool bad = false;
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane;
      if (k < n) {
        const int t = t0 + k;
        const double yv = yr[t], rv = rr[t];
        bad |= !finite2(yv, rv);
        const double e = yv - rv, ae = fabs(e);
        iae += ae;
        ise += e * e;
        itae += (double)k * ae;
        if (ae > m) {  // strict: the first of equal maxima within the lane
          m = ae;
          tm = t;
        }
        om = fmax(om, sg * e);
        if (!(fabs(yv - rf) <= band)) lastv = t;
      }
    }
    const bool invalid = __ballot(bad) != 0;
    iae = wave_sum64(iae);
    ise = wave_sum64(ise);
    itae = wave_sum64(itae);
    double nm = -m;
    wave_argmin64(nm, tm);  // the largest m and the smallest t among the lanes that hold it
    const double emax = -nm;
    om = wave_max64(om);
    const double over = sg == 0.0 ? emax : (om > 0.0 ? om : 0.0);
    const int settle = wave_max64_i(lastv) + 1;
    if (lane == 0) {
      const size_t o = (size_t)row;
      if (out.iae) out.iae[o] = invalid ? kNaN : iae;
      if (out.ise) out.ise[o] = invalid ? kNaN : ise;
      if (out.itae) out.itae[o] = invalid ? kNaN : itae;
      if (out.emax) out.emax[o] = invalid ? kNaN : emax;
      if (out.t_emax) out.t_emax[o] = invalid ? -1 : tm;
      if (out.over) out.over[o] = invalid ? kNaN : over;
      if (out.e_final) out.e_final[o] = invalid ? kNaN : yr[nit - 1] - rf;
      if (out.settle) out.settle[o] = invalid ? -1 : settle;
    }
  } else {
    // ---- input row (s, j): q = s * nu + j
    const long long q = row - ny;
    const double* ur = u + (size_t)q * nit;
    double tv = 0.0, du2 = 0.0, dm = 0.0, lo = INFINITY, hi = -INFINITY, carry = 0.0;
    bool bad = false;
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane;
      const bool active = k < n;
      const double uv = active ? ur[t0 + k] : 0.0;
      double pv = lane_prev<64>(uv);  // every lane takes part; lane 0's comes from the block before
      if (lane == 0) pv = carry;
      carry = bcast(uv, kWave - 1);
      if (active) {
        bad |= !isfinite(uv);
        lo = fmin(lo, uv);
        hi = fmax(hi, uv);
        if (k >= 1) {
          const double du = uv - pv, a = fabs(du);
          tv += a;
          du2 += du * du;
          dm = fmax(dm, a);
        }
      }
    }
    const bool invalid = __ballot(bad) != 0;
    tv = wave_sum64(tv);
    du2 = wave_sum64(du2);
    dm = wave_max64(dm);
    // a zero extreme is +0.0 whatever the signs of the zeros in the row
    lo = wave_min64(lo) + 0.0;
    hi = wave_max64(hi) + 0.0;
    if (lane == 0) {
      const size_t o = (size_t)q;
      if (out.tv) out.tv[o] = invalid ? kNaN : tv;
      if (out.du2) out.du2[o] = invalid ? kNaN : du2;
      if (out.dumax) out.dumax[o] = invalid ? kNaN : dm;
      if (out.u_lo) out.u_lo[o] = invalid ? kNaN : lo;
      if (out.u_hi) out.u_hi[o] = invalid ? kNaN : hi;
    }
  }
}

int launch_traj_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu, int nit,
                        const IndexParams& p, const IndexOut& out, hipStream_t stream, std::string* err) {
  const long long ny = out.any_y() ? S * my : 0, nrows = ny + (out.any_u() ? S * nu : 0);
  if (nrows == 0) return 0;
  const unsigned grid = (unsigned)((nrows + kIndexWaves - 1) / kIndexWaves);
  hipLaunchKernelGGL(traj_indices_kernel, dim3(grid), dim3(kWave * kIndexWaves), 0, stream, y, u, r, ny, nrows, nref, my,
                     nu, nit, p, out);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

}  // namespace mpct
