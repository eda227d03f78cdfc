// segment_indices.hip — step-response indices per setpoint segment of stored trajectories (include/mpct.h,
// "Step-response indices per setpoint segment"): per (output row, segment) IAE, ISE, ITAE, peak
// error and its time, overshoot, undershoot (inverse response), final error, settling time and rise time; per
// (input row, segment) total variation, sum of squared moves, peak move and range.
//
// One 64-lane wave per unit (row, segment), kSegWaves units per workgroup, the segment index fastest so that
// neighbouring waves read adjacent memory; no LDS, no scratch.  The segment's bounds a = tseg[g], b = tseg[g+1]
// come from the kernel argument at a wave-uniform index.  A wave walks [a, b) in blocks of 64 samples: lane l
// reads sample a + 64 k + l, one coalesced load per signal and block, and accumulates exactly the samples with
// (t - a) mod 64 = l in ascending t from 0.0 (the contract's summation order); wave_sum64 (wave_ops.h) combines
// the 64 partials as a pairwise tree in lane order.  r(b-1), the base level c and u(a-1) are read once per
// unit at a wave-uniform address.  The previous input sample of a lane comes from its neighbour (lane_prev),
// lane 0 takes the last sample of the block before (a carry that starts at u(a-1)), so u is read once.  The
// first crossings of the rise levels are integer wave minima over the lanes' first crossings, the settling time
// an integer wave maximum of the last violating sample.
//
// Every product is rounded before it is added: contraction is off for this unit (the pragma below and the
// unit's flags in __graft_entry__.UNIT_FLAGS).  Every loop bound is a function of a and b alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "segment_indices.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {
__device__ __forceinline__ double wave_min64(double v) { return pair_min<true>(pair_min<false>(row_min(v))); }
__device__ __forceinline__ double wave_max64(double v) { return -wave_min64(-v); }
__device__ __forceinline__ int wave_min64_i(int v) { return pair_min_i<true>(pair_min_i<false>(row_min_i(v))); }
__device__ __forceinline__ int wave_max64_i(int v) { return -wave_min64_i(-v); }
__device__ __forceinline__ bool finite2(double a, double b) { return isfinite(a) && isfinite(b); }
}  // namespace

__global__ void __launch_bounds__(64 * kSegWaves)
    segment_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                           long long ny, long long nunits, int nref, int my, int nu, int nit, SegParams p, SegOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long unit = (long long)blockIdx.x * kSegWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= nunits) return;  // wave-uniform
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const int kNone = 0x7fffffff;
  const int nseg = p.nseg;
  if (unit < ny) {
    // ---- output unit (s, i, g): unit = (s * my + i) * nseg + g
    const long long row = unit / nseg;
    const int g = (int)(unit - row * nseg);
    const int a = p.tseg[g], b = p.tseg[g + 1], n = b - a;
    const long long s = row / my;
    const int i = (int)(row - s * my);
    const double* yr = y + (size_t)row * nit;
    const double* rr = r + ((size_t)(s % nref) * my + i) * nit;
    const double rg = rr[b - 1];
    const double c = (g == 0 || p.base == 0) ? yr[a] : rr[a - 1];
    const double d = rg - c;
    const double sg = d > 0.0 ? 1.0 : (d < 0.0 ? -1.0 : 0.0);
    const double band = p.band_rel * fabs(d) + p.band_abs;
    const double lvl_lo = p.rise_lo * fabs(d), lvl_hi = p.rise_hi * fabs(d);
    double iae = 0.0, ise = 0.0, itae = 0.0, m = -1.0, om = -INFINITY, um = -INFINITY;
    int tm = kNone, lastv = a - 1, tlo = kNone, thi = kNone;
    bool bad = !isfinite(c);  // y(a) is read again below; r(a-1) only here
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane;
      if (k < n) {
        const int t = a + k;
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
        if (!(fabs(yv - rg) <= band)) lastv = t;
        const double pv = sg * (yv - c);
        um = fmax(um, -pv);
        // ascending t within the lane: the minimum keeps the lane's first crossing
        if (pv >= lvl_lo) tlo = min(tlo, t);
        if (pv >= lvl_hi) thi = min(thi, t);
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
    um = wave_max64(um);
    const double over = sg == 0.0 ? emax : (om > 0.0 ? om : 0.0);
    const double under = sg == 0.0 ? 0.0 : (um > 0.0 ? um : 0.0);
    const int settle = wave_max64_i(lastv) + 1;
    tlo = wave_min64_i(tlo);
    thi = wave_min64_i(thi);
    const int rise = sg == 0.0 ? -1 : (thi == kNone ? n : thi - tlo);
    if (lane == 0) {
      const size_t o = (size_t)unit;
      if (out.iae) out.iae[o] = invalid ? kNaN : iae;
      if (out.ise) out.ise[o] = invalid ? kNaN : ise;
      if (out.itae) out.itae[o] = invalid ? kNaN : itae;
      if (out.emax) out.emax[o] = invalid ? kNaN : emax;
      if (out.t_emax) out.t_emax[o] = invalid ? -1 : tm;
      if (out.over) out.over[o] = invalid ? kNaN : over;
      if (out.under) out.under[o] = invalid ? kNaN : under;
      if (out.e_final) out.e_final[o] = invalid ? kNaN : yr[b - 1] - rg;
      if (out.settle) out.settle[o] = invalid ? -1 : settle;
      if (out.rise) out.rise[o] = invalid ? -1 : rise;
    }
  } else {
    // ---- input unit (s, j, g): q = (s * nu + j) * nseg + g
    const long long q = unit - ny;
    const long long row = q / nseg;
    const int g = (int)(q - row * nseg);
    const int a = p.tseg[g], b = p.tseg[g + 1], n = b - a;
    const double* ur = u + (size_t)row * nit;
    // the move across a boundary belongs to the segment it starts: segment g >= 1 begins with u(a) - u(a-1)
    const int kmin = g == 0 ? 1 : 0;
    double carry = g == 0 ? 0.0 : ur[a - 1];
    double tv = 0.0, du2 = 0.0, dm = 0.0, lo = INFINITY, hi = -INFINITY;
    bool bad = !isfinite(carry);
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane;
      const bool active = k < n;
      const double uv = active ? ur[a + k] : 0.0;
      double pv = lane_prev<64>(uv);  // every lane takes part; lane 0's comes from the block before
      if (lane == 0) pv = carry;
      carry = bcast(uv, kWave - 1);
      if (active) {
        bad |= !isfinite(uv);
        lo = fmin(lo, uv);
        hi = fmax(hi, uv);
        if (k >= kmin) {
          const double du = uv - pv, ad = fabs(du);
          tv += ad;
          du2 += du * du;
          dm = fmax(dm, ad);
        }
      }
    }
    const bool invalid = __ballot(bad) != 0;
    tv = wave_sum64(tv);
    du2 = wave_sum64(du2);
    dm = wave_max64(dm);
    // a zero extreme is +0.0 whatever the signs of the zeros in the segment
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

int launch_segment_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu,
                           int nit, const SegParams& p, const SegOut& out, hipStream_t stream, std::string* err) {
  const long long ny = out.any_y() ? S * my * p.nseg : 0, nunits = ny + (out.any_u() ? S * nu * p.nseg : 0);
  if (nunits == 0) return 0;
  const unsigned grid = (unsigned)((nunits + kSegWaves - 1) / kSegWaves);
  hipLaunchKernelGGL(segment_indices_kernel, dim3(grid), dim3(kWave * kSegWaves), 0, stream, y, u, r, ny, nunits, nref, my,
                     nu, nit, p, out);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

}  // namespace mpct
