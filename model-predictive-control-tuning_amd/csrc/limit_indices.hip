// limit_indices.hip — limit indices of stored trajectories (include/mpct.h, "Limit indices"):
// band violation (sum, sum of squares, peak and its time, samples outside, time of re-entry, margin) per
// output row; samples at the amplitude bounds and at the rate bounds, the longest saturated run and the
// margins per input row.
//
// One 64-lane wave per row, kLimitWaves rows per workgroup, no LDS, no scratch.  A wave walks its row in
// blocks of 64 samples from t0: lane l reads sample t0 + 64 b + l, one coalesced 512-byte load per block, and
// accumulates exactly the samples with (t - t0) mod 64 = l in ascending t from 0.0 (the contract's summation
// order); wave_sum64 (wave_ops.h) combines the 64 partials as a pairwise tree in lane order.  The bounds of the
// row's channel are read from the kernel argument at a wave-uniform index.  The previous input sample of a
// lane comes from its neighbour (lane_prev), lane 0 takes the last sample of the block before (a carry).
//
// Counts and times come from __ballot masks, which hold a block's flags in time order (bit l = sample
// t0 + 64 b + l): a count is the mask's population, the last sample outside the band its highest bit, both
// wave-uniform integers.  sat_run: with the block's mask m of saturated samples, lane l takes the length of
// the run of ones that ends at bit l -- l minus the position of the highest zero at or below l, or, where
// there is none, l + 1 plus the running length carried from the blocks before -- and keeps the largest it
// saw; the carry becomes carry + 64 for a full mask, else the mask's count of leading ones.  A lane past the
// row's end has a zero bit.  One wave-wide integer maximum at the end gives the exact longest run, whatever
// block edges it crossed; no loop runs over the bits.
//
// Every product is rounded before it is added: contraction is off for this unit (the pragma below and the
// unit's flags in __graft_entry__.UNIT_FLAGS).  Every loop bound is a function of nit - t0 alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "limit_indices.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {
__device__ __forceinline__ double wave_min64(double v) { return pair_min<true>(pair_min<false>(row_min(v))); }
__device__ __forceinline__ int wave_max64_i(int v) { return -pair_min_i<true>(pair_min_i<false>(row_min_i(-v))); }
}  // namespace

__global__ void __launch_bounds__(64 * kLimitWaves)
    limit_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, long long ny, long long nrows, int my,
                         int nu, int nit, LimitParams p, LimitOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long row = (long long)blockIdx.x * kLimitWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (row >= nrows) return;  // wave-uniform
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const int t0 = p.t0, n = nit - t0;
  if (row < ny) {
    // ---- output row (s, i): row = s * my + i
    const int i = (int)((unsigned)row % (unsigned)my);  // row < 2^31
    const double* yr = y + (size_t)row * nit;
    const double lo = p.y_lo[i], hi = p.y_hi[i], tol = p.out_tol;
    double viol = 0.0, viol2 = 0.0, vm = -1.0, marg = INFINITY;
    int tm = 0x7fffffff, nout = 0, last = t0 - 1;
    bool bad = false;
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane, t = t0 + k;
      const bool active = k < n;
      const double yv = active ? yr[t] : 0.0;
      const double m = fmax(lo - yv, yv - hi);
      const double ex = m > 0.0 ? m : 0.0;  // fmax(m, 0.0) with a zero always +0.0
      if (active) {
        bad |= !isfinite(yv);
        viol += ex;
        viol2 += ex * ex;
        if (ex > vm) {  // strict: the first of equal maxima within the lane
          vm = ex;
          tm = t;
        }
        marg = fmin(marg, fmin(yv - lo, hi - yv));
      }
      const unsigned long long om = __ballot(active && ex > tol);  // bit l: sample t0 + k0 + l is outside
      nout += __popcll(om);
      if (om) last = t0 + k0 + 63 - __clzll(om);
    }
    const bool invalid = __ballot(bad) != 0;
    viol = wave_sum64(viol);
    viol2 = wave_sum64(viol2);
    double nm = -vm;
    wave_argmin64(nm, tm);  // the largest ex and the smallest t among the lanes that hold it
    // a zero margin is +0.0 whatever the signs of the zeros in the row
    marg = wave_min64(marg) + 0.0;
    if (lane == 0) {
      const size_t o = (size_t)row;
      if (out.viol) out.viol[o] = invalid ? kNaN : viol;
      if (out.viol2) out.viol2[o] = invalid ? kNaN : viol2;
      if (out.vmax) out.vmax[o] = invalid ? kNaN : -nm;
      if (out.t_vmax) out.t_vmax[o] = invalid ? -1 : tm;
      if (out.n_out) out.n_out[o] = invalid ? -1 : nout;
      if (out.t_in) out.t_in[o] = invalid ? -1 : last + 1;
      if (out.y_margin) out.y_margin[o] = invalid ? kNaN : marg;
    }
  } else {
    // ---- input row (s, j): q = s * nu + j
    const long long q = row - ny;
    const int j = (int)((unsigned)q % (unsigned)nu);
    const double* ur = u + (size_t)q * nit;
    const double ulo = p.u_lo[j], uhi = p.u_hi[j], dlo = p.du_lo[j], dhi = p.du_hi[j], tol = p.sat_tol;
    double um = INFINITY, dm = INFINITY, carry = 0.0;
    int nlo = 0, nhi = 0, nrate = 0, run = 0, best = 0;
    bool bad = false;
    // the bits at or below this lane's
    const unsigned long long below = (2ull << lane) - 1ull;
    for (int k0 = 0; k0 < n; k0 += kWave) {
      const int k = k0 + lane;
      const bool active = k < n;
      const double uv = active ? ur[t0 + k] : 0.0;
      double pv = lane_prev<64>(uv);  // every lane takes part; lane 0's comes from the block before
      if (lane == 0) pv = carry;
      carry = bcast(uv, kWave - 1);
      const double du = uv - pv;
      const bool at_lo = active && uv - ulo <= tol, at_hi = active && uhi - uv <= tol;
      const bool moved = active && k >= 1;
      const bool at_rate = moved && (du - dlo <= tol || dhi - du <= tol);
      if (active) {
        bad |= !isfinite(uv);
        um = fmin(um, fmin(uv - ulo, uhi - uv));
      }
      if (moved) dm = fmin(dm, fmin(du - dlo, dhi - du));
      nlo += __popcll(__ballot(at_lo));
      nhi += __popcll(__ballot(at_hi));
      nrate += __popcll(__ballot(at_rate));
      const unsigned long long m = __ballot(at_lo || at_hi);  // bit l: sample t0 + k0 + l is saturated
      const unsigned long long z = ~m & below;                // the unsaturated samples up to this lane's
      const int len = z ? lane - (63 - __clzll(z)) : lane + 1 + run;
      best = max(best, len);
      run = ~m ? __clzll(~m) : run + kWave;
    }
    const bool invalid = __ballot(bad) != 0;
    best = wave_max64_i(best);
    um = wave_min64(um) + 0.0;
    dm = wave_min64(dm) + 0.0;
    if (lane == 0) {
      const size_t o = (size_t)q;
      if (out.n_lo) out.n_lo[o] = invalid ? -1 : nlo;
      if (out.n_hi) out.n_hi[o] = invalid ? -1 : nhi;
      if (out.n_rate) out.n_rate[o] = invalid ? -1 : nrate;
      if (out.sat_run) out.sat_run[o] = invalid ? -1 : best;
      if (out.u_margin) out.u_margin[o] = invalid ? kNaN : um;
      if (out.du_margin) out.du_margin[o] = invalid ? kNaN : dm;
    }
  }
}

int launch_limit_indices(const double* y, const double* u, long long S, int my, int nu, int nit, const LimitParams& p,
                         const LimitOut& out, hipStream_t stream, std::string* err) {
  const long long ny = out.any_y() ? S * my : 0, nrows = ny + (out.any_u() ? S * nu : 0);
  if (nrows == 0) return 0;
  const unsigned grid = (unsigned)((nrows + kLimitWaves - 1) / kLimitWaves);
  hipLaunchKernelGGL(limit_indices_kernel, dim3(grid), dim3(kWave * kLimitWaves), 0, stream, y, u, ny, nrows, my, nu, nit,
                     p, out);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

}  // namespace mpct
