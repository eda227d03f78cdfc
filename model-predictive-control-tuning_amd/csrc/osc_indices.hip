// osc_indices.hip — oscillation indices per setpoint segment of stored trajectories (include/mpct.h,
// "Oscillation indices per setpoint segment"): per (output row, segment) the number of band
// crossings, the decay ratio and the period of the first two peaks on one side, and the peak of the last
// lobe; per (input row, segment) the moves outside the dead zone, their direction reversals and the last
// reversing move.
//
// One 64-lane wave per unit (row, segment), kOscWaves units per workgroup, the segment index fastest so that
// neighbouring waves read adjacent memory; no LDS, no scratch.  The segment's bounds a = tseg[g], b = tseg[g+1]
// come from the kernel argument at a wave-uniform index.  A wave walks [a, b) in blocks of 64 samples, lane l
// reading sample a + 64 k + l, one coalesced load per block.
//
// These fields depend on the ORDER of the events, which a lane does not see.  Per block the wave takes the
// ballots P and N of the samples above and below the band (for the inputs: of the moves up and down).  The
// previous outside sample of a lane is the highest set bit of (P | N) below it; where there is none, a
// wave-uniform carry from the blocks before, which a block without any outside sample leaves as it is.  The
// ballot X of the crossings follows, and the lobe of a lane is the carried crossing count plus the number of
// crossings at or below it.  From there on everything is lane-local: a lane keeps the peak and the first
// sample of its own samples in the lobes k0 and k0 + 2 (strictly greater replaces: ascending t within a lane),
// and the peak of its samples in the last lobe so far, which restarts when a block opens a new lobe.  One
// arg-max per tracked lobe (largest value, then smallest t among the lanes that hold it: the first sample that
// attains the peak) and one maximum close the unit; a block costs ballots and scalar bit counts only.
// r(b-1), the base level c and u(a-1) are read once per unit at a wave-uniform address.  The previous input
// sample of a lane comes from its neighbour (lane_prev), lane 0 takes the last sample of the block before.
//
// band_rel*|d| is rounded before band_abs is added: contraction is off for this unit (the pragma below and
// the unit's flags in __graft_entry__.UNIT_FLAGS).  Every loop bound is a function of a and b alone.
#include <hip/hip_runtime.h>
#include <math.h>

#include "osc_indices.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {
__device__ __forceinline__ double wave_max64(double v) { return -pair_min<true>(pair_min<false>(row_min(-v))); }

// the order of the outside samples of one block.  pos / neg: this lane's sample lies above / below the band
// (never both; neither: inside, or no sample).  carry: the state (+1, -1; 0: none yet) of the last outside
// sample of the blocks before, ncross the crossings so far; both wave-uniform, both updated.
struct BlockOrder {
  unsigned long long outside, cross;  // ballots: the outside samples, and those that are crossings
  int lobe;                           // this lane's lobe index (meaningful on an outside lane)
  int last;                           // the highest lobe index so far, this block included
};
__device__ __forceinline__ BlockOrder block_order(bool pos, bool neg, unsigned long long below, unsigned long long upto,
                                                  int& carry, int& ncross) {
  const unsigned long long P = __ballot(pos), N = __ballot(neg), O = P | N;
  BlockOrder o{O, 0ull, ncross, ncross};
  if (O != 0ull) {  // wave-uniform; a block without an outside sample leaves carry and ncross alone
    const unsigned long long lower = O & below;
    int prev = carry;
    if (lower != 0ull) prev = (P >> top_bit(lower)) & 1ull ? 1 : -1;
    const int st = pos ? 1 : -1;
    o.cross = __ballot((pos || neg) && prev != 0 && prev != st);
    o.lobe = ncross + __popcll(o.cross & upto);
    o.last = ncross + __popcll(o.cross);
    carry = (P >> top_bit(O)) & 1ull ? 1 : -1;
    ncross = o.last;
  }
  return o;
}
}  // namespace

__global__ void __launch_bounds__(64 * kOscWaves)
    osc_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                       long long ny, long long nunits, int nref, int my, int nu, int nit, OscParams p, OscOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long unit = (long long)blockIdx.x * kOscWaves + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  if (unit >= nunits) return;  // wave-uniform
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const int kNone = 0x7fffffff;
  const int nseg = p.nseg;
  const unsigned long long below = lanes_below(lane), upto = below | (1ull << lane);
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
    const double h = p.band_rel * fabs(d) + p.band_abs;
    const int k0 = d != 0.0 ? 1 : 0;  // sigma != 0: lobe 0 is the approach to the new level
    int carry = 0, ncross = 0;
    double m0 = -1.0, m2 = -1.0, ml = 0.0;  // an outside |x| is > h >= 0
    int t0 = kNone, t2 = kNone;
    bool bad = !isfinite(c) || !isfinite(rg);
    for (int blk = 0; blk < n; blk += kWave) {
      const int k = blk + lane, t = a + k;
      const bool active = k < n;
      const double yv = active ? yr[t] : 0.0;
      bad |= active && !isfinite(yv);
      const double x = yv - rg, ax = fabs(x);
      const bool pos = active && x > h, neg = active && x < -h;  // |x| == h is inside; a NaN is neither
      const int before = ncross;
      const BlockOrder o = block_order(pos, neg, below, upto, carry, ncross);
      if (o.last > before) ml = 0.0;  // wave-uniform: the block opens a new last lobe
      if (pos || neg) {
        if (o.lobe == k0 && ax > m0) {  // strict: the first of equal peaks within the lane
          m0 = ax;
          t0 = t;
        }
        if (o.lobe == k0 + 2 && ax > m2) {
          m2 = ax;
          t2 = t;
        }
        if (o.lobe == o.last) ml = fmax(ml, ax);
      }
    }
    const bool invalid = __ballot(bad) != 0;
    double n0 = -m0, n2 = -m2;
    wave_argmin64(n0, t0);  // the largest peak and the smallest t among the lanes that hold it
    wave_argmin64(n2, t2);
    ml = wave_max64(ml);
    const bool two = ncross >= k0 + 2;  // a second peak on the side of lobe k0 left the band
    const double decay = two ? n2 / n0 : 0.0;  // (-A_{k0+2}) / (-A_{k0}): the same quotient
    if (lane == 0) {
      const size_t o = (size_t)unit;
      if (out.ncross) out.ncross[o] = invalid ? -1 : ncross;
      if (out.decay) out.decay[o] = invalid ? kNaN : decay;
      if (out.period) out.period[o] = (invalid || !two) ? -1 : t2 - t0;
      if (out.a_last) out.a_last[o] = invalid ? kNaN : (ncross >= k0 ? ml : 0.0);
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
    double prev_u = g == 0 ? 0.0 : ur[a - 1];
    const double tol = p.rev_tol;
    int carry = 0, nrev = 0, nmove = 0, t_rev = -1;
    bool bad = !isfinite(prev_u);
    for (int blk = 0; blk < n; blk += kWave) {
      const int k = blk + lane;
      const bool active = k < n;
      const double uv = active ? ur[a + k] : 0.0;
      double pv = lane_prev<64>(uv);  // every lane takes part; lane 0's comes from the block before
      if (lane == 0) pv = prev_u;
      prev_u = bcast(uv, kWave - 1);
      bad |= active && !isfinite(uv);
      const bool mv = active && k >= kmin;
      const double du = uv - pv;
      const bool pos = mv && du > tol, neg = mv && du < -tol;  // |du| == rev_tol is no move; +-0.0 neither
      const BlockOrder o = block_order(pos, neg, below, upto, carry, nrev);
      nmove += __popcll(o.outside);
      if (o.cross != 0ull) t_rev = a + blk + top_bit(o.cross);
    }
    const bool invalid = __ballot(bad) != 0;
    if (lane == 0) {
      const size_t o = (size_t)q;
      if (out.nmove) out.nmove[o] = invalid ? -1 : nmove;
      if (out.nrev) out.nrev[o] = invalid ? -1 : nrev;
      if (out.t_rev) out.t_rev[o] = invalid ? -1 : t_rev;
    }
  }
}

int launch_osc_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu,
                       int nit, const OscParams& p, const OscOut& out, hipStream_t stream, std::string* err) {
  const long long ny = out.any_y() ? S * my * p.nseg : 0, nunits = ny + (out.any_u() ? S * nu * p.nseg : 0);
  if (nunits == 0) return 0;
  const unsigned grid = (unsigned)((nunits + kOscWaves - 1) / kOscWaves);
  hipLaunchKernelGGL(osc_indices_kernel, dim3(grid), dim3(kWave * kOscWaves), 0, stream, y, u, r, ny, nunits, nref, my, nu,
                     nit, p, out);
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

}  // namespace mpct
