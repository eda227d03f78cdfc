// envelope.hip — trajectory envelopes over plant draws (include/mpct.h, "Trajectory envelopes"):
// per sample (c, row, t) of stored trajectories the statistics of draw_stats.h over the D draws of a
// candidate, and per (c, row) the spread of the band hi - lo over time.
//
// draw_envelope_kernel.  The table is x[C][D][m], m = rows * nit.  One lane owns one column j of a candidate's
// [D][m] block; a workgroup owns a tile of consecutive columns of one candidate, so for each draw k a wave's
// load is 64 consecutive doubles and every byte of the table is read once.  alive[c][k] is wave-uniform.
//   * base statistics: one pass over k ascending in the lane's registers, by the rules of draw_stats.h: n,
//     the mean's single accumulator from 0.0, lo / hi with the lowest draw on ties (a strict comparison
//     replaces the extreme; -0.0 == +0.0, so the first of them keeps its bits).
//   * with levels: the same pass stages the column into an LDS tile Js[D][T] (NaN for a draw that does not
//     survive: no comparison with it is true) -- consecutive lanes are consecutive doubles, so every
//     ds_read_b64 / ds_write_b64 is conflict-free -- and the lane then makes robust_tail's ranking, scatter
//     and tail walks on its own column, statement for statement: rank(k) = #{j : J_j < J_k or (J_j == J_k and
//     j > k)}, idx[rank] = k (a byte per draw, idx[D][T]; D <= kEnvLaneMaxDraws <= 256), m_j = ceil(a_j * n)
//     clamped, the quantile, its draw, and cvar with one accumulator in ascending rank order.  A column is
//     private to its lane from the staging to the last walk, so the kernel has no barrier and no hand-off.
// The workgroups stride over the tiles (C * ceil(m / T) of them).  No products are added anywhere (the unit
// is built without contraction all the same, __graft_entry__.UNIT_FLAGS).
//
// envelope_spread_kernel.  One wave per (c, row), kEnvSpreadWaves rows per workgroup, no LDS: d(t) = hi(t) -
// lo(t), rounded once; lane (t - t0) mod 64 accumulates its d in ascending t from 0.0 and wave_sum64 combines
// the 64 partials as a pairwise tree in lane order (the summation order of traj_indices.hip); the maximum and
// the first t that attains it are exact selections.  A sample without a survivor has lo = NaN: the row then
// gives NaN / -1.
#include <hip/hip_runtime.h>
#include <math.h>

#include "envelope.h"
#include "mpct_dev.h"
#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

// ncols = m columns per candidate, ntile = ceil(m / T) tiles per candidate, nitems = C * ntile;
// blockDim.x = max(T, 64); LEVELS: dynamic LDS = envelope_lds_bytes(D, T)
template <bool LEVELS>
__global__ void __launch_bounds__(kEnvMaxTile)
    draw_envelope_kernel(const double* __restrict__ x, const int* __restrict__ alive, long long nitems, int ntile, int T,
                         int D, int m, int nlev, const TailLevels lv, const DrawStatsOut out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int tid = threadIdx.x;
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  double* Js = lds + tid;                                                    // Js[k * T]: draw k of this lane's column
  unsigned char* idx = reinterpret_cast<unsigned char*>(lds + (size_t)D * T) + tid;  // idx[r * T]: the draw of rank r
  for (long long g = blockIdx.x; g < nitems; g += gridDim.x) {
    const long long c = g / ntile;
    const int j = (int)(g - c * ntile) * T + tid;
    if (tid >= T || j >= m) continue;  // no barrier below: a lane without a column just skips the item
    const double* col = x + c * D * (long long)m + j;
    const int* al = alive ? alive + c * D : nullptr;
    int n = 0, lod = -1, hid = -1;
    double sum = 0.0, lo = kNaN, hi = kNaN;
    for (int k = 0; k < D; ++k) {
      double v = col[(long long)k * m];
      if (!isfinite(v)) v = kNaN;
      if (al && al[k] == 0) v = kNaN;  // the same address in every lane
      if (LEVELS) Js[k * T] = v;
      if (v == v) {
        sum += v;
        if (n == 0 || v < lo) lo = v, lod = k;
        if (n == 0 || v > hi) hi = v, hid = k;
        ++n;
      }
    }
    const long long o = c * m + j;
    if (out.n) out.n[o] = n;
    if (out.mean) out.mean[o] = n ? sum / (double)n : kNaN;
    if (out.lo) out.lo[o] = lo;
    if (out.lo_draw) out.lo_draw[o] = lod;
    if (out.hi) out.hi[o] = hi;
    if (out.hi_draw) out.hi_draw[o] = hid;
    if (!LEVELS) continue;
    if (n > 0) {
      for (int k = 0; k < D; ++k) {
        const double Jk = Js[k * T];
        int rank = 0;
        for (int q = 0; q < D; ++q) {
          const double Jj = Js[q * T];
          rank += (Jj < Jk || (Jj == Jk && q > k)) ? 1 : 0;
        }
        if (Jk == Jk) idx[rank * T] = (unsigned char)k;  // the survivors' ranks are a permutation of 0 .. n-1
      }
    }
    for (int q = 0; q < nlev; ++q) {
      const double a = lv.a[q];
      double qv = kNaN, cv = kNaN;
      int qd = -1;
      if (n > 0) {
        const double xr = ceil(a * (double)n);
        const int mr = xr < 1.0 ? 1 : (xr > (double)n ? n : (int)xr);
        qd = idx[(mr - 1) * T];
        qv = Js[qd * T];
        double acc = 0.0;
        for (int r = mr - 1; r < n; ++r) acc += Js[(int)idx[r * T] * T];
        cv = acc / (double)(n - mr + 1);
      }
      if (out.quantile) out.quantile[o * nlev + q] = qv;
      if (out.cvar) out.cvar[o * nlev + q] = cv;
      if (out.q_draw) out.q_draw[o * nlev + q] = qd;
    }
  }
}

// lo, hi [nrows][nit]; one wave per row
__global__ void __launch_bounds__(kWave* kEnvSpreadWaves)
    envelope_spread_kernel(const double* __restrict__ lo, const double* __restrict__ hi, long long nrows, int nit, int t0,
                           const EnvSpreadOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long row = (long long)blockIdx.x * kEnvSpreadWaves + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (row >= nrows) return;  // wave-uniform
  const double kNaN = __longlong_as_double(0x7ff8000000000000LL);
  const double* lr = lo + row * nit;
  const double* hr = hi + row * nit;
  const int n = nit - t0;
  double sp = 0.0, mx = -1.0;
  int tm = 0x7fffffff;
  bool bad = false;
  for (int k0 = 0; k0 < n; k0 += kWave) {
    const int k = k0 + lane;
    if (k < n) {
      const double l = lr[t0 + k], h = hr[t0 + k];
      bad |= !(l == l);  // no survivor at this sample
      const double d = h - l;
      sp += d;
      if (d > mx) {  // strict: the first of equal maxima within the lane
        mx = d;
        tm = t0 + k;
      }
    }
  }
  const bool invalid = __ballot(bad) != 0;
  sp = wave_sum64(sp);
  double nm = -mx;
  wave_argmin64(nm, tm);  // the largest d and the smallest t among the lanes that hold it
  if (lane == 0) {
    if (out.spread) out.spread[row] = invalid ? kNaN : sp;
    if (out.spread_max) out.spread_max[row] = invalid ? kNaN : -nm;
    if (out.t_spread_max) out.t_spread_max[row] = invalid ? -1 : tm;
  }
}

// ------------------------------------------------------------------------------------------
// host-side launches

static int env_launched(std::string* err) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

int launch_draw_envelope(const double* x, const int* alive, long long C, int D, int m, int nlev, const double* levels,
                         const DrawStatsOut& out, int grid_cap, hipStream_t stream, std::string* err) {
  if (C == 0) return 0;
  const bool lev = nlev > 0 && out.any_level();
  if (lev && D > kEnvLaneMaxDraws) {
    *err = "draw_envelope_kernel: D exceeds the lane kernel's LDS tile";
    return -3;
  }
  TailLevels lv;
  for (int q = 0; q < kTailMaxLevels; ++q) lv.a[q] = q < nlev ? levels[q] : 1.0;
  const int T = envelope_tile(D, lev), ntile = (m + T - 1) / T;
  const long long nitems = C * ntile, cap = grid_cap > 0 ? grid_cap : kEnvGridCap;
  const unsigned grid = (unsigned)(nitems < cap ? nitems : cap);
  const unsigned block = (unsigned)(T < kWave ? kWave : T);
  if (lev)
    hipLaunchKernelGGL(draw_envelope_kernel<true>, dim3(grid), dim3(block), envelope_lds_bytes(D, T), stream, x, alive,
                       nitems, ntile, T, D, m, nlev, lv, out);
  else
    hipLaunchKernelGGL(draw_envelope_kernel<false>, dim3(grid), dim3(block), 0, stream, x, alive, nitems, ntile, T, D, m, 0,
                       lv, out);
  return env_launched(err);
}

int launch_envelope_spread(const double* lo, const double* hi, long long nrows, int nit, int t0, const EnvSpreadOut& out,
                           hipStream_t stream, std::string* err) {
  if (nrows == 0 || !out.any()) return 0;
  const unsigned grid = (unsigned)((nrows + kEnvSpreadWaves - 1) / kEnvSpreadWaves);
  hipLaunchKernelGGL(envelope_spread_kernel, dim3(grid), dim3(kWave * kEnvSpreadWaves), 0, stream, lo, hi, nrows, nit, t0,
                     out);
  return env_launched(err);
}

}  // namespace mpct
