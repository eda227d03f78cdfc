// robust_tail.h — one candidate's tail statistics over its D plant draws (mpct_eval_robust_tail,
// include/mpct.h): type-1 empirical quantiles of the total cost J and the mean of the tail from each
// quantile upwards (CVaR).  The single definition of the order and of the summation, called by
// robust_tail_kernel (dtc_robust.hip).
//
// Draw k survives exactly as in robust_reduce.h: status 0, J(k) = sum_i J1_i(k) finite (summed over
// i = 0, 1, .., my - 1 in that order, so the two classifications agree bit for bit) and J(k) <=
// j_bound; a candidate with MPCT_ST_SKIPPED or MPCT_ST_BADHORIZON on any draw has no survivor.  The
// n survivors are ordered by J ascending and, among equal J, by draw index DESCENDING (-0.0 and
// +0.0 compare equal): the last of the order is then the largest J at its lowest index, which is
// robust_reduce's worst_draw.  Level a selects rank m = ceil(a * (double)n) clamped to [1, n];
// quantile = J_(m), q_draw = its draw, cvar = (J_(m) + .. + J_(n)) / (n - m + 1) with one accumulator
// from 0.0 in ascending rank order.  n = 0: NaN, NaN, -1.
//
// One wave, lane L owns draws L, L + 64, ..  LDS of the candidate, 12 B per draw: Js[D] the staged
// totals (NaN for a failed draw: no comparison with it is true, so it is never counted and never
// ranked) and idx[D], the draws in rank order.  A lane ranks its draw by counting the survivors
// below it; the count reads every Js[j] at a wave-uniform address (an LDS broadcast, no bank
// conflict).  The ranks of the survivors are a permutation of 0 .. n - 1, so the scatter idx[rank] = k
// stays inside idx[0 .. n).  Every LDS value is written and read by this one wave only: lds_sync()
// (wave_ops.h) is the hand-off, and no other wave of a workgroup may share the slice.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mpct_dev.h"
#include "wave_ops.h"

namespace mpct {

constexpr int kTailMaxLevels = 8;   // MPCT_TAIL_MAX_LEVELS
constexpr int kTailMaxDraws = 4096;  // MPCT_TAIL_MAX_DRAWS: 48 KB of LDS

// the levels travel by value (a call parameter like j_bound)
struct TailLevels {
  double a[kTailMaxLevels];
};

// per-candidate outputs (device pointers, any may be null), each [C][nlev]
struct TailOut {
  double* quantile;
  double* cvar;
  int32_t* q_draw;
};

__host__ __device__ inline size_t robust_tail_lds_bytes(int D) { return ((size_t)D * 12 + 15) & ~(size_t)15; }

// j1(k, i): J1_i of draw k; st(k): its status.  Js, idx: this wave's LDS slice.  Writes candidate
// c's record; on return the slice may be reused.
template <class FJ, class FS>
__device__ __forceinline__ void robust_tail(int lane, int D, int my, double j_bound, FJ j1, FS st, int nlev,
                                            const TailLevels& lv, const TailOut& out, long long c, double* Js,
                                            int* idx) {
  int never = 0, n = 0;
  for (int k0 = 0; k0 < D; k0 += kWave) {
    const int k = k0 + lane;
    bool surv = false;
    if (k < D) {
      const int s = st(k);
      never |= s & (MPCT_ST_SKIPPED_ | MPCT_ST_BADHORIZON_);
      double J = 0.0;
      for (int q = 0; q < my; ++q) J += j1(k, q);
      surv = s == 0 && isfinite(J) && J <= j_bound;
      Js[k] = surv ? J : NAN;
    }
    n += __popcll(__ballot(surv));
  }
  if (__ballot(never != 0)) n = 0;  // never simulated: no survivor
  lds_sync();
  if (n > 0) {
    for (int k0 = 0; k0 < D; k0 += kWave) {
      const int k = k0 + lane;
      const double Jk = k < D ? Js[k] : NAN;
      int rank = 0;
      for (int j = 0; j < D; ++j) {
        const double Jj = Js[j];  // the same address in every lane
        rank += (Jj < Jk || (Jj == Jk && j > k)) ? 1 : 0;
      }
      if (Jk == Jk) idx[rank] = k;
    }
    lds_sync();
  }
  if (lane < nlev) {
    double a = lv.a[0];
#pragma unroll
    for (int q = 1; q < kTailMaxLevels; ++q) a = lane == q ? lv.a[q] : a;
    double qv = NAN, cv = NAN;
    int qd = -1;
    if (n > 0) {
      const double x = ceil(a * (double)n);
      const int m = x < 1.0 ? 1 : (x > (double)n ? n : (int)x);
      qd = idx[m - 1];
      qv = Js[qd];
      double acc = 0.0;
      for (int r = m - 1; r < n; ++r) acc += Js[idx[r]];
      cv = acc / (double)(n - m + 1);
    }
    if (out.quantile) out.quantile[c * nlev + lane] = qv;
    if (out.cvar) out.cvar[c * nlev + lane] = cv;
    if (out.q_draw) out.q_draw[c * nlev + lane] = qd;
  }
  lds_sync();  // the slice is free for the next candidate
}

}  // namespace mpct
