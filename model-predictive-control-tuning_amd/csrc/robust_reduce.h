// robust_reduce.h — one candidate's statistics over its D plant draws / reference sets
// (mpct_eval_robust, include/mpct.h): the single definition of the semantics and of the summation
// order, called by the fused kernel (dtc_robust_kernel, records in LDS) and by the generic
// reduction (robust_reduce_kernel, records in global memory), both in dtc_robust.hip.
//
// Draw k fails when its status is non-zero, or J(k) = sum_i J1_i(k) is not finite, or J(k) >
// j_bound; every other draw survives.  A candidate whose draws carry MPCT_ST_SKIPPED or
// MPCT_ST_BADHORIZON was never simulated: NaN statistics, n_failed = 0, worst_draw = -1.
//
// Order (fixed; a record depends on nothing but the candidate's own D records): lane i < my owns
// output i and walks the draws k = 0, 1, .., D - 1 in that order with one accumulator; J(k) is
// summed over i = 0, 1, .., my - 1 in that order; mean_i = (sum of the surviving J1_i(k)) / n.  The
// worst draw is the first k whose J(k) exceeds every earlier surviving one (lowest index on ties).
// With a finite j_bound every surviving term is <= j_bound, so a sum of D of them stays finite for
// D * j_bound < 1.8e308 (the default 1e100: any D); with j_bound = +inf a finite J still survives
// and the mean's sum may round to +inf (never NaN: the terms are non-negative).
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mpct_dev.h"

namespace mpct {

constexpr double kRobustDefaultBound = 1e100;  // j_bound = 0

// per-candidate outputs (device pointers, any may be null)
struct RobustOut {
  double* mean;         // [C][my]
  double* worst;        // [C][my]
  int32_t* n_failed;    // [C]
  int32_t* worst_draw;  // [C]
  int32_t* status;      // [C]
};

// One wave, lanes 0..my-1 active in the sums (every lane may call; lanes >= my write nothing).
// j1(k, i): J1_i of draw k; st(k): its status.  Writes candidate c's record.
template <class FJ, class FS>
__device__ __forceinline__ void robust_reduce(int lane, int D, int my, double j_bound, FJ j1, FS st,
                                              const RobustOut& out, long long c) {
  const int i = lane < my ? lane : 0;
  int sor = 0, nfail = 0, nsurv = 0, wd = -1;
  double sum = 0.0, mx = 0.0, jw = 0.0;
  for (int k = 0; k < D; ++k) {
    const int s = st(k);
    sor |= s;
    double J = 0.0;
    for (int q = 0; q < my; ++q) J += j1(k, q);
    if (s == 0 && isfinite(J) && J <= j_bound) {
      const double v = j1(k, i);
      sum += v;
      mx = (nsurv == 0 || v > mx) ? v : mx;
      if (nsurv == 0 || J > jw) {
        jw = J;
        wd = k;
      }
      ++nsurv;
    } else {
      ++nfail;
    }
  }
  if (sor & (MPCT_ST_SKIPPED_ | MPCT_ST_BADHORIZON_)) {  // never simulated: not a failed draw
    nfail = 0;
    nsurv = 0;
    wd = -1;
  }
  if (lane < my) {
    if (out.mean) out.mean[c * my + lane] = nsurv ? sum / (double)nsurv : NAN;
    if (out.worst) out.worst[c * my + lane] = nsurv ? mx : NAN;
  }
  if (lane == 0) {
    if (out.n_failed) out.n_failed[c] = nfail;
    if (out.worst_draw) out.worst_draw[c] = wd;
    if (out.status) out.status[c] = sor;
  }
}

}  // namespace mpct
