// dtc_robust.h — constants and host-side launch interface of dtc_robust.hip (robust scoring over
// plant draws: the fused small_dtc kernel, the generic reduction, the tail statistics).
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "mpct_dev.h"
#include "robust_reduce.h"
#include "robust_tail.h"

namespace mpct {

constexpr int kRobustW = 4;       // waves of one candidate's workgroup (one per SIMD of a CU)
constexpr int kRecW = 3;          // draw record in LDS: J1_0, J1_1, status (small_dtc: my <= 2)
constexpr int kRobustMaxD = 128;  // draws the fused kernel's LDS record array holds (3 KB); more: generic path

struct LaunchFan;

// the fused path serves this scenario at D draws
inline bool dtc_robust_eligible(const DevScenario& sc, int D) {
  return sc.small_dtc && sc.my <= kRecW - 1 && sc.nu * sc.numax <= 32 && D <= kRobustMaxD;
}

int launch_robust_reduce(long long C, int D, int my, double j_bound, const double* J1, const int* status,
                         const RobustOut& out, hipStream_t stream, std::string* err);
int launch_robust_tail(long long C, int D, int my, double j_bound, const double* J1, const int* status, int nlev,
                       const double* levels, const TailOut& out, hipStream_t stream, std::string* err);
long long dtc_robust_lds_bytes(const DevScenario& sc, int M, int D);
int launch_dtc_robust(const DevScenario& sc, long long C, int D, const int* N2, const int* Nu, const double* delta,
                      const double* lambda, const double* r, const double* v, const int* perm, int* lists,
                      double j_bound, const RobustOut& out, double* J1, int ncu, LaunchFan* fan, hipStream_t stream,
                      std::string* err);

}  // namespace mpct
