// draw_stats.h — statistics of a [C][D][m] table over its draw axis, one record per column (c, i)
// (mpct_draw_stats_device / mpct_eval_robust_indices, include/mpct.h): survivor count,
// mean, smallest and largest surviving value with their draws, and the type-1 quantiles / tail means of
// robust_tail.h at up to kTailMaxLevels levels.  Kernels in draw_stats.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "robust_tail.h"

namespace mpct {

constexpr int kStatF64 = 0, kStatI32 = 1;   // MPCT_STAT_F64, MPCT_STAT_I32
constexpr int kStatMaxWaves = 4;            // columns (waves) of one workgroup, at most
constexpr int kStatLdsBytes = 64 * 1024;    // LDS of one workgroup, at most: its waves' slices of 12 B per draw
constexpr int kStatGridCap = 1 << 20;       // workgroups of one launch, at most; beyond it they stride

// device pointers, any may be null.  Column (c, i) of the table writes element o = c * ldo + off + i of the
// first six and elements o * nlev + j of the last three
struct DrawStatsOut {
  int32_t* n;
  double* mean;
  double* lo;
  int32_t* lo_draw;
  double* hi;
  int32_t* hi_draw;
  double* quantile;
  double* cvar;
  int32_t* q_draw;
  __host__ __device__ bool any() const { return n || mean || lo || lo_draw || hi || hi_draw || quantile || cvar || q_draw; }
  __host__ __device__ bool any_level() const { return quantile || cvar || q_draw; }
  // the records of output row r0 onwards (rows of ldo elements)
  DrawStatsOut from(long long r0, int ldo, int nlev) const {
    const long long a = r0 * ldo, b = a * nlev;
    auto d = [](double* p, long long o) { return p ? p + o : nullptr; };
    auto i = [](int32_t* p, long long o) { return p ? p + o : nullptr; };
    return DrawStatsOut{i(n, a), d(mean, a), d(lo, a), i(lo_draw, a), d(hi, a), i(hi_draw, a),
                        d(quantile, b), d(cvar, b), i(q_draw, b)};
  }
};

// waves of one workgroup at D draws: as many slices as kStatLdsBytes holds, 1 .. kStatMaxWaves
inline int draw_stats_waves(int D) {
  const int w = (int)(kStatLdsBytes / robust_tail_lds_bytes(D));
  return w < 1 ? 1 : (w > kStatMaxWaves ? kStatMaxWaves : w);
}

// x [C][D][m] of doubles (kStatF64) or int32 (kStatI32), alive [C][D] or null; D <= kTailMaxDraws,
// 0 <= nlev <= kTailMaxLevels, C * m <= 2^31 - 1 (the callers check).  levels on the host.  The record of
// column (c, i) goes to row c, element off + i of output rows of ldo elements.  grid_cap: 0 = kStatGridCap.
// All pointers device pointers, enqueued on `stream`, not synchronised.
int launch_draw_stats(const void* x, int x_type, const int* alive, long long C, int D, int m, int nlev,
                      const double* levels, const DrawStatsOut& out, int ldo, int off, int grid_cap, hipStream_t stream,
                      std::string* err);

// alive[c][k] of C candidates x D draws by the rule of robust_reduce.h: status 0, J = sum_i J1_i finite
// (summed over i = 0 .. my-1 in that order) and J <= j_bound; a candidate carrying MPCT_ST_SKIPPED or
// MPCT_ST_BADHORIZON on any draw has no live draw.  j_bound is the bound itself (never 0 = default here).
int launch_draw_alive(long long C, int D, int my, double j_bound, const double* J1, const int* status, int* alive,
                      hipStream_t stream, std::string* err);

}  // namespace mpct
