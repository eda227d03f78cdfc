// envelope.h — trajectory envelopes over plant draws (mpct_envelope_device / mpct_eval_robust_envelope,
// include/mpct.h): stored trajectories y[S][rows][nit] with s = c * D + k are, as they lie in
// memory, the table x[C][D][m] of draw_stats.h with m = rows * nit, so the envelope of a side is that table's
// statistics over its draw axis, one record per sample (c, row, t), by the contract of draw_stats.h.  The
// spread reduces the lo / hi just written to one number per (c, row).  Kernels in envelope.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "draw_stats.h"

namespace mpct {

constexpr int kEnvMaxTile = 256;          // columns (lanes) of one workgroup, at most
constexpr int kEnvMinTile = 32;           // and at least: half a wave idles at the widest D
constexpr int kEnvLdsBytes = 32 * 1024;   // LDS of one workgroup while a tile of >= 64 columns fits it ..
constexpr int kEnvLdsMax = 64 * 1024;     // .. and at most, with kEnvMinTile columns
constexpr int kEnvGridCap = 1 << 20;      // workgroups of one launch, at most; beyond it they stride
constexpr int kEnvSpreadWaves = 4;        // rows (waves) of one workgroup of envelope_spread_kernel

// LDS of a tile with levels, 9 B per draw and column: the staged value and the draw of that rank (one byte)
__host__ __device__ inline size_t envelope_lds_bytes(int D, int tile) { return (size_t)D * tile * 9; }

// the most draws the lane kernel takes with levels: kEnvMinTile columns in kEnvLdsMax, and a draw in a byte
constexpr int kEnvLaneMaxDraws = kEnvLdsMax / (9 * kEnvMinTile) < 256 ? kEnvLdsMax / (9 * kEnvMinTile) : 256;  // 227

// the draws up to which mpct_envelope's levels run on the lane kernel; above it the host dispatches
// draw_stats_kernel on the same table.  Measured: the lane kernel takes 0.82 of draw_stats_kernel's
// time at D = 48 and 1.13 at D = 56, its ranking growing with D^2
constexpr int kEnvDefaultDlane = 48;

// columns of one workgroup at D draws with levels: the widest power of two that fits kEnvLdsBytes, at least
// kEnvMinTile.  Without levels the kernel needs no LDS and a tile is kEnvMaxTile columns
inline int envelope_tile(int D, bool levels) {
  if (!levels) return kEnvMaxTile;
  int t = kEnvMaxTile;
  while (t > kEnvMinTile && envelope_lds_bytes(D, t) > (size_t)kEnvLdsBytes) t >>= 1;
  return t;
}

// per (c, row) outputs of the spread (device pointers, any may be null), each [C][rows]
struct EnvSpreadOut {
  double* spread;
  double* spread_max;
  int32_t* t_spread_max;
  __host__ __device__ bool any() const { return spread || spread_max || t_spread_max; }
  EnvSpreadOut from(long long r0) const {
    return EnvSpreadOut{spread ? spread + r0 : nullptr, spread_max ? spread_max + r0 : nullptr,
                        t_spread_max ? t_spread_max + r0 : nullptr};
  }
};

// x [C][D][m] of doubles, alive [C][D] or null; the record of column (c, i) goes to element c * m + i (and
// (c * m + i) * nlev + j) of out.  With level outputs D <= kEnvLaneMaxDraws (the caller dispatches);
// 0 <= nlev <= kTailMaxLevels, C * m <= 2^31 - 1.  levels on the host.  grid_cap: 0 = kEnvGridCap.
// All pointers device pointers, enqueued on `stream`, not synchronised.
int launch_draw_envelope(const double* x, const int* alive, long long C, int D, int m, int nlev, const double* levels,
                         const DrawStatsOut& out, int grid_cap, hipStream_t stream, std::string* err);

// lo, hi [nrows][nit] as launch_draw_envelope wrote them -> the spread of each row over t = t0 .. nit - 1
int launch_envelope_spread(const double* lo, const double* hi, long long nrows, int nit, int t0, const EnvSpreadOut& out,
                           hipStream_t stream, std::string* err);

}  // namespace mpct
