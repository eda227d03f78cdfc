// osc_indices.h — oscillation indices per setpoint segment of stored trajectories: one record per
// (output row, segment) -- band crossings, decay ratio, period, last peak -- and per (input row, segment) --
// moves, direction reversals, last reversal -- reduced on the device
// (mpct_osc_indices_device / mpct_eval_osc_indices, include/mpct.h).  Kernel in osc_indices.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "segment_indices.h"  // kSegMax: the segments are those of the segment indices

namespace mpct {

constexpr int kOscWaves = 4;  // waves (units) of one workgroup

// the call's parameters, by value in the kernel argument: the nseg + 1 boundaries, the base rule, the band
// and the dead zone of a move
struct OscParams {
  int nseg, base;
  int tseg[kSegMax + 1];
  double band_rel, band_abs, rev_tol;
};

// device pointers, any may be null; the first four are [S][my][nseg], the last three [S][nu][nseg]
struct OscOut {
  int* ncross;
  double* decay;
  int* period;
  double* a_last;
  int* nmove;
  int* nrev;
  int* t_rev;
  bool any_y() const { return ncross || decay || period || a_last; }
  bool any_u() const { return nmove || nrev || t_rev; }
  // the records of simulation s0 onwards
  OscOut from(long long s0, int my, int nu, int nseg) const {
    const long long a = s0 * my * nseg, b = s0 * nu * nseg;
    auto d = [](double* p, long long o) { return p ? p + o : nullptr; };
    auto i = [](int* p, long long o) { return p ? p + o : nullptr; };
    return OscOut{i(ncross, a), d(decay, a), i(period, a), d(a_last, a), i(nmove, b), i(nrev, b), i(t_rev, b)};
  }
};

// One wave per unit (row, segment), the segment fastest: units 0 .. ny-1 are the output units
// (s, i, g) = (unit / nseg / my, unit / nseg % my, unit % nseg) when an output field is asked for
// (ny = S * my * nseg, else 0), the next S * nu * nseg the input units.  y [S][my][nit], u [S][nu][nit],
// r [nref][my][nit]; simulation s reads reference set s % nref.
__global__ void __launch_bounds__(64 * kOscWaves)
    osc_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                       long long ny, long long nunits, int nref, int my, int nu, int nit, OscParams p, OscOut out);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked
// (1 <= nseg <= kSegMax, 0 <= tseg[0] < .. < tseg[nseg] <= nit).
int launch_osc_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu,
                       int nit, const OscParams& p, const OscOut& out, hipStream_t stream, std::string* err);

}  // namespace mpct
