// segment_indices.h — step-response indices per setpoint segment of stored trajectories: one record per
// (output row, segment) and per (input row, segment), reduced on the device
// (mpct_segment_indices_device / mpct_eval_segment_indices, include/mpct.h).  Kernel in
// segment_indices.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr int kSegWaves = 4;  // waves (units) of one workgroup
constexpr int kSegMax = 16;   // MPCT_SEG_MAX

// the call's parameters, by value in the kernel argument: the nseg + 1 boundaries, the base rule, the band
// and the rise levels
struct SegParams {
  int nseg, base;
  int tseg[kSegMax + 1];
  double band_rel, band_abs, rise_lo, rise_hi;
};

// device pointers, any may be null; the first ten are [S][my][nseg], the last five [S][nu][nseg]
struct SegOut {
  double* iae;
  double* ise;
  double* itae;
  double* emax;
  int* t_emax;
  double* over;
  double* under;
  double* e_final;
  int* settle;
  int* rise;
  double* tv;
  double* du2;
  double* dumax;
  double* u_lo;
  double* u_hi;
  bool any_y() const { return iae || ise || itae || emax || t_emax || over || under || e_final || settle || rise; }
  bool any_u() const { return tv || du2 || dumax || u_lo || u_hi; }
  // the records of simulation s0 onwards
  SegOut from(long long s0, int my, int nu, int nseg) const {
    const long long a = s0 * my * nseg, b = s0 * nu * nseg;
    auto d = [](double* p, long long o) { return p ? p + o : nullptr; };
    auto i = [](int* p, long long o) { return p ? p + o : nullptr; };
    return SegOut{d(iae, a),     d(ise, a),    d(itae, a), d(emax, a), i(t_emax, a), d(over, a), d(under, a), d(e_final, a),
                  i(settle, a),  i(rise, a),   d(tv, b),   d(du2, b),  d(dumax, b),  d(u_lo, b), d(u_hi, b)};
  }
};

// One wave per unit (row, segment), the segment fastest: units 0 .. ny-1 are the output units
// (s, i, g) = (unit / nseg / my, unit / nseg % my, unit % nseg) when an output field is asked for
// (ny = S * my * nseg, else 0), the next S * nu * nseg the input units.  y [S][my][nit], u [S][nu][nit],
// r [nref][my][nit]; simulation s reads reference set s % nref.
__global__ void __launch_bounds__(64 * kSegWaves)
    segment_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                           long long ny, long long nunits, int nref, int my, int nu, int nit, SegParams p, SegOut out);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked
// (1 <= nseg <= kSegMax, 0 <= tseg[0] < .. < tseg[nseg] <= nit).
int launch_segment_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu,
                           int nit, const SegParams& p, const SegOut& out, hipStream_t stream, std::string* err);

}  // namespace mpct
