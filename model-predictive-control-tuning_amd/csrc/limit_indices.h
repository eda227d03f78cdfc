// limit_indices.h — limit indices of stored trajectories: band violation per output row (simulation x output),
// saturation and rate-limit use per input row (simulation x input), reduced on the device
// (mpct_limit_indices_device / mpct_eval_limit_indices, include/mpct.h).  Kernel in
// limit_indices.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr int kLimitWaves = 4;    // waves (rows) of one workgroup
constexpr int kLimitMaxCh = 32;   // MPCT_LIMIT_MAX_CH: output channels, input channels, each

// the call's parameters, by value in the kernel argument: 6 x 32 bounds (1,536 B), the tolerances and t0
struct LimitParams {
  double y_lo[kLimitMaxCh], y_hi[kLimitMaxCh];
  double u_lo[kLimitMaxCh], u_hi[kLimitMaxCh], du_lo[kLimitMaxCh], du_hi[kLimitMaxCh];
  double out_tol, sat_tol;
  int t0;
};

// device pointers, any may be null; the first seven are [S][my], the last six [S][nu]
struct LimitOut {
  double* viol;
  double* viol2;
  double* vmax;
  int* t_vmax;
  int* n_out;
  int* t_in;
  double* y_margin;
  int* n_lo;
  int* n_hi;
  int* n_rate;
  int* sat_run;
  double* u_margin;
  double* du_margin;
  bool any_y() const { return viol || viol2 || vmax || t_vmax || n_out || t_in || y_margin; }
  bool any_u() const { return n_lo || n_hi || n_rate || sat_run || u_margin || du_margin; }
  // the records of simulation s0 onwards
  LimitOut from(long long s0, int my, int nu) const {
    const long long a = s0 * my, b = s0 * nu;
    auto d = [](double* p, long long o) { return p ? p + o : nullptr; };
    auto i = [](int* p, long long o) { return p ? p + o : nullptr; };
    return LimitOut{d(viol, a), d(viol2, a), d(vmax, a), i(t_vmax, a), i(n_out, a),    i(t_in, a),    d(y_margin, a),
                    i(n_lo, b), i(n_hi, b),  i(n_rate, b), i(sat_run, b), d(u_margin, b), d(du_margin, b)};
  }
};

// One wave per row: rows 0 .. ny-1 are the output rows (s, i) = (row / my, row % my) when an output field is
// asked for (ny = S * my, else 0), the next S * nu the input rows.  y [S][my][nit], u [S][nu][nit].
__global__ void __launch_bounds__(64 * kLimitWaves)
    limit_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, long long ny, long long nrows, int my,
                         int nu, int nit, LimitParams p, LimitOut out);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked
// (my, nu <= kLimitMaxCh, 0 <= t0 < nit).
int launch_limit_indices(const double* y, const double* u, long long S, int my, int nu, int nit, const LimitParams& p,
                         const LimitOut& out, hipStream_t stream, std::string* err);

}  // namespace mpct
