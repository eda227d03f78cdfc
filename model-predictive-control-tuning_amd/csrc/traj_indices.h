// traj_indices.h — closed-loop performance indices of stored trajectories, one record per output row
// (simulation x output) and per input row (simulation x input), reduced on the device
// (mpct_indices_device / mpct_eval_indices, include/mpct.h).  Kernel in traj_indices.hip.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

namespace mpct {

constexpr int kIndexWaves = 4;                      // waves (rows) of one workgroup
constexpr long long kIndexMaxRows = 0x7fffffffLL;   // MPCT_INDEX_MAX_ROWS: S * my and S * nu, each

// the call's parameters, by value
struct IndexParams {
  int t0;
  double band_rel, band_abs;
};

// device pointers, any may be null; the first eight are [S][my], the last five [S][nu]
struct IndexOut {
  double* iae;
  double* ise;
  double* itae;
  double* emax;
  int* t_emax;
  double* over;
  double* e_final;
  int* settle;
  double* tv;
  double* du2;
  double* dumax;
  double* u_lo;
  double* u_hi;
  bool any_y() const { return iae || ise || itae || emax || t_emax || over || e_final || settle; }
  bool any_u() const { return tv || du2 || dumax || u_lo || u_hi; }
  // the records of simulation s0 onwards
  IndexOut from(long long s0, int my, int nu) const {
    const long long a = s0 * my, b = s0 * nu;
    auto d = [](double* p, long long o) { return p ? p + o : nullptr; };
    auto i = [](int* p, long long o) { return p ? p + o : nullptr; };
    return IndexOut{d(iae, a), d(ise, a), d(itae, a), d(emax, a), i(t_emax, a), d(over, a), d(e_final, a),
                    i(settle, a), d(tv, b), d(du2, b), d(dumax, b), d(u_lo, b), d(u_hi, b)};
  }
};

// One wave per row: rows 0 .. ny-1 are the output rows (s, i) = (row / my, row % my) when an output field is
// asked for (ny = S * my, else 0), the next S * nu the input rows.  y [S][my][nit], u [S][nu][nit],
// r [nref][my][nit]; simulation s reads reference set s % nref.
__global__ void __launch_bounds__(64 * kIndexWaves)
    traj_indices_kernel(const double* __restrict__ y, const double* __restrict__ u, const double* __restrict__ r,
                        long long ny, long long nrows, int nref, int my, int nu, int nit, IndexParams p, IndexOut out);

// All pointers device pointers, enqueued on `stream`, not synchronised; arguments already checked.
int launch_traj_indices(const double* y, const double* u, const double* r, long long S, int nref, int my, int nu, int nit,
                        const IndexParams& p, const IndexOut& out, hipStream_t stream, std::string* err);

}  // namespace mpct
