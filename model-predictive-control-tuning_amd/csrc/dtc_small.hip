// dtc_small.hip — the DTC-GPC closed loop of small plants (WoodBerry
// with its plant-only disturbance and Monte-Carlo plant variants): one wavefront per simulation,
// every per-step quantity in a fixed lane layout, and no QP.
//
// DTC_GPC_WW.m is the unconstrained loop: deltaU = Km * (Ref - yf) (:149) with Km the first-move rows
// of K = (H'QH + W) \ H'Q (:98-105).  So a scenario in DTC mode whose move bounds are all infinite
// (what DTC_GPC_WW.m restates) needs, per step, only the nu first-move rows of the gain: no QP, no
// R^-1, no factor state.  The host marks such scenarios `small_dtc` (scenario_tables.h dtc_small_plant):
// DTC mode, my <= 2 outputs, nu <= 2 MVs, nu + nq <= 4 plant inputs (MVs and plant-only
// disturbances, no measured disturbances), every plant variant's, Pz's and Gz's entry <= 4 terms,
// filters Fr_i of <= 4 taps, y difference state <= 4 per output, past-control registers <= 8 per
// MV, cost-only batches.  Everything else runs gpc_closed_loop_kernel<MAXM, true, ...> unchanged.
//
// Lane layout (lane L = 16 k + e, e = 4 q + p), the gpc_small.hip scheme extended by the predictor:
//   * quads q = i < my: term k of plant entry (output i, input p) of this simulation's plant variant
//     (Monte-Carlo draw kref % nvar): a numerator tap b u_p(t - c) or a denominator tap -a y_e(t - c),
//     one LDS read from a history ring; input p >= nu is a plant-only disturbance (its ring is fed
//     from v);
//   * quad q = 2 + i: p = 0, 1 the model entries Pz(i, p), p = 2, 3 the dead-time-free Gz(i, p - 2)
//     (OptimalPredictor2.m: lsim(Pz, u), lsim(Gz, u) as recursions on the controller's own inputs).
//   One v_permlane16/32_swap sum over the four term rows gives every entry's output; one DPP stage
//   pairs them (Pz_i, Gz_i on lanes 8 + 4i, 10 + 4i) and a second sums each plant quad (y_i).
//   Output lane 4 i fetches Pz_i and Gz_i by DPP row shifts, runs the robustness filter
//   yfr = Fr_i (y_i - Pz_i) (mimofilter.m, coefficients in LDS) and drives the free response with
//   the predictor output yp = Gz_i + yfr (OptimalPredictor2.m:24-40) while the costs use y_i.
//   * dU(first moves) = Km x: lane (n, g), n < nu, quarter g of row n of the gain (quarter 0 the y
//   part, quarters 1..3 MV g - 1's past-control ring), 12 FMAs, one permlane sum: row n on lane n.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mpct_dev.h"
#include "wave_ops.h"
#include "gpc_prologue.h"
#include "gpc_record.h"
#include "dtc_step.h"

namespace mpct {

// waves per SIMD the launch bounds ask for, and the prologue's Householder block (gpc_prologue.h
// kHB): unbounded the <16> instance needs 119 VGPRs (four waves; 22.9 ms for config 4's 320,000
// simulations); five waves with 8-row blocks spill 80 B per lane in the prologue (21.3 ms, but 1.33 GB
// of scratch write-backs per evaluation against 10 MB of records); four waves with 4-row blocks fit
// 103 VGPRs without a spill: 21.5 ms and 10.2 MB written (profiles/r06i_dtc_prologue_ab.txt)
#ifndef MPCT_DTC_HB
#define MPCT_DTC_HB 4
#endif
#ifndef MPCT_DTC_W16
#define MPCT_DTC_W16 4
#endif
#ifndef MPCT_DTC_W32
#define MPCT_DTC_W32 3
#endif
template <int MAXM>
__global__ void __launch_bounds__(64, MAXM <= 16 ? MPCT_DTC_W16 : MPCT_DTC_W32)
    dtc_small_kernel(const DevScenario sc, long long C, int nref, const int* __restrict__ N2v,
                     const int* __restrict__ Nuv, const double* __restrict__ deltav,
                     const double* __restrict__ lambdav, const double* __restrict__ rv,
                     const double* __restrict__ vv, const int* __restrict__ perm, const DevOpts o,
                     const DevResult out, int mlo, int first) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  const long long slot = blockIdx.x;
  const long long S = C * nref;
  if (slot >= S) return;
  const long long cs = slot / nref;
  const int kref = (int)(slot - cs * nref);
  const long long c = perm ? (long long)perm[cs] : cs;
  const long long sim = c * nref + kref;
  const int my = sc.my, nu = sc.nu;
  const int N2 = N2v[c], Nu = Nuv[c];
  const int M = nu * Nu;
  auto write_nan = [&](int status) __attribute__((always_inline)) {
    put_record(out, slot, S, sim, my, nu, lane, NAN, NAN, NAN, NAN, status, 0);
  };
  if (N2 <= 0) {
    if (first) write_nan(MPCT_ST_SKIPPED_);
    return;
  }
  if (N2 > sc.n2max || Nu < 1 || Nu > sc.numax || Nu > N2) {
    if (first) write_nan(MPCT_ST_BADHORIZON_);
    return;
  }
  if (M <= mlo || M > MAXM) return;  // the other class launch simulates it
  const DtcLayout L = dtc_layout(sc, M);
  for (int e = lane; e < L.total - L.A; e += kWave) lds[L.A + e] = 0.0;  // gain pads, state, rings
  if (lane < 2 * 8) {  // filter coefficients: fb (taps 0..3), then fa (taps 0..3), zero-padded
    const int i = lane >> 3, k = lane & 7;
    lds[L.fr + lane] = i < my ? sc.sm_fr[i * 8 + k] : 0.0;
  }
  lds_sync();

  // ------------------------------------------------------------------ prologue (gpc_prologue.h):
  // the first-move rows of A only (row n = A row n Nu), no R^-1
  if (!gpc_prologue<MAXM, false, false, true, MPCT_DTC_HB>(sc, lane, M, Nu, N2, deltav + c * my, lambdav + c * nu, lds + L.R,
                                              nullptr, lds + L.A, kSmA, sc.sm_acol)) {
    write_nan(MPCT_ST_NONFINITE_);
    return;
  }

  // ------------------------------------------------------------------ the closed loop (dtc_step.h)
  double j1, j22;
  dtc_closed_loop<false>(sc, lds, L, lane, kref, rv, vv, j1, j22);

  // ------------------------------------------------------------------ results (lane i <- lane 4 i)
  const double j1o = __shfl(j1, (lane & 3) * 4, kWave);
  const double j22o = __shfl(j22, (lane & 3) * 4, kWave);
  int st = 0;
  if (lane < my && !isfinite(j1o)) st |= MPCT_ST_NONFINITE_;
  const unsigned long long nf = __ballot(st & MPCT_ST_NONFINITE_);
  put_record(out, slot, S, sim, my, nu, lane, j1o, NAN, j22o, NAN, nf ? MPCT_ST_NONFINITE_ : 0, 0);
}

}  // namespace mpct

// ------------------------------------------------------------------------------------------
// host-side launch
#include <string>

namespace mpct {

long long dtc_small_lds_bytes(const DevScenario& sc, int M) { return (long long)dtc_layout(sc, M).total * 8; }

// one QP-size class (M <= 16 or 16 < M <= 32) of a cost-only batch on a small_dtc scenario
// (launch_closed_loop); first: this launch also writes the statuses of skipped / bad-horizon candidates
int launch_dtc_small(const DevScenario& sc, int cls, long long C, int nref, const int* N2, const int* Nu,
                     const double* delta, const double* lambda, const double* r, const double* v, const DevOpts& o,
                     const DevResult& out, const int* perm, int mlo, int first, hipStream_t stream, std::string* err) {
  const int nu_cls = sc.numax < cls / sc.nu ? sc.numax : cls / sc.nu;
  const long long lds = dtc_small_lds_bytes(sc, sc.nu * nu_cls);
  const long long S = C * nref;
  if (cls == 16)
    hipLaunchKernelGGL(dtc_small_kernel<16>, dim3((unsigned)S), dim3(kWave), (size_t)lds, stream, sc, C, nref, N2, Nu,
                       delta, lambda, r, v, perm, o, out, mlo, first);
  else
    hipLaunchKernelGGL(dtc_small_kernel<32>, dim3((unsigned)S), dim3(kWave), (size_t)lds, stream, sc, C, nref, N2, Nu,
                       delta, lambda, r, v, perm, o, out, mlo, first);
  hipError_t e = hipGetLastError();
  if (e != hipSuccess) {
    *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
    return -3;
  }
  return 0;
}

}  // namespace mpct
