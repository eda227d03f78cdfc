// dtc_step.h — one closed loop of the DTC-GPC small-plant scheme (dtc_small.hip's lane layout): the
// LDS layout of one simulation and the step loop from a zeroed state to the costs.  Shared by
// dtc_small_kernel (one wave per simulation) and dtc_robust_kernel (dtc_robust.hip: one workgroup
// per candidate, every wave walking its share of the plant draws), so both run the same loop.
#pragma once
#include <hip/hip_runtime.h>
#include <math.h>

#include "mpct_dev.h"
#include "wave_ops.h"

namespace mpct {

// LDS layout of one simulation (doubles): R (the prologue's M x M scratch), the first-move rows of
// the gain, the y part of x, the past-control rings (two copies each), the input rings [4][kSmU] |
// the entry output rings [16][ke] (from kDtcEOff), the filters' coefficients [my][8] (fb 0..3,
// fa 0..3) and their input / output rings [my][2][4]: 4.6 KB at M = 16 (Shell-sized plants).
// R, A and fr depend on the candidate only; xy, ring, hist and frh are the state of one loop
// (dtc_state_doubles of them, contiguous from xy when laid out by dtc_state_layout)
struct DtcLayout {
  int R, A, xy, ring, hist, fr, frh, total;
};
__host__ __device__ inline DtcLayout dtc_layout(const DevScenario& sc, int M) {
  DtcLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 1) & ~1; return r; };
  L.R = take(M * M);
  L.A = take(2 * kSmA);
  L.xy = take(kSmY);
  L.ring = take(3 * 2 * kSmR);  // three MVs' worth: the product's quarter 3 reads zeros for nu = 2
  L.hist = take(kDtcEOff + 16 * sc.sm_ke);
  L.fr = take(2 * 8);
  L.frh = take(2 * 2 * 4);
  L.total = (o + 1) & ~1;
  return L;
}

// the per-loop state alone (xy | ring | hist | frh), laid out from `base`; R, A and fr are set by
// the caller.  L.total is the first double after the state
__host__ __device__ inline DtcLayout dtc_state_layout(const DevScenario& sc, int base) {
  DtcLayout L;
  int o = base;
  auto take = [&](int n) { int r = o; o += (n + 1) & ~1; return r; };
  L.R = L.A = L.fr = 0;
  L.xy = take(kSmY);
  L.ring = take(3 * 2 * kSmR);
  L.hist = take(kDtcEOff + 16 * sc.sm_ke);
  L.frh = take(2 * 2 * 4);
  L.total = o;
  return L;
}

// opaque lane id: predicates derived from it are recomputed where used, not kept live across the
// step loop (gpc_small.hip sm_lane).  MULTI: the workgroup holds several waves
template <bool MULTI>
__device__ __forceinline__ int dtc_lane() {
  int l = MULTI ? (int)(threadIdx.x & (kWave - 1)) : (int)threadIdx.x;
  asm volatile("" : "+v"(l));
  return l;
}

// One closed loop of nit steps: reference set / plant variant `kref`, gain rows at L.A, filter
// coefficients at L.fr, state (zeroed by the caller) at L.xy / L.ring / L.hist / L.frh.  Lane 4 i
// returns J1_i in j1 and j22_i in j22.  Every LDS hand-off is within the calling wave (lds_sync);
// A and fr are only read
template <bool MULTI>
__device__ __forceinline__ void dtc_closed_loop(const DevScenario& sc, double* lds, const DtcLayout& L, int lane,
                                                int kref, const double* __restrict__ rv,
                                                const double* __restrict__ vv, double& j1out, double& j22out) {
  const int my = sc.my, nu = sc.nu, nit = sc.nit;
  // per-lane constants of the step loop: this lane's term of this simulation's plant variant
  const int pv = sc.nvar > 1 ? (kref % sc.nvar) * kWave : 0;
  const double pcoef = sc.sm_coef[pv + lane];
  const int pbase = L.hist + sc.sm_hoff[pv + lane];
  const int pc = sc.sm_hc[pv + lane], pmask = sc.sm_hmask[pv + lane];
  const int ke = sc.sm_ke;
  const int oi = (lane >> 2) & 3;  // output lane 4 i
  const int yoff = oi < my ? sc.yoff[oi] : 0;
  const int nyh = oi < my ? sc.nyhi[oi] : 0;
  const int qm = lane & 15, qg = lane >> 4;  // product lane (n, g)
  const int aoff = L.A + qm * kSmA + (qg ? kSmY + kSmR * (qg - 1) : 0);
  const int xoff = qg ? L.ring + 2 * kSmR * (qg - 1) : L.xy;
  const int ink0 = sc.ink0;
  const int nq = sc.nd;  // ring-fed plant inputs: the plant-only disturbances (no MDs here)
  const double* rr = rv + (long long)kref * my * nit;
  const int si = oi < my ? oi : my - 1;
  const double* psr = rr + (long long)si * nit;
  const double* psy = sc.yref + (long long)si * nit;
  // lane nu + k < nu + nq: disturbance k of this simulation's signal set
  const int qk = lane - nu < nq && lane >= nu ? lane - nu : 0;
  const double* psq = vv ? vv + ((long long)kref * nq + qk) * nit : nullptr;
  double yd0 = 0.0;    // lane 4 i: yp_i(t - 1)
  double uprev = 0.0;  // lane n < nu: u_n(t - 1)
  double j1 = 0.0, j22 = 0.0;
  double r_t = psr[0], yr_t = psy[0];
  double q_t = psq ? psq[0] : 0.0;
  __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0): per-lane constants land before the loop

  for (int t = 0; t < nit; ++t) {
    // the disturbances known at t (DTC_GPC_WW.m:123-132: the plant sees q(t)), then the hand-off of
    // step t - 1's rings to this step's terms
    {
      const int l = dtc_lane<MULTI>();
      if (l >= nu && l < nu + nq) lds[L.hist + l * kSmU + (t & (kSmU - 1))] = q_t;
    }
    const int tn = t + 1 < nit ? t + 1 : t;
    const double q_n = psq ? psq[tn] : 0.0;
    lds_sync();
    // ---- plant entries, Pz and Gz: one term per lane, summed over the four term rows
    const double hv = lds[pbase + ((t - pc) & pmask)];
    const double o1e = lds[L.xy + yoff + 1], o2e = lds[L.xy + yoff + 2];
    const double ye = row4_sum(pcoef * hv);  // entry e's output on lane e of every row
    const double s1 = ye + dppd<kQx1>(ye);  // pair sums: Pz_i on lane 8 + 4i, Gz_i on lane 10 + 4i
    const double yq = s1 + dppd<kQx2>(s1);  // quad sums: y_i on the lanes of quad i < my
    const double pz = dppd<0x108>(s1);      // row_shl:8  -> lane 4i holds Pz_i
    const double gz = dppd<0x10A>(s1);      // row_shl:10 -> lane 4i holds Gz_i
    if (dtc_lane<MULTI>() < 16) lds[L.hist + kDtcEOff + dtc_lane<MULTI>() * ke + (t & (ke - 1))] = ye;
    // ---- predictor, y update and costs (lane 4 i)
    {
      const int l = dtc_lane<MULTI>();
      if ((l & ~12) == 0 && (l >> 2) < my) {
        const int i = l >> 2;
        // yfr = Fr_i (y - Pz_i): zero-padded taps, the general kernel's order (fb taps, then fa)
        const double* fb = lds + L.fr + i * 8;
        double* eh = lds + L.frh + i * 8;  // eM ring [4], then the filter output ring [4]
        double* fh = eh + 4;
        const double em = yq - pz;
        eh[t & 3] = em;
        double yfr = 0.0;
        yfr = fma(fb[0], em, yfr);
        yfr = fma(fb[1], eh[(t - 1) & 3], yfr);
        yfr = fma(fb[2], eh[(t - 2) & 3], yfr);
        yfr = fma(fb[3], eh[(t - 3) & 3], yfr);
        yfr = fma(-fb[5], fh[(t - 1) & 3], yfr);
        yfr = fma(-fb[6], fh[(t - 2) & 3], yfr);
        yfr = fma(-fb[7], fh[(t - 3) & 3], yfr);
        fh[t & 3] = yfr;
        const double ym = gz + yfr;
        double* xs = lds + L.xy + yoff;
        const double n1 = ym - yd0, n2 = n1 - o1e, n3 = n2 - o2e;
        xs[0] = ym - r_t;
        if (nyh > 1) xs[1] = n1;
        if (nyh > 2) xs[2] = n2;
        if (nyh > 3) xs[3] = n3;
        yd0 = ym;
        const double e1 = yq - yr_t;  // the costs use the plant output
        j1 = fma(e1, e1, j1);
        if (t >= ink0) j22 = fma(e1, e1, j22);
      }
    }
    const double r_n = psr[tn], yr_n = psy[tn];
    lds_sync();  // y state -> product
    // ---- first moves dU = Km x: quarter 0 the y part, quarters 1..3 the MV rings
    double du;
    {
      const int h = (1 - t) & (kSmR - 1);
      const int xo = xoff + (dtc_lane<MULTI>() >= 16 ? h : 0);
      const double2* av = reinterpret_cast<const double2*>(lds + aoff);
      const double* xv = lds + xo;
      double a0 = 0.0, a1 = 0.0;
      if ((dtc_lane<MULTI>() & 15) < nu) {
#pragma unroll
        for (int p = 0; p < kSmR / 2; ++p) {
          const double2 a = av[p];
          a0 = fma(a.x, xv[2 * p], a0);
          a1 = fma(a.y, xv[2 * p + 1], a1);
        }
        if (dtc_lane<MULTI>() < 16) {
#pragma unroll
          for (int p = kSmR / 2; p < kSmY / 2; ++p) {
            const double2 a = av[p];
            a0 = fma(a.x, xv[2 * p], a0);
            a1 = fma(a.y, xv[2 * p + 1], a1);
          }
        }
      }
      du = row4_sum(a0 + a1);  // first move of MV n on lane n
    }
    // ---- u update (lane n < nu): plant input ring, past-control ring
    {
      const int l = dtc_lane<MULTI>();
      if (l < nu) {
        const double un = uprev + du;
        uprev = un;
        lds[L.hist + l * kSmU + (t & (kSmU - 1))] = un;
        double* ring = lds + L.ring + 2 * kSmR * l;
        const int p = (-t) & (kSmR - 1);
        ring[p] = du;
        ring[p + kSmR] = du;
      }
    }
    r_t = r_n;
    yr_t = yr_n;
    q_t = q_n;
  }
  j1out = j1;
  j22out = j22;
}

}  // namespace mpct
