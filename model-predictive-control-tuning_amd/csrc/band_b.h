// band_b.h — the band kernel's second QP factor B = R_A^-1 (mdband_kernel.hip): its packed index,
// gi_add's hook that appends a column, the two products over the active set, the wave prefix sum and
// the drop that takes its rotations from B's own row, and the kernel's active-row marks.  A header of
// its own so that tests/device_units/band_probe.hip reaches the code one update at a time.
#pragma once
#include "gi_core.h"

namespace mpct {

// B = R_A^-1 of the band kernel, in R_A's packed layout (gi_core.h RAPacked: column
// k holds rows 0..k+1).  Entry (k + 1, k) is kept zero on the active block, and bt_mul / bt_tmul
// read it in place of every entry below the stored ones.
__device__ __forceinline__ int bt_idx(int w, int k) { return (int)(__umul24((unsigned)k, (unsigned)(k + 3)) >> 1) + w; }
// gi_add's hook: column q = [-r / alpha; 1 / alpha] (r = R_A^-1 d(0:q), the iteration's dual
// direction), the stored entries below the diagonal next to it zeroed
struct BandBAdd {
  double* bt;
  double r;  // this lane's r_w
  __device__ __forceinline__ void add(int q, double ia) const {
    const int lane = threadIdx.x;
    if (lane < q) bt[bt_idx(lane, q)] = -r * ia;
    else if (lane == q) bt[bt_idx(q, q)] = ia;
    if (lane == q && q > 0) bt[bt_idx(q, q - 1)] = 0.0;
    if (lane == q + 1) bt[bt_idx(q + 1, q)] = 0.0;
  }
};
// lane w < q: sum_{k < q} B(w,k) c_k, c in LDS
__device__ __forceinline__ double bt_mul(const double* bt, const double* c, int q) {
  const int lane = threadIdx.x;
  double r0 = 0.0, r1 = 0.0;
  if (lane < q) {
    auto b = [&](int k) __attribute__((always_inline)) { return bt[bt_idx(min(lane, k + 1), k)]; };
    int k = 0;
    for (; k + 3 < q; k += 4) {
      const double b0 = b(k), b1 = b(k + 1), b2 = b(k + 2), b3 = b(k + 3);
      const double c0 = c[k], c1 = c[k + 1], c2 = c[k + 2], c3 = c[k + 3];
      r0 = fma(b0, c0, r0);
      r1 = fma(b1, c1, r1);
      r0 = fma(b2, c2, r0);
      r1 = fma(b3, c3, r1);
    }
    for (; k < q; ++k) r0 = fma(b(k), c[k], r0);
  }
  return r0 + r1;
}
// lane v < q: (B'c)_v = sum_{k < q} B(k,v) c_k, i.e. w with R_A'w = c
__device__ __forceinline__ double bt_tmul(const double* bt, const double* c, int q) {
  const int lane = threadIdx.x;
  double r0 = 0.0, r1 = 0.0;
  if (lane < q) {
    const double* col = bt + bt_idx(0, lane);
    auto b = [&](int k) __attribute__((always_inline)) { return col[min(k, lane + 1)]; };
    int k = 0;
    for (; k + 3 < q; k += 4) {
      const double b0 = b(k), b1 = b(k + 1), b2 = b(k + 2), b3 = b(k + 3);
      const double c0 = c[k], c1 = c[k + 1], c2 = c[k + 2], c3 = c[k + 3];
      r0 = fma(b0, c0, r0);
      r1 = fma(b1, c1, r1);
      r0 = fma(b2, c2, r0);
      r1 = fma(b3, c3, r1);
    }
    for (; k < q; ++k) r0 = fma(b(k), c[k], r0);
  }
  return r0 + r1;
}
// inclusive prefix sum over the wave's lanes: DPP row_shr within each 16-lane row, then the row
// totals (readlane) carried into the rows above
__device__ __forceinline__ double wave_prefix_sum(double v) {
  const int i = threadIdx.x & 15, b = threadIdx.x >> 4;
  double t;
  t = dppd<0x111>(v); if (i >= 1) v += t;
  t = dppd<0x112>(v); if (i >= 2) v += t;
  t = dppd<0x114>(v); if (i >= 4) v += t;
  t = dppd<0x118>(v); if (i >= 8) v += t;
  const double t0 = bcast(v, 15), t1 = bcast(v, 31), t2 = bcast(v, 47);
  if (b >= 1) v += t0;
  if (b >= 2) v += t1;
  if (b >= 3) v += t2;
  return v;
}
// remove active constraint kd with B alone.  R_A E (column kd removed) is re-triangularised by
// rotations G on rows (jj, jj + 1), jj = kd..q-2; then B_new = (B G')[rows != kd, columns < q-1],
// which is upper triangular exactly when G turns B's row kd into a multiple of e_{q-1} (row kd of
// B G' times R_new = row kd of E = 0).  So rotation jj zeroes the running entry x of row kd against
// y = B(kd, jj + 1): cs = y / r, sn = -x / r, r = |row kd (kd..jj+1)|, all from one prefix sum of
// B(kd, .)^2 -- no serial chain of LDS round trips (the R_A form's rsq + RMW + lds_sync per
// rotation).  The same rotations go to J's columns; each lane then sweeps its row of J and of B
// through them with the running entry in a register, writing B's rows kd + 1.. one row up.
// The same factorisation as the R_A form up to the signs of R_new's rows (Givens QR is unique up
// to them), which J and B carry consistently.  cs / sn are staged in sc_ / ss_ (Mz doubles each).
template <int MAXM, class Mark>
__device__ __forceinline__ void band_drop_b(GIState<MAXM>& S, double* sJT, double* bt, int Mz, int kd,
                                            const Mark& mark, double* sc_, double* ss_) {
  const int lane = threadIdx.x;
  const int q = S.q;
  const int idk = __builtin_amdgcn_readlane(S.ww, kd);
  mark(S, idk, false);
  {
    const double un = lane_next<MAXM>(S.uw);
    const int wn = lane_next_i<MAXM>(S.ww);
    if (lane >= kd && lane < q - 1) {
      S.uw = un;
      S.ww = wn;
    }
  }
  // rotation parameters: lane jj in [kd, q-2]
  const double y = (lane >= kd && lane < q) ? bt[bt_idx(kd, lane)] : 0.0;
  const double s2 = wave_prefix_sum(y * y);  // lane j: |B(kd, kd..j)|^2
  const double yn = lane_next<MAXM>(y), r2 = lane_next<MAXM>(s2);
  if (lane >= kd && lane < q - 1) {
    const double x = lane == kd ? y : (s2 > 0.0 ? s2 * rsq_nr(s2) : 0.0);
    double cs = 1.0, sn = 0.0;
    if (r2 > 0.0) {
      const double ri = rsq_nr(r2);
      cs = yn * ri;
      sn = -x * ri;
    }
    sc_[lane] = cs;
    ss_[lane] = sn;
  }
  lds_sync();
  // J's columns (lanes = rows of J) and B's rows by slot (lanes = rows w < q)
  const bool jrow = lane < Mz, brow = lane < q;
  double cj = jrow ? sJT[kd * Mz + lane] : 0.0;
  double cb = (brow && lane <= kd + 1) ? bt[bt_idx(lane, kd)] : 0.0;
  const int wdst = lane > kd ? lane - 1 : lane;  // B's row kd leaves: rows below move up one
  for (int jj = kd; jj < q - 1; ++jj) {
    const double cs = sc_[jj], sn = ss_[jj];
    const double nj = jrow ? sJT[(jj + 1) * Mz + lane] : 0.0;
    const double nb = (brow && lane <= jj + 2) ? bt[bt_idx(min(lane, jj + 2), jj + 1)] : 0.0;
    if (jrow) sJT[jj * Mz + lane] = cs * cj + sn * nj;
    const double vb = cs * cb + sn * nb;
    if (brow && lane != kd && wdst <= jj + 1) bt[bt_idx(wdst, jj)] = vb;
    cj = -sn * cj + cs * nj;
    cb = -sn * cb + cs * nb;
  }
  if (jrow) sJT[(q - 1) * Mz + lane] = cj;
  const int qn = q - 1;
  if (lane == qn) {
    S.uw = 0.0;
    S.ww = -1;
  }
  S.nrot += q - 1 - kd;
  S.q = qn;
  lds_sync();
}

// active flags: box rows (p < 4*Mz) in the lanes' act bits, output rows in the LDS bitmap
struct BandMark {
  unsigned* bits;
  int base;
  template <class St>
  __device__ __forceinline__ void operator()(St& S, int p, bool on) const {
    if (p < base) {
      BoxMark{}(S, p, on);
    } else if (threadIdx.x == 0) {
      const int q = p - base;
      if (on) bits[q >> 5] |= 1u << (q & 31);
      else bits[q >> 5] &= ~(1u << (q & 31));
    }
  }
};

}  // namespace mpct
