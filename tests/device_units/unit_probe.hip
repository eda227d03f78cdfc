// unit_probe.hip — test-only probes of the device headers wave_ops.h, gi_core.h, gpc_qp.h and
// gpc_qp16.h (included unmodified).  Each extern "C" entry takes host pointers, allocates, copies,
// launches one-wave workgroups (64 threads, dynamic LDS sized from M), synchronises, copies back,
// frees and returns the HIP error code.  Built into tests/device_units/libmpct_unit_probe.so by
// __graft_entry__.build_unit_probe(); never linked into libmpct.so.  The layouts of the arguments
// are documented in tests/qp_unit_ref.py (class Probe), which is the only caller.
#include <hip/hip_runtime.h>

#include <vector>

#include "wave_ops.h"
#include "gi_core.h"
#include "gpc_qp.h"
#include "gpc_qp16.h"

using namespace mpct;

namespace {

// ------------------------------------------------------------------------------------------------
// primitives.  Case c reads a = in_a[c][lane], b = in_b[c][lane], k = in_i[c][lane]; row4_sum4 takes
// its third and fourth operands from case (c + 1) % ncase.  Results: out_d[c][0..3][lane],
// out_i[c][lane].
enum {
  OP_BCAST = 0, OP_ROW_SUM, OP_ROW_MIN, OP_ROW_MIN_I, OP_ROW_ARGMIN,
  OP_PAIR_MIN16, OP_PAIR_MIN32, OP_PAIR_MIN_I16, OP_PAIR_MIN_I32, OP_PAIR_ARGMIN16, OP_PAIR_ARGMIN32,
  OP_WAVE_ARGMIN64, OP_ROW4_SUM, OP_ROW4_SUM2, OP_ROW4_SUM4, OP_WAVE_SUM64,
  OP_QSUM16, OP_QSUM64, OP_QARGMIN16_M1, OP_QARGMIN16_0, OP_QARGMIN16_2, OP_QARGMIN64,
  OP_LANE_NEXT16, OP_LANE_NEXT64, OP_LANE_PREV16, OP_LANE_PREV64, OP_LANE_NEXT_I16, OP_LANE_NEXT_I64,
  OP_BLOCK_PREFIX16, OP_BLOCK_PREFIX64, OP_RCP_NR, OP_RSQ_NR, OP_N,
  OP_ROW_BCAST16 = 100  // + k, k = 0..15
};

__global__ void __launch_bounds__(64) prim_kernel(int op, int ncase, const double* __restrict__ in_a,
                                                  const double* __restrict__ in_b, const int* __restrict__ in_i,
                                                  double* __restrict__ out_d, int* __restrict__ out_i) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x, c = blockIdx.x;
  const int c1 = (c + 1) % ncase;
  double a = in_a[c * 64 + lane], b = in_b[c * 64 + lane];
  double e = in_a[c1 * 64 + lane], f = in_b[c1 * 64 + lane];
  int k = in_i[c * 64 + lane];
  double r0 = 0.0, r1 = 0.0, r2 = 0.0, r3 = 0.0;
  int ri = 0;
  if (op >= OP_ROW_BCAST16 && op < OP_ROW_BCAST16 + 16) {
    switch (op - OP_ROW_BCAST16) {
      case 0: r0 = row_bcast16(a, 0); break;
      case 1: r0 = row_bcast16(a, 1); break;
      case 2: r0 = row_bcast16(a, 2); break;
      case 3: r0 = row_bcast16(a, 3); break;
      case 4: r0 = row_bcast16(a, 4); break;
      case 5: r0 = row_bcast16(a, 5); break;
      case 6: r0 = row_bcast16(a, 6); break;
      case 7: r0 = row_bcast16(a, 7); break;
      case 8: r0 = row_bcast16(a, 8); break;
      case 9: r0 = row_bcast16(a, 9); break;
      case 10: r0 = row_bcast16(a, 10); break;
      case 11: r0 = row_bcast16(a, 11); break;
      case 12: r0 = row_bcast16(a, 12); break;
      case 13: r0 = row_bcast16(a, 13); break;
      case 14: r0 = row_bcast16(a, 14); break;
      default: r0 = row_bcast16(a, 15); break;
    }
  } else {
    switch (op) {
      case OP_BCAST: r0 = bcast(a, __builtin_amdgcn_readfirstlane(k) & 63); break;
      case OP_ROW_SUM: r0 = row_sum(a); break;
      case OP_ROW_MIN: r0 = row_min(a); break;
      case OP_ROW_MIN_I: ri = row_min_i(k); break;
      case OP_ROW_ARGMIN: r0 = a; ri = k; row_argmin(r0, ri); break;
      case OP_PAIR_MIN16: r0 = pair_min<false>(a); break;
      case OP_PAIR_MIN32: r0 = pair_min<true>(a); break;
      case OP_PAIR_MIN_I16: ri = pair_min_i<false>(k); break;
      case OP_PAIR_MIN_I32: ri = pair_min_i<true>(k); break;
      case OP_PAIR_ARGMIN16: r0 = a; ri = k; pair_argmin<false>(r0, ri); break;
      case OP_PAIR_ARGMIN32: r0 = a; ri = k; pair_argmin<true>(r0, ri); break;
      case OP_WAVE_ARGMIN64: r0 = a; ri = k; wave_argmin64(r0, ri); break;
      case OP_ROW4_SUM: r0 = row4_sum(a); r1 = row4_sum(b); r2 = row4_sum(e); r3 = row4_sum(f); break;
      case OP_ROW4_SUM2: r0 = a; r1 = b; row4_sum2(r0, r1); break;
      case OP_ROW4_SUM4: r0 = a; r1 = b; r2 = e; r3 = f; row4_sum4(r0, r1, r2, r3); break;
      case OP_WAVE_SUM64: r0 = wave_sum64(a); break;
      case OP_QSUM16: r0 = qsum<16>(a); break;
      case OP_QSUM64: r0 = qsum<64>(a); break;
      case OP_QARGMIN16_M1: r0 = a; ri = k; qargmin<16>(r0, ri); break;
      case OP_QARGMIN16_0: r0 = a; ri = k; qargmin<16>(r0, ri, 0); break;
      case OP_QARGMIN16_2: r0 = a; ri = k; qargmin<16>(r0, ri, 2); break;
      case OP_QARGMIN64: r0 = a; ri = k; qargmin<64>(r0, ri); break;
      case OP_LANE_NEXT16: r0 = lane_next<16>(a); break;
      case OP_LANE_NEXT64: r0 = lane_next<64>(a); break;
      case OP_LANE_PREV16: r0 = lane_prev<16>(a); break;
      case OP_LANE_PREV64: r0 = lane_prev<64>(a); break;
      case OP_LANE_NEXT_I16: ri = lane_next_i<16>(k); break;
      case OP_LANE_NEXT_I64: ri = lane_next_i<64>(k); break;
      case OP_BLOCK_PREFIX16:
      case OP_BLOCK_PREFIX64: {
        // k = l | Nu << 8 | M << 16 (Nu and M wave-uniform)
        const int l = min(k & 255, lane);  // block_prefix<64> reads sxc[lane - l ..]
        const int Nu = (__builtin_amdgcn_readfirstlane(k) >> 8) & 255;
        const int M = (__builtin_amdgcn_readfirstlane(k) >> 16) & 255;
        if (op == OP_BLOCK_PREFIX16) r0 = block_prefix<16>(a, l, Nu, lane < M, nullptr);
        else r0 = block_prefix<64>(a, l, Nu, lane < M, lds);
        break;
      }
      case OP_RCP_NR: r0 = rcp_nr(a); break;
      case OP_RSQ_NR: r0 = rsq_nr(a); break;
      default: break;
    }
  }
  double* od = out_d + (long long)c * 256;
  od[lane] = r0;
  od[64 + lane] = r1;
  od[128 + lane] = r2;
  od[192 + lane] = r3;
  out_i[c * 64 + lane] = ri;
}

// ------------------------------------------------------------------------------------------------
// the QP rows' constraint data as the kernels set it (gpc_kernel.hip, gpc_small.hip): qrow = the
// lane's QP row, bnd = [4][nu] dmin, dmax, umin, umax
__device__ __forceinline__ RowCons row_cons(int qrow, int M, int Nu, int nu, const double* bnd) {
  RowCons rc;
  rc.n = qrow < M ? qrow / Nu : 0;
  rc.l = qrow < M ? qrow - rc.n * Nu : 0;
  rc.dmin = bnd ? bnd[rc.n] : 0.0;
  rc.dmax = bnd ? bnd[nu + rc.n] : 0.0;
  rc.umin = bnd ? bnd[2 * nu + rc.n] : 0.0;
  rc.umax = bnd ? bnd[3 * nu + rc.n] : 0.0;
  rc.bnd = nullptr;
  return rc;
}

struct FactorOut {
  double *J, *RA, *B, *lane_d;  // per entry: J [M*M | 256], R_A [rasz], B [256], [3][64] rdg, uw, backsub
  int *lane_i, *scal;           // per entry: [2][64] ww, act; [2] q, nrot
  double* beta;                 // per entry: [2] beta, |d|^2 of an add (0 for a drop)
};

__host__ __device__ inline int ra_size(int layout, int M) { return layout == 1 ? ra_packed_size(M) : M * M; }

// gi_core.h: J' (sJT), R_A, d in LDS; script entry e = (kind, arg): kind 0 adds constraint arg, kind 1
// drops position arg.  d, beta, z as gi_qp's rebuild loop computes them
template <int MAXM, class RAL>
__device__ __forceinline__ void factors_core(int M, int Nu, const double* rinv, const int* script, int nscript,
                                             const double* rhs, const FactorOut& o, double* lds, const RAL& ra,
                                             int rasz) {
  const int lane = threadIdx.x;
  const bool row = lane < M;
  double* sRi = lds;
  double* sJT = sRi + M * M;
  double* sRA = sJT + M * M;
  double* sd = sRA + ((rasz + 1) & ~1);
  for (int e = lane; e < M * M; e += 64) {
    sRi[e] = rinv[e];
    sJT[e] = 0.0;
  }
  for (int e = lane; e < rasz; e += 64) sRA[e] = 0.0;
  sd[lane] = 0.0;
  lds_sync();
  const RowCons rc = row_cons(lane, M, Nu, M / Nu, nullptr);
  GIState<MAXM> S;
  gi_reset<MAXM>(S);
  gi_load_rinv<MAXM>(S, sJT, sRi, M, row);
  const double c = rhs[lane];
  for (int e = 0; e < nscript; ++e) {
    const int kind = script[2 * e], arg = script[2 * e + 1];
    double beta = 0.0, dn2 = 0.0;
    if (kind == 0) {
      int j0, mp;
      double sg;
      gi_normal(arg, rc, j0, mp, sg);
      const double dk = gi_dvec<MAXM>(sJT, sd, M, j0, mp, sg, row);
      dn2 = qsum<MAXM>(dk * dk);
      beta = qsum<MAXM>(lane >= S.q ? dk * dk : 0.0);
      lds_sync();
      const double zm = gi_z(sJT, sd, S.q, M, row);
      gi_add<MAXM>(S, sJT, sRA, sd, M, arg, dk, beta, zm, (double)(e + 1), row, BoxMark{}, ra);
    } else {
      gi_drop<MAXM>(S, sJT, sRA, M, arg, BoxMark{}, ra);
    }
    const double bs = gi_backsub<MAXM>(S, sRA, M, c, ra);
    for (int x = lane; x < M * M; x += 64) o.J[(long long)e * M * M + x] = sJT[x];
    for (int x = lane; x < rasz; x += 64) o.RA[(long long)e * rasz + x] = sRA[x];
    o.lane_d[e * 192 + lane] = S.rdg;
    o.lane_d[e * 192 + 64 + lane] = S.uw;
    o.lane_d[e * 192 + 128 + lane] = bs;
    o.lane_i[e * 128 + lane] = S.ww;
    o.lane_i[e * 128 + 64 + lane] = (int)S.act;
    if (lane == 0) {
      o.scal[2 * e] = S.q;
      o.scal[2 * e + 1] = S.nrot;
      o.beta[2 * e] = beta;
      o.beta[2 * e + 1] = dn2;
    }
    lds_sync();
  }
}

// gpc_qp16.h: J in registers (dumped as J[i][4b + r], 16 x 16), B in LDS (stride kBS), R_A in LDS
__device__ __forceinline__ void factors_reg(int M, int Nu, const double* rinv, const int* script, int nscript,
                                            const FactorOut& o, double* lds) {
  const int lane = threadIdx.x, i = lane & 15, b = lane >> 4;
  double* sRi = lds;
  double* sRA = sRi + ((M * M + 1) & ~1);
  double* sB = sRA + ((M * M + 1) & ~1);
  for (int e = lane; e < M * M; e += 64) {
    sRi[e] = rinv[e];
    sRA[e] = 0.0;
  }
  for (int e = lane; e < 16 * kBS; e += 64) sB[e] = 0.0;
  lds_sync();
  const RowCons rc = row_cons(i, M, Nu, M / Nu, nullptr);
  GIState<16> S;
  gi_reset<16>(S);
  RegFactors F;
  FOR4(r, F.J[r] = 0.0;);
  F.sB = sB;
  gi16_load_rinv<false>(S, F, sRi, M);
  for (int e = 0; e < nscript; ++e) {
    const int kind = script[2 * e], arg = script[2 * e + 1];
    double beta = 0.0, dn2 = 0.0;
    if (kind == 0) {
      int j0, mp;
      double sg;
      gi_normal(arg, rc, j0, mp, sg);
      d4v Bl, d;
      lds_sync();
      b_row4(F.sB, Bl);
      gi16_dvec(F, j0, mp, sg, d);
      double z, jq, rk;
      gi16_products(F, Bl, d, S.q, z, jq, rk, dn2, beta);
      gi16_add(S, F, sRA, M, arg, d, beta, z, jq, rk, (double)(e + 1), BoxMark16{});
    } else {
      gi16_drop(S, F, sRA, M, arg, BoxMark16{});
    }
    FOR4(r, o.J[e * 256 + i * 16 + 4 * b + r] = F.J[r];);
    for (int x = lane; x < M * M; x += 64) o.RA[(long long)e * M * M + x] = sRA[x];
    for (int x = lane; x < 16 * kBS; x += 64) o.B[e * 256 + x] = sB[x];
    o.lane_d[e * 192 + lane] = S.rdg;
    o.lane_d[e * 192 + 64 + lane] = S.uw;
    o.lane_d[e * 192 + 128 + lane] = 0.0;
    o.lane_i[e * 128 + lane] = S.ww;
    o.lane_i[e * 128 + 64 + lane] = (int)S.act;
    if (lane == 0) {
      o.scal[2 * e] = S.q;
      o.scal[2 * e + 1] = S.nrot;
      o.beta[2 * e] = beta;
      o.beta[2 * e + 1] = dn2;
    }
    lds_sync();
  }
}

// layout: 0 RAFull, 1 RAPacked, 2 the register variant (maxm 16 only)
__global__ void __launch_bounds__(64) factors_kernel(int maxm, int layout, int M, int Nu, const double* rinv,
                                                     const int* script, int nscript, const double* rhs,
                                                     const FactorOut o) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int rasz = ra_size(layout, M);
  if (layout == 2) {
    factors_reg(M, Nu, rinv, script, nscript, o, lds);
  } else if (maxm == 16) {
    if (layout == 0) factors_core<16>(M, Nu, rinv, script, nscript, rhs, o, lds, RAFull{M}, rasz);
    else factors_core<16>(M, Nu, rinv, script, nscript, rhs, o, lds, RAPacked{}, rasz);
  } else if (maxm == 32) {
    if (layout == 0) factors_core<32>(M, Nu, rinv, script, nscript, rhs, o, lds, RAFull{M}, rasz);
    else factors_core<32>(M, Nu, rinv, script, nscript, rhs, o, lds, RAPacked{}, rasz);
  } else {
    if (layout == 0) factors_core<64>(M, Nu, rinv, script, nscript, rhs, o, lds, RAFull{M}, rasz);
    else factors_core<64>(M, Nu, rinv, script, nscript, rhs, o, lds, RAPacked{}, rasz);
  }
}

// ------------------------------------------------------------------------------------------------
// QP drivers.  Sequence s: rinv [s][M*M] (row-major upper R^-1), bounds [s][4][nu], xu [s][T][M],
// up [s][T][nu]; one GIState (and RegFactors) kept across the T steps, as the step loops keep it.
struct QpOut {
  double* x;                     // [s][T][M]
  int *it, *st, *q, *ids, *nrot;  // [s][T], [s][T] (this step's bits), [s][T], [s][T][64], [s][T]
};

template <int MAXM>
__device__ __forceinline__ void qp_core(int T, int M, int Nu, const double* rinv, const double* bnd,
                                        const double* xu, const double* up, double tol, int maxit,
                                        const QpOut& o, double* lds) {
  const int lane = threadIdx.x, s = blockIdx.x, nu = M / Nu;
  const bool row = lane < M;
  double* sRi = lds;
  double* sJT = sRi + M * M;
  double* sRA = sJT + M * M;
  double* sd = sRA + M * M;
  double* sxc = sd + 64;
  double* ssl = sxc + 64;
  for (int e = lane; e < M * M; e += 64) {
    sRi[e] = rinv[(long long)s * M * M + e];
    sJT[e] = 0.0;
    sRA[e] = 0.0;
  }
  sd[lane] = 0.0;
  sxc[lane] = 0.0;
  for (int k = 0; k < 4; ++k) ssl[4 * lane + k] = 0.0;
  lds_sync();
  const RowCons rc = row_cons(lane, M, Nu, nu, bnd + (long long)s * 4 * nu);
  GIState<MAXM> S;
  gi_reset<MAXM>(S);
  const QPBufs qb{sRi, sxc, sJT, sd, sRA, ssl};
  for (int t = 0; t < T; ++t) {
    const long long st_i = (long long)s * T + t;
    const double x_u = row ? xu[st_i * M + lane] : 0.0;
    const double up_row = row ? up[st_i * nu + rc.n] : 0.0;
    if (row) sxc[lane] = x_u;
    lds_sync();
    int st = 0;
    const int it = gi_qp<MAXM>(qb, M, Nu, rc, up_row, x_u, tol, maxit, &st, S);
    if (row) o.x[st_i * M + lane] = sxc[lane];
    o.ids[st_i * 64 + lane] = S.ww;
    if (lane == 0) {
      o.it[st_i] = it;
      o.st[st_i] = st;
      o.q[st_i] = S.q;
      o.nrot[st_i] = S.nrot;
    }
    lds_sync();
  }
}

template <bool PACKED, bool BLDS>
__device__ __forceinline__ void qp_reg(int T, int M, int Nu, const double* rinv, const double* bnd,
                                       const double* xu, const double* up, double tol, int maxit, int rebuild,
                                       const QpOut& o, double* lds) {
  const int lane = threadIdx.x, s = blockIdx.x, nu = M / Nu, i = lane & 15;
  const bool row = i < M;
  double* sRi = lds;
  double* sRA = sRi + ((M * M + 1) & ~1);
  double* sB = sRA + ((M * M + 1) & ~1);
  double* sbnd = sB + 16 * kBS;  // [nu][dmin, dmax, umin, umax] (gpc_small.hip)
  const double* rin = rinv + (long long)s * M * M;
  const double* bn = bnd + (long long)s * 4 * nu;
  for (int e = lane; e < M * M; e += 64) {
    const int r = e / M, k = e - r * M;
    if (!PACKED) sRi[e] = rin[e];
    else if (k >= r) sRi[rinv_idx<true>(r, k, M)] = rin[e];
    sRA[e] = 0.0;
  }
  for (int e = lane; e < 16 * kBS; e += 64) sB[e] = 0.0;
  if (lane < 4 * nu) sbnd[lane] = bn[(lane & 3) * nu + (lane >> 2)];
  lds_sync();
  RowCons rc = row_cons(i, M, Nu, nu, bn);
  if (BLDS) rc.bnd = sbnd + 4 * rc.n;
  GIState<16> S;
  gi_reset<16>(S);
  RegFactors F;
  FOR4(r, F.J[r] = 0.0;);
  F.sB = sB;
  for (int t = 0; t < T; ++t) {
    const long long st_i = (long long)s * T + t;
    const double x_u = row ? xu[st_i * M + i] : 0.0;
    const double up_row = row ? up[st_i * nu + rc.n] : 0.0;
    int st = 0;
    double xq = 0.0;
    const int it = gi_qp16<PACKED, void, BLDS>(sRi, sRA, M, Nu, rc, up_row, x_u, tol, maxit, &st, S, F, rebuild, xq);
    if (lane < M) o.x[st_i * M + lane] = xq;
    o.ids[st_i * 64 + lane] = S.ww;
    if (lane == 0) {
      o.it[st_i] = it;
      o.st[st_i] = st;
      o.q[st_i] = S.q;
      o.nrot[st_i] = S.nrot;
    }
    lds_sync();
  }
}

// variant: 0 gi_qp<16>, 1 gi_qp<32>, 2 gi_qp<64>, 3 gi_qp16<false, void, false>, 4 gi_qp16<true, void, true>
__global__ void __launch_bounds__(64) qp_kernel(int variant, int T, int M, int Nu, const double* rinv,
                                                const double* bnd, const double* xu, const double* up,
                                                double tol, int maxit, int rebuild, const QpOut o) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  switch (variant) {
    case 0: qp_core<16>(T, M, Nu, rinv, bnd, xu, up, tol, maxit, o, lds); break;
    case 1: qp_core<32>(T, M, Nu, rinv, bnd, xu, up, tol, maxit, o, lds); break;
    case 2: qp_core<64>(T, M, Nu, rinv, bnd, xu, up, tol, maxit, o, lds); break;
    case 3: qp_reg<false, false>(T, M, Nu, rinv, bnd, xu, up, tol, maxit, rebuild, o, lds); break;
    default: qp_reg<true, true>(T, M, Nu, rinv, bnd, xu, up, tol, maxit, rebuild, o, lds); break;
  }
}

// ------------------------------------------------------------------------------------------------
// host side: device copies of the arguments, freed on every path
struct Arena {
  std::vector<void*> ptrs;
  hipError_t err = hipSuccess;
  ~Arena() {
    for (void* p : ptrs) (void)hipFree(p);
  }
  template <class T>
  T* up(const T* host, size_t n) {  // device copy of host[n] (zeros when host is null)
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    const size_t bytes = (n ? n : 1) * sizeof(T);
    err = hipMalloc(&d, bytes);
    if (err != hipSuccess) return nullptr;
    ptrs.push_back(d);
    err = host ? hipMemcpy(d, host, n * sizeof(T), hipMemcpyHostToDevice) : hipMemset(d, 0, bytes);
    return static_cast<T*>(d);
  }
  template <class T>
  void down(T* host, const T* dev, size_t n) {
    if (err == hipSuccess && host && n) err = hipMemcpy(host, dev, n * sizeof(T), hipMemcpyDeviceToHost);
  }
};

template <class K>
hipError_t allow_lds(K kern, size_t bytes) {
  if (bytes <= 64 * 1024) return hipSuccess;
  return hipFuncSetAttribute(reinterpret_cast<const void*>(kern), hipFuncAttributeMaxDynamicSharedMemorySize,
                             (int)bytes);
}

hipError_t finish(Arena& A) {
  if (A.err != hipSuccess) return A.err;
  A.err = hipGetLastError();
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  return A.err;
}

}  // namespace

extern "C" {

int probe_prim(int op, int ncase, const double* in_a, const double* in_b, const int* in_i, double* out_d,
               int* out_i) {
  const bool bcast16 = op >= OP_ROW_BCAST16 && op < OP_ROW_BCAST16 + 16;
  if (ncase < 1 || ncase > 65535 || !((op >= 0 && op < OP_N) || bcast16)) return (int)hipErrorInvalidValue;
  Arena A;
  const size_t n = (size_t)ncase * 64;
  const double* da = A.up(in_a, n);
  const double* db = A.up(in_b, n);
  const int* di = A.up(in_i, n);
  double* dd = A.up<double>(nullptr, n * 4);
  int* dk = A.up<int>(nullptr, n);
  if (A.err != hipSuccess) return (int)A.err;
  prim_kernel<<<ncase, 64, 64 * sizeof(double)>>>(op, ncase, da, db, di, dd, dk);
  if (finish(A) != hipSuccess) return (int)A.err;
  A.down(out_d, dd, n * 4);
  A.down(out_i, dk, n);
  return (int)A.err;
}

int probe_factors(int maxm, int layout, int M, int Nu, const double* rinv, const int* script, int nscript,
                  const double* rhs, double* outJ, double* outRA, double* outB, double* out_lane_d,
                  int* out_lane_i, int* out_scal, double* out_beta) {
  const bool reg = layout == 2;
  if (!(maxm == 16 || maxm == 32 || maxm == 64) || layout < 0 || layout > 2 || (reg && maxm != 16) || M < 1 ||
      M > maxm || Nu < 1 || M % Nu != 0 || nscript < 1 || nscript > 4096)
    return (int)hipErrorInvalidValue;
  // the script must keep 0 <= q <= M, drop positions below q and constraint ids below 4 M
  {
    int q = 0;
    for (int e = 0; e < nscript; ++e) {
      const int kind = script[2 * e], arg = script[2 * e + 1];
      if (kind == 0) {
        if (q >= M || arg < 0 || arg >= 4 * M) return (int)hipErrorInvalidValue;
        ++q;
      } else if (kind == 1) {
        if (arg < 0 || arg >= q) return (int)hipErrorInvalidValue;
        --q;
      } else {
        return (int)hipErrorInvalidValue;
      }
    }
  }
  const int rasz = ra_size(layout, M);
  const size_t jsz = reg ? 256 : (size_t)M * M;
  const size_t lds = reg ? sizeof(double) * (2 * ((M * M + 1) & ~1) + 16 * kBS)
                         : sizeof(double) * (2 * (size_t)M * M + ((rasz + 1) & ~1) + 64);
  Arena A;
  const double* dri = A.up(rinv, (size_t)M * M);
  const int* dsc = A.up(script, (size_t)2 * nscript);
  const double* drh = A.up(rhs, 64);
  FactorOut o;
  o.J = A.up<double>(nullptr, jsz * nscript);
  o.RA = A.up<double>(nullptr, (size_t)rasz * nscript);
  o.B = A.up<double>(nullptr, (size_t)256 * nscript);
  o.lane_d = A.up<double>(nullptr, (size_t)192 * nscript);
  o.lane_i = A.up<int>(nullptr, (size_t)128 * nscript);
  o.scal = A.up<int>(nullptr, (size_t)2 * nscript);
  o.beta = A.up<double>(nullptr, (size_t)2 * nscript);
  if (A.err != hipSuccess) return (int)A.err;
  A.err = allow_lds(factors_kernel, lds);
  if (A.err != hipSuccess) return (int)A.err;
  factors_kernel<<<1, 64, lds>>>(maxm, layout, M, Nu, dri, dsc, nscript, drh, o);
  if (finish(A) != hipSuccess) return (int)A.err;
  A.down(outJ, o.J, jsz * nscript);
  A.down(outRA, o.RA, (size_t)rasz * nscript);
  if (reg) A.down(outB, o.B, (size_t)256 * nscript);
  A.down(out_lane_d, o.lane_d, (size_t)192 * nscript);
  A.down(out_lane_i, o.lane_i, (size_t)128 * nscript);
  A.down(out_scal, o.scal, (size_t)2 * nscript);
  A.down(out_beta, o.beta, (size_t)2 * nscript);
  return (int)A.err;
}

int probe_qp(int variant, int nseq, int T, int M, int Nu, const double* rinv, const double* bounds,
             const double* xu, const double* up, double tol, int maxit, int rebuild, double* out_x, int* out_it,
             int* out_st, int* out_q, int* out_ids, int* out_nrot) {
  const int maxm = variant == 1 ? 32 : variant == 2 ? 64 : 16;
  if (variant < 0 || variant > 4 || nseq < 1 || nseq > 65535 || T < 1 || M < 1 || M > maxm || Nu < 1 ||
      M % Nu != 0 || maxit < 1 || rebuild < 1)
    return (int)hipErrorInvalidValue;
  const int nu = M / Nu;
  const size_t lds = variant <= 2 ? sizeof(double) * (3 * (size_t)M * M + 64 + 64 + 256)
                                  : sizeof(double) * (2 * ((M * M + 1) & ~1) + 16 * kBS + 64);
  const size_t steps = (size_t)nseq * T;
  Arena A;
  const double* dri = A.up(rinv, (size_t)nseq * M * M);
  const double* dbn = A.up(bounds, (size_t)nseq * 4 * nu);
  const double* dxu = A.up(xu, steps * M);
  const double* dup = A.up(up, steps * nu);
  QpOut o;
  o.x = A.up<double>(nullptr, steps * M);
  o.it = A.up<int>(nullptr, steps);
  o.st = A.up<int>(nullptr, steps);
  o.q = A.up<int>(nullptr, steps);
  o.ids = A.up<int>(nullptr, steps * 64);
  o.nrot = A.up<int>(nullptr, steps);
  if (A.err != hipSuccess) return (int)A.err;
  A.err = allow_lds(qp_kernel, lds);
  if (A.err != hipSuccess) return (int)A.err;
  qp_kernel<<<nseq, 64, lds>>>(variant, T, M, Nu, dri, dbn, dxu, dup, tol, maxit, rebuild, o);
  if (finish(A) != hipSuccess) return (int)A.err;
  A.down(out_x, o.x, steps * M);
  A.down(out_it, o.it, steps);
  A.down(out_st, o.st, steps);
  A.down(out_q, o.q, steps);
  A.down(out_ids, o.ids, steps * 64);
  A.down(out_nrot, o.nrot, steps);
  return (int)A.err;
}

}  // extern "C"
