// band_probe.hip — test-only probes of band_b.h, the band kernel's B = R_A^-1 factor (with wave_ops.h
// and gi_core.h, all three included unmodified).  Each extern "C" entry takes host pointers, validates
// its arguments, allocates, copies, launches one-wave workgroups (64 threads, dynamic LDS sized from
// Mz), synchronises, copies back, frees and returns the HIP error code.  Built into
// tests/device_units/libmpct_band_probe.so by __graft_entry__.build_band_probe(); never linked into
// libmpct.so.  The layouts of the arguments are documented in tests/band_factor_ref.py, and
// tests/test_band_factors_gpu.py is the only caller.
#include <hip/hip_runtime.h>

#include <vector>

#include "wave_ops.h"
#include "gi_core.h"
#include "band_b.h"

using namespace mpct;

namespace {

constexpr int kBitWords = 8;  // the LDS bitmap of the probe: ids base .. base + 32 * kBitWords - 1

__global__ void __launch_bounds__(64) prefix_kernel(const double* __restrict__ in, double* __restrict__ out) {
  const int lane = threadIdx.x, c = blockIdx.x;
  out[c * 64 + lane] = wave_prefix_sum(in[c * 64 + lane]);
}

struct BandOut {
  double *J, *B, *lane_d;  // per entry: J' [Mz*Mz], the packed B [rasz], [3][64] uw, w, lam
  int *lane_i;             // per entry: [2][64] ww, act
  unsigned* bits;          // per entry: [kBitWords]
  int* scal;               // per entry: [2] q, nrot
  double* beta;            // per entry: beta of an add (0 for a drop)
};

// LDS of one launch, every piece padded to an even number of doubles as band_layout pads its own
struct ProbeLayout {
  int ri, jt, bt, dv, nv, bits, total;
};
__host__ __device__ inline ProbeLayout probe_layout(int Mz, bool full_ri) {
  ProbeLayout L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 1) & ~1; return r; };
  L.ri = take(full_ri ? Mz * Mz : Mz);
  L.jt = take(Mz * Mz);
  L.bt = take(ra_packed_size(Mz));
  L.dv = take(Mz);
  L.nv = take(Mz);
  L.bits = take(kBitWords / 2);
  L.total = o;
  return L;
}

// the band kernel's QP state one update at a time: J' (sJT), B packed (sBT), d (sd) and the staged
// normal (snv) in LDS, no R_A (RANone, sRA = nullptr).  Script entry e = (kind, arg): kind 0 adds the
// constraint in row arg of `normals` (id ids[arg]), kind 1 drops position arg.  d, beta, z and r as
// the kernel's GI step computes them; after every entry w = B'c and lam = B w as its warm start does
template <int MAXM>
__device__ __forceinline__ void band_core(int Mz, bool full_ri, const double* rinv, const double* normals,
                                          const int* ids, int base, const int* script, int nscript,
                                          const double* rhs, const BandOut& o, double* lds) {
  const int lane = threadIdx.x;
  const bool row = lane < Mz;
  const ProbeLayout L = probe_layout(Mz, full_ri);
  const int rasz = ra_packed_size(Mz);
  double* sRi = lds + L.ri;
  double* sJT = lds + L.jt;
  double* sBT = lds + L.bt;
  double* sd = lds + L.dv;
  double* snv = lds + L.nv;
  unsigned* sbits = reinterpret_cast<unsigned*>(lds + L.bits);
  double* sRA = nullptr;  // RANone must never touch it
  const double poison = __builtin_nan("");
  if (full_ri) {
    for (int e = lane; e < Mz * Mz; e += 64) sRi[e] = rinv[e];
  } else if (row) {
    sRi[lane] = rinv[lane * Mz + lane];
  }
  for (int e = lane; e < Mz * Mz; e += 64) sJT[e] = poison;
  for (int e = lane; e < rasz; e += 64) sBT[e] = poison;
  if (row) {
    sd[lane] = poison;
    snv[lane] = poison;
  }
  if (lane < kBitWords) sbits[lane] = 0u;
  lds_sync();
  const BandMark mark{sbits, base};
  GIState<MAXM> S;
  gi_reset<MAXM>(S);
  // J = R^-1 (gi_load_rinv), or its diagonal in band mode: the kernel's load_j
  if (full_ri) {
    gi_load_rinv<MAXM>(S, sJT, sRi, Mz, row);
  } else {
    if (row) {
      const double dj = sRi[lane];
      for (int k = 0; k < Mz; ++k) sJT[k * Mz + lane] = k == lane ? dj : 0.0;
    }
    S.nrot = 0;
    S.jinit = true;
    lds_sync();
  }
  const double c = rhs[lane];
  for (int e = 0; e < nscript; ++e) {
    const int kind = script[2 * e], arg = script[2 * e + 1];
    double beta = 0.0;
    if (kind == 0) {
      const int p = ids[arg];
      if (row) snv[lane] = normals[arg * Mz + lane];
      lds_sync();
      double dk = 0.0;
      if (row) {  // d = J'n: lane k sums column k of J, the loop of the kernel's dvec
        const double* jc = sJT + lane * Mz;
        double d1 = 0.0;
        int r = 0;
        for (; r + 3 < Mz; r += 4) {
          const double j0 = jc[r], j1 = jc[r + 1], j2 = jc[r + 2], j3 = jc[r + 3];
          const double n0 = snv[r], n1 = snv[r + 1], n2 = snv[r + 2], n3 = snv[r + 3];
          dk += j0 * n0;
          d1 += j1 * n1;
          dk += j2 * n2;
          d1 += j3 * n3;
        }
        for (; r + 1 < Mz; r += 2) {
          dk += jc[r] * snv[r];
          d1 += jc[r + 1] * snv[r + 1];
        }
        if (r < Mz) dk += jc[r] * snv[r];
        dk += d1;
        sd[lane] = dk;
      }
      const double d2 = row ? dk * dk : 0.0;
      beta = qsum<MAXM>(lane >= S.q ? d2 : 0.0);
      lds_sync();
      const double zm = gi_z(sJT, sd, S.q, Mz, row);
      const double rk = bt_mul(sBT, sd, S.q);
      gi_add<MAXM>(S, sJT, sRA, sd, Mz, p, dk, beta, zm, (double)(e + 1), row, mark, RANone{}, BandBAdd{sBT, rk});
    } else {
      band_drop_b(S, sJT, sBT, Mz, arg, mark, snv, sd);
    }
    // w = B'c (c staged in snv), lam = B w (w staged in sd): the warm start's two products
    const int q = S.q;
    if (row) snv[lane] = lane < q ? c : 0.0;
    lds_sync();
    const double wv = bt_tmul(sBT, snv, q);
    if (row) sd[lane] = lane < q ? wv : 0.0;
    lds_sync();
    const double lam = bt_mul(sBT, sd, q);
    lds_sync();
    for (int x = lane; x < Mz * Mz; x += 64) o.J[(long long)e * Mz * Mz + x] = sJT[x];
    for (int x = lane; x < rasz; x += 64) o.B[(long long)e * rasz + x] = sBT[x];
    o.lane_d[e * 192 + lane] = S.uw;
    o.lane_d[e * 192 + 64 + lane] = wv;
    o.lane_d[e * 192 + 128 + lane] = lam;
    o.lane_i[e * 128 + lane] = S.ww;
    o.lane_i[e * 128 + 64 + lane] = (int)S.act;
    if (lane < kBitWords) o.bits[e * kBitWords + lane] = sbits[lane];
    if (lane == 0) {
      o.scal[2 * e] = S.q;
      o.scal[2 * e + 1] = S.nrot;
      o.beta[e] = beta;
    }
    // the staging vectors are poisoned again: the next entry must write what it reads
    if (row) {
      sd[lane] = poison;
      snv[lane] = poison;
    }
    lds_sync();
  }
}

__global__ void __launch_bounds__(64) band_kernel(int maxm, int Mz, int full_ri, const double* rinv,
                                                  const double* normals, const int* ids, int base,
                                                  const int* script, int nscript, const double* rhs,
                                                  const BandOut o) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  if (maxm == 16) band_core<16>(Mz, full_ri != 0, rinv, normals, ids, base, script, nscript, rhs, o, lds);
  else if (maxm == 32) band_core<32>(Mz, full_ri != 0, rinv, normals, ids, base, script, nscript, rhs, o, lds);
  else band_core<64>(Mz, full_ri != 0, rinv, normals, ids, base, script, nscript, rhs, o, lds);
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

// in, out: [ncase][64]
int probe_band_prefix(int ncase, const double* in, double* out) {
  if (ncase < 1 || ncase > 65535 || !in || !out) return (int)hipErrorInvalidValue;
  Arena A;
  const size_t n = (size_t)ncase * 64;
  const double* di = A.up(in, n);
  double* dd = A.up<double>(nullptr, n);
  if (A.err != hipSuccess) return (int)A.err;
  prefix_kernel<<<ncase, 64>>>(di, dd);
  if (finish(A) != hipSuccess) return (int)A.err;
  A.down(out, dd, n);
  return (int)A.err;
}

// rinv [Mz][Mz] (row-major upper R^-1; full_ri = 0 takes its diagonal), normals [nrows][Mz], ids [nrows],
// script [nscript][2], rhs [64]; the outputs per script entry as in BandOut
int probe_band_factors(int maxm, int Mz, int full_ri, const double* rinv, int nrows, const double* normals,
                       const int* ids, int base, const int* script, int nscript, const double* rhs, double* outJ,
                       double* outB, double* out_lane_d, int* out_lane_i, unsigned* out_bits, int* out_scal,
                       double* out_beta) {
  if (!(maxm == 16 || maxm == 32 || maxm == 64) || Mz < 1 || Mz > maxm || (full_ri != 0 && full_ri != 1) ||
      nrows < 1 || nrows > 4096 || nscript < 1 || nscript > 4096 || base < 1 || base > 256 || !rinv || !normals ||
      !ids || !script || !rhs)
    return (int)hipErrorInvalidValue;
  // box ids mark lane id >> 2 (< 64 with base <= 256), output ids one bit of the probe's bitmap
  for (int r = 0; r < nrows; ++r)
    if (ids[r] < 0 || ids[r] >= base + 32 * kBitWords) return (int)hipErrorInvalidValue;
  // the script must keep 0 <= q <= Mz, drop positions below q and rows below nrows
  {
    int q = 0;
    for (int e = 0; e < nscript; ++e) {
      const int kind = script[2 * e], arg = script[2 * e + 1];
      if (kind == 0) {
        if (q >= Mz || arg < 0 || arg >= nrows) return (int)hipErrorInvalidValue;
        ++q;
      } else if (kind == 1) {
        if (arg < 0 || arg >= q) return (int)hipErrorInvalidValue;
        --q;
      } else {
        return (int)hipErrorInvalidValue;
      }
    }
  }
  const int rasz = ra_packed_size(Mz);
  const size_t jsz = (size_t)Mz * Mz;
  const size_t lds = sizeof(double) * (size_t)probe_layout(Mz, full_ri != 0).total;
  Arena A;
  const double* dri = A.up(rinv, jsz);
  const double* dnm = A.up(normals, (size_t)nrows * Mz);
  const int* did = A.up(ids, (size_t)nrows);
  const int* dsc = A.up(script, (size_t)2 * nscript);
  const double* drh = A.up(rhs, 64);
  BandOut o;
  o.J = A.up<double>(nullptr, jsz * nscript);
  o.B = A.up<double>(nullptr, (size_t)rasz * nscript);
  o.lane_d = A.up<double>(nullptr, (size_t)192 * nscript);
  o.lane_i = A.up<int>(nullptr, (size_t)128 * nscript);
  o.bits = A.up<unsigned>(nullptr, (size_t)kBitWords * nscript);
  o.scal = A.up<int>(nullptr, (size_t)2 * nscript);
  o.beta = A.up<double>(nullptr, (size_t)nscript);
  if (A.err != hipSuccess) return (int)A.err;
  A.err = allow_lds(band_kernel, lds);
  if (A.err != hipSuccess) return (int)A.err;
  band_kernel<<<1, 64, lds>>>(maxm, Mz, full_ri, dri, dnm, did, base, dsc, nscript, drh, o);
  if (finish(A) != hipSuccess) return (int)A.err;
  A.down(outJ, o.J, jsz * nscript);
  A.down(outB, o.B, (size_t)rasz * nscript);
  A.down(out_lane_d, o.lane_d, (size_t)192 * nscript);
  A.down(out_lane_i, o.lane_i, (size_t)128 * nscript);
  A.down(out_bits, o.bits, (size_t)kBitWords * nscript);
  A.down(out_scal, o.scal, (size_t)2 * nscript);
  A.down(out_beta, o.beta, (size_t)nscript);
  return (int)A.err;
}

}  // extern "C"
