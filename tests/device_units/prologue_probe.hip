// prologue_probe.hip — test-only probe of gpc_prologue.h, the once-per-candidate prologue of the linear
// closed-loop kernels (with mpct_dev.h and wave_ops.h, all three included unmodified).  The one extern "C"
// entry takes host pointers, validates its arguments, allocates, copies, launches one 64-thread workgroup
// per case, synchronises, copies back, frees and returns the HIP error code.  Built into
// tests/device_units/libmpct_prologue_probe.so by __graft_entry__.build_prologue_probe(); never linked
// into libmpct.so.  The layouts of the arguments are documented in tests/prologue_ref.py, and
// tests/test_prologue_units_gpu.py is the only caller.
//
// Instances (the `instance` field of a case): 0..2 gpc_prologue<16|32|64> (gpc_closed_loop_kernel),
// 3 <16, true, true, false, 12, true> (gpc_small_kernel), 4 its TABLES = false twin, 5..6
// <16|32, false, false, true, 4> (dtc_small_kernel at its default MPCT_DTC_HB = 4, dtc_robust.hip).  Three
// more exist only as the other side of a bitwise comparison and are no kernel's instance: 7..8
// <16|32, false, false, false, 4> (every row of A, for the FIRST rows of 5..6) and 9
// <16, false, true, false, 12, false> (the full R^-1 of the 12-row blocks, for the packed one of 3..4).
#include <hip/hip_runtime.h>

#include <vector>

#include "mpct_dev.h"
#include "wave_ops.h"
#include "gpc_prologue.h"

using namespace mpct;

namespace {

// header of one case, kHdr ints; the *_off fields index the double pool (step, phi, delta, lambda, qrt) or
// the int pool (n1, acol, qoff); -1 = absent (acol, qrt, qoff only)
enum { H_INST = 0, H_MY, H_NU, H_NX, H_WSQ, H_TLEN, H_N2MAX, H_NUMAX, H_M, H_NUC, H_N2, H_ASTRIDE, H_STEP, H_PHI,
       H_N1, H_DELTA, H_LAMBDA, H_ACOL, H_QRT, H_QRTLEN, H_QOFF, kHdr };
constexpr int kInstances = 10;
constexpr int kGuard = 64;  // sentinel doubles standing in for sRi (RINV = false) and closing the image
constexpr unsigned long long kSentinel = 0x7ff8a5c3d2e1f097ull;  // a quiet NaN with a payload of its own

struct Inst {
  int maxm;
  bool packed, rinv, first;
};
__host__ __device__ inline Inst inst_of(int k) {
  switch (k) {
    case 0: return {16, false, true, false};
    case 1: return {32, false, true, false};
    case 2: return {64, false, true, false};
    case 3: return {16, true, true, false};
    case 4: return {16, true, true, false};
    case 5: return {16, false, false, true};
    case 6: return {32, false, false, true};
    case 7: return {16, false, false, false};
    case 8: return {32, false, false, false};
    default: return {16, false, true, false};
  }
}
// LDS image of a case, in doubles: sR [M * M], sRi (full M * M, packed M (M + 1) / 2, or kGuard sentinel
// doubles without R^-1), sA [rows * astride] (rows = M, or M / Nu first-move rows), kGuard closing doubles
struct Layout {
  int ri, a, end, total;
};
__host__ __device__ inline Layout layout_of(int inst, int M, int Nu, int astride) {
  const Inst I = inst_of(inst);
  Layout L;
  L.ri = M * M;
  L.a = L.ri + (!I.rinv ? kGuard : I.packed ? M * (M + 1) / 2 : M * M);
  L.end = L.a + (I.first ? M / Nu : M) * astride;
  L.total = L.end + kGuard;
  return L;
}

template <int MAXM, bool PACKED, bool RINV, bool FIRST, int kHB, bool TABLES>
__global__ void __launch_bounds__(64) prologue_kernel(const int* __restrict__ hdr, const double* __restrict__ dp,
                                                      const int* __restrict__ ip, int ldsn,
                                                      double* __restrict__ out, int* __restrict__ flags) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x, c = blockIdx.x;
  const int* h = hdr + c * kHdr;
  DevScenario sc{};  // only what the prologue reads; everything else zero or null
  sc.my = h[H_MY];
  sc.nu = h[H_NU];
  sc.nx = h[H_NX];
  sc.wsq = h[H_WSQ];
  sc.tlen = h[H_TLEN];
  sc.n2max = h[H_N2MAX];
  sc.numax = h[H_NUMAX];
  sc.step = dp + h[H_STEP];
  sc.phi = dp + h[H_PHI];
  sc.n1 = ip + h[H_N1];
  sc.qrt = h[H_QRT] >= 0 ? dp + h[H_QRT] : nullptr;
  sc.qrt_off = h[H_QOFF] >= 0 ? ip + h[H_QOFF] : nullptr;
  const int M = h[H_M], Nu = h[H_NUC], N2 = h[H_N2], astride = h[H_ASTRIDE];
  const int* acol = h[H_ACOL] >= 0 ? ip + h[H_ACOL] : nullptr;
  const Layout L = layout_of(h[H_INST], M, Nu, astride);
  const double poison = __longlong_as_double((long long)kSentinel);
  for (int e = lane; e < ldsn; e += 64) lds[e] = poison;
  lds_sync();
  // RINV = false: the callers pass nullptr; the probe passes a sentinel region and the test checks it
  const bool ok = gpc_prologue<MAXM, PACKED, RINV, FIRST, kHB, TABLES>(sc, lane, M, Nu, N2, dp + h[H_DELTA],
                                                                        dp + h[H_LAMBDA], lds, lds + L.ri,
                                                                        lds + L.a, astride, acol);
  lds_sync();
  flags[c * 64 + lane] = ok ? 1 : 0;
  for (int e = lane; e < ldsn; e += 64) out[(long long)c * ldsn + e] = lds[e];
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
hipError_t launch(K kern, int ncase, size_t bytes, const int* hdr, const double* dp, const int* ip, int ldsn,
                  double* out, int* flags) {
  if (bytes > 64 * 1024) {
    const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kern),
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)bytes);
    if (e != hipSuccess) return e;
  }
  kern<<<ncase, 64, bytes>>>(hdr, dp, ip, ldsn, out, flags);
  return hipGetLastError();
}

// a [off, off + len) range of a pool of n entries
inline bool in_pool(long long off, long long len, long long n) { return off >= 0 && len >= 0 && off <= n - len; }

// everything gpc_prologue reads or writes for this case lies inside the pools and the LDS image
bool case_fits(const int* h, int inst, long long ndbl, long long nint, const int* ip) {
  const int my = h[H_MY], nu = h[H_NU], nx = h[H_NX], tlen = h[H_TLEN], n2max = h[H_N2MAX], numax = h[H_NUMAX];
  const int M = h[H_M], Nu = h[H_NUC], N2 = h[H_N2], astride = h[H_ASTRIDE];
  const Inst I = inst_of(inst);
  if (h[H_INST] != inst) return false;  // one instance per launch
  if (my < 1 || my > kMaxOut || nu < 1 || nu > kMaxIn || nx < 1 || nx > 256) return false;
  if (h[H_WSQ] != 0 && h[H_WSQ] != 1) return false;
  if (M < 1 || M >= kWave || M > I.maxm || Nu < 1 || M != nu * Nu) return false;
  if (N2 < 1 || N2 > n2max || n2max > 128 || Nu > numax || numax > 64 || tlen < 1 || tlen > 512) return false;
  if (astride < 1 || astride > 256) return false;
  if (!in_pool(h[H_STEP], (long long)my * nu * tlen, ndbl)) return false;
  if (!in_pool(h[H_PHI], (long long)my * n2max * nx, ndbl)) return false;
  if (!in_pool(h[H_DELTA], my, ndbl) || !in_pool(h[H_LAMBDA], nu, ndbl)) return false;
  if (!in_pool(h[H_N1], my, nint)) return false;
  for (int i = 0; i < my; ++i) {  // step index n1 + r - c, r < N2, c >= 0
    const int n1 = ip[h[H_N1] + i];
    if (n1 < 0 || n1 + N2 - 1 >= tlen) return false;
  }
  if (h[H_ACOL] >= 0) {
    if (!in_pool(h[H_ACOL], nx, nint)) return false;
    for (int v = 0; v < nx; ++v)
      if (ip[h[H_ACOL] + v] < 0 || ip[h[H_ACOL] + v] >= astride) return false;
  } else if (h[H_ACOL] != -1 || nx > astride) {
    return false;
  }
  if (h[H_QRT] >= 0) {  // tables: an offset table of every cell, this cell's rows inside the table
    const long long qlen = h[H_QRTLEN];
    if (!in_pool(h[H_QRT], qlen, ndbl) || !in_pool(h[H_QOFF], (long long)n2max * numax, nint)) return false;
    const int off = ip[h[H_QOFF] + (N2 - 1) * numax + (Nu - 1)];
    if (off < -1) return false;
    if (off >= 0 && !in_pool(off, (long long)my * (N2 < M ? N2 : M) * (M + nx), qlen)) return false;
  } else if (h[H_QRT] != -1 || h[H_QOFF] != -1) {
    return false;
  }
  return true;
}

}  // namespace

extern "C" {

// hdr [ncase][kHdr], dpool [ndbl], ipool [nint]; out_lds [ncase][ldsn] receives every case's whole LDS image
// (ldsn = the largest layout_of(..).total of the launch, returned through out_ldsn when out_lds is null: a
// size query, no launch), out_flags [ncase][64] the flag every lane returned
int probe_prologue(int instance, int ncase, const int* hdr, const double* dpool, long long ndbl, const int* ipool,
                   long long nint, double* out_lds, int* out_flags, int* out_ldsn) {
  if (instance < 0 || instance >= kInstances || ncase < 1 || ncase > 1024 || !hdr || !dpool || !ipool ||
      ndbl < 1 || ndbl > (1ll << 26) || nint < 1 || nint > (1ll << 26) || !out_ldsn)
    return (int)hipErrorInvalidValue;
  int ldsn = 0;
  for (int c = 0; c < ncase; ++c) {
    const int* h = hdr + c * kHdr;
    if (!case_fits(h, instance, ndbl, nint, ipool)) return (int)hipErrorInvalidValue;
    const int t = layout_of(instance, h[H_M], h[H_NUC], h[H_ASTRIDE]).total;
    ldsn = t > ldsn ? t : ldsn;
  }
  *out_ldsn = ldsn;
  if (!out_lds && !out_flags) return (int)hipSuccess;
  if (!out_lds || !out_flags) return (int)hipErrorInvalidValue;
  const size_t bytes = sizeof(double) * (size_t)ldsn;
  int dev = 0, maxlds = 0;
  hipError_t e = hipGetDevice(&dev);
  if (e == hipSuccess) e = hipDeviceGetAttribute(&maxlds, hipDeviceAttributeMaxSharedMemoryPerBlock, dev);
  if (e != hipSuccess) return (int)e;
  if (bytes > (size_t)maxlds) return (int)hipErrorInvalidValue;  // more LDS than the device reports
  Arena A;
  const int* dh = A.up(hdr, (size_t)ncase * kHdr);
  const double* dd = A.up(dpool, (size_t)ndbl);
  const int* di = A.up(ipool, (size_t)nint);
  double* dout = A.up<double>(nullptr, (size_t)ncase * ldsn);
  int* dfl = A.up<int>(nullptr, (size_t)ncase * 64);
  if (A.err != hipSuccess) return (int)A.err;
#define MPCT_LAUNCH(...) A.err = launch(prologue_kernel<__VA_ARGS__>, ncase, bytes, dh, dd, di, ldsn, dout, dfl)
  switch (instance) {
    case 0: MPCT_LAUNCH(16, false, true, false, 8, false); break;
    case 1: MPCT_LAUNCH(32, false, true, false, 8, false); break;
    case 2: MPCT_LAUNCH(64, false, true, false, 8, false); break;
    case 3: MPCT_LAUNCH(16, true, true, false, 12, true); break;
    case 4: MPCT_LAUNCH(16, true, true, false, 12, false); break;
    case 5: MPCT_LAUNCH(16, false, false, true, 4, false); break;
    case 6: MPCT_LAUNCH(32, false, false, true, 4, false); break;
    case 7: MPCT_LAUNCH(16, false, false, false, 4, false); break;
    case 8: MPCT_LAUNCH(32, false, false, false, 4, false); break;
    default: MPCT_LAUNCH(16, false, true, false, 12, false); break;
  }
#undef MPCT_LAUNCH
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) return (int)A.err;
  A.down(out_lds, dout, (size_t)ncase * ldsn);
  A.down(out_flags, dfl, (size_t)ncase * 64);
  return (int)A.err;
}

}  // extern "C"
