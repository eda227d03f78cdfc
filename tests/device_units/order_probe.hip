// order_probe.hip — test-only probe of the dispatch order (csrc/work_order.hip) with the host
// precompute it reads (csrc/scenario_tables.h), both included unmodified: this unit is self-contained,
// so order_candidates and its kernels are visible here.  Built into
// tests/device_units/libmpct_order_probe.so by __graft_entry__.build_order_probe(); never linked into
// libmpct.so.  tests/order_key_ref.py (class Probe) is the only caller.
#include "scenario_tables.h"
#include "work_order.hip"

using namespace mpct;

namespace {

// every device allocation of one call, freed on every path; err keeps the first HIP error
struct Arena {
  std::vector<void*> ptrs;
  hipError_t err = hipSuccess;
  WorkOrder wo;
  ~Arena() {
    order_release(wo);
    for (void* p : ptrs) (void)hipFree(p);
  }
  void* raw(const void* host, size_t bytes) {
    if (err != hipSuccess) return nullptr;
    void* d = nullptr;
    err = hipMalloc(&d, bytes ? bytes : 1);
    if (err != hipSuccess) return nullptr;
    ptrs.push_back(d);
    if (host && bytes) err = hipMemcpy(d, host, bytes, hipMemcpyHostToDevice);
    return d;
  }
  template <class T>
  const T* up(const T* host, size_t n) {
    return static_cast<const T*>(raw(host, n * sizeof(T)));
  }
};

}  // namespace

extern "C" {

// The keys and the permutation of one batch, as the library's launches get them.
//   desc   the public scenario descriptor, or NULL: no scenario (order_candidates without sc: the
//          weight-ratio key of kOrderGpc, the N Nu key of kOrderNmpc), with my and nu as given
//   kind   kOrderGpc / kOrderNmpc
//   flags  bit 0: drop the Gram tables (ds.gram = nullptr), so H is correlated in LDS
//   N2, Nu [C], delta [C][my], lambda [C][nu], r [nref][my][desc->nit] (desc only): host arrays
//   keys   [C] out, perm [C] out
// With a descriptor the steps are the library's (mpct_host.cpp build_ctx, gpc_kernel.hip): build_scenario,
// pack_tables, the blob copied to the device, rebased(dev), order_candidates on a fresh WorkOrder with
// no prefill, synchronise.  Returns the HIP error code; hipErrorInvalidValue for a descriptor the
// builder rejects, a batch below kOrderMinC (no order is computed) or a null array, hipErrorUnknown
// when order_candidates fails without a pending HIP error.
int probe_order(const mpct_scenario_desc* desc, int kind, int flags, int my, int nu, long long C, const int* N2,
                const int* Nu, const double* delta, const double* lambda, int nref, const double* r, unsigned* keys,
                int* perm) {
  if (C < kOrderMinC || C > (1ll << 24) || !N2 || !Nu || !delta || !lambda || !keys || !perm ||
      (kind != kOrderGpc && kind != kOrderNmpc))
    return (int)hipErrorInvalidValue;
  std::unique_ptr<mpct_scenario> s;
  if (desc) {
    BuildError be;
    s = build_scenario(*desc, &be);
    if (!s || nref < 1 || !r) return (int)hipErrorInvalidValue;
    my = s->my;
    nu = s->nu;
  } else if (my < 1 || my > kMaxOut || nu < 1 || nu > kMaxIn) {
    return (int)hipErrorInvalidValue;
  }
  Arena A;
  DevScenario ds{};
  const double* dr = nullptr;
  if (s) {
    const PackedTables pk = pack_tables(s.get());
    const void* blob = A.raw(pk.blob.data(), pk.blob.size());
    ds = pk.rebased(blob);
    if (flags & 1) ds.gram = nullptr;
    dr = A.up(r, (size_t)nref * my * s->nit);
  }
  const int* dN2 = A.up(N2, (size_t)C);
  const int* dNu = A.up(Nu, (size_t)C);
  const double* dd = A.up(delta, (size_t)C * my);
  const double* dl = A.up(lambda, (size_t)C * nu);
  if (A.err != hipSuccess) return (int)A.err;
  const int* dperm = nullptr;
  std::string msg;
  const int rc = s ? order_candidates(kind, my, nu, C, dN2, dNu, dd, dl, A.wo, &dperm, nullptr, &msg, &ds, nref, dr)
                   : order_candidates(kind, my, nu, C, dN2, dNu, dd, dl, A.wo, &dperm, nullptr, &msg);
  A.err = hipGetLastError();
  if (A.err == hipSuccess) A.err = hipDeviceSynchronize();
  if (A.err != hipSuccess) return (int)A.err;
  if (rc != 0 || !dperm) return (int)hipErrorUnknown;
  // order_candidates writes the keys into the first array of wo.buf (kin) and neither the counting
  // rank nor the radix sort (kin -> kout) overwrites it: the C keys are read back from there
  A.err = hipMemcpy(keys, A.wo.buf, (size_t)C * sizeof(unsigned), hipMemcpyDeviceToHost);
  if (A.err == hipSuccess) A.err = hipMemcpy(perm, dperm, (size_t)C * sizeof(int), hipMemcpyDeviceToHost);
  return (int)A.err;
}

}  // extern "C"
