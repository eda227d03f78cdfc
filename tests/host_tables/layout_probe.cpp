// Stand-alone layout probe of the host-only scenario precompute (csrc/scenario_tables.h), built by
// tests/test_plant_family.py with the flags of host_tables_check.cpp.  No GPU, no HIP runtime.
// It reads one linear GPC descriptor from stdin (whitespace-separated numbers, written by
// tests/plant_family.py descriptor_text):
//   my nu nit n2_max nu_max
//   n1[my]
//   my*nu plant entries, row-major, each `len num[len] den[len] delay`
//   my*nu model entries, the same way
//   du_min[nu] du_max[nu] u_min[nu] u_max[nu]
// builds the scenario the way a host without CARIMA tables does (the library derives them from the
// model), and prints one line of `key=value` pairs: the kernel-choice flags and plant table sizes of
// dev_scenario / pack_tables, and for small scenarios the 64 plant-term coefficients of
// gpc_small_kernel's lanes (sm_coef=c0,c1,...,c63).  Exit status 0 on success, 1 on a malformed
// descriptor, 2 when the builder rejects it (its message is printed).
#include "scenario_tables.h"

#include <cstdio>
#include <iostream>

using namespace mpct;

struct Entries {
  std::vector<std::vector<double>> num, den;
  std::vector<mpct_dtf> tf;
  bool read(int n) {
    num.resize(n);
    den.resize(n);
    tf.resize(n);
    for (int e = 0; e < n; ++e) {
      int len = 0, delay = 0;
      if (!(std::cin >> len) || len < 1 || len > 64) return false;
      num[e].resize(len);
      den[e].resize(len);
      for (double& x : num[e])
        if (!(std::cin >> x)) return false;
      for (double& x : den[e])
        if (!(std::cin >> x)) return false;
      if (!(std::cin >> delay)) return false;
      tf[e] = {len, num[e].data(), den[e].data(), delay};
    }
    return true;
  }
};

static bool read_vec(std::vector<double>& v, int n) {
  v.resize(n);
  for (double& x : v)
    if (!(std::cin >> x)) return false;
  return true;
}

int main() {
  int my = 0, nu = 0, nit = 0, n2max = 0, numax = 0;
  if (!(std::cin >> my >> nu >> nit >> n2max >> numax) || my < 1 || my > kMaxOut || nu < 1 || nu > kMaxIn ||
      nit < 1) {
    std::printf("malformed descriptor: dims\n");
    return 1;
  }
  std::vector<int32_t> n1(my);
  for (int32_t& x : n1)
    if (!(std::cin >> x)) {
      std::printf("malformed descriptor: n1\n");
      return 1;
    }
  Entries plant, model;
  std::vector<double> dumin, dumax, umin, umax;
  if (!plant.read(my * nu) || !model.read(my * nu) || !read_vec(dumin, nu) || !read_vec(dumax, nu) ||
      !read_vec(umin, nu) || !read_vec(umax, nu)) {
    std::printf("malformed descriptor: entries / bounds\n");
    return 1;
  }
  const std::vector<double> yref((size_t)my * nit, 0.0);
  mpct_scenario_desc d{};
  d.abi_version = MPCT_ABI_VERSION;
  d.my = my;
  d.nu = nu;
  d.nit = nit;
  d.n2_max = n2max;
  d.nu_max = numax;
  d.weights_squared = 1;
  d.vns_ink = 10;
  d.n1 = n1.data();
  d.plant = plant.tf.data();
  d.model = model.tf.data();
  d.du_min = dumin.data();
  d.du_max = dumax.data();
  d.u_min = umin.data();
  d.u_max = umax.data();
  d.yref = yref.data();
  BuildError err;
  const std::unique_ptr<mpct_scenario> s = build_scenario(d, &err);
  if (!s) {
    std::printf("rejected %d \"%s\"\n", err.code, err.msg.c_str());
    return 2;
  }
  const DevScenario q = dev_scenario(s.get());
  const PackedTables pk = pack_tables(s.get());
  const DevScenario ds = pk.rebased(pk.blob.data());
  if (q.small != ds.small || q.small_dtc != ds.small_dtc || q.regpath != ds.regpath || q.sm_ke != ds.sm_ke) {
    std::printf("dev_scenario and pack_tables disagree\n");
    return 1;
  }
  int nyhi_max = 0, dum_max = 0;
  for (int i = 0; i < my; ++i) nyhi_max = std::max(nyhi_max, s->nyhi[i]);
  for (int n = 0; n < nu; ++n) dum_max = std::max(dum_max, s->dum[n]);
  std::printf("small=%d small_dtc=%d regpath=%d sm_ke=%d", ds.small, ds.small_dtc, ds.regpath, ds.sm_ke);
  std::printf(" ne=%d pl_maxb=%d pl_maxa=%d pl_maxbc=%d", ds.ne, ds.pl_maxb, ds.pl_maxa, ds.pl_maxbc);
  std::printf(" nx=%d nyh=%d nyhi_max=%d dum_max=%d", ds.nx, ds.nyh, nyhi_max, dum_max);
  if (ds.small) {
    std::printf(" sm_coef=");
    for (int L = 0; L < kWave; ++L) std::printf(L ? ",%.17g" : "%.17g", ds.sm_coef[L]);
  }
  std::printf("\n");
  return 0;
}
