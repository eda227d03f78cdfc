// Stand-alone layout probe of the host-only scenario precompute (csrc/scenario_tables.h), built by
// tests/test_plant_family.py with the flags of host_tables_check.cpp.  No GPU, no HIP runtime.
// It reads one linear GPC descriptor from stdin (text_descriptor.h; written by tests/plant_family.py
// descriptor_text), builds the scenario the way a host without CARIMA tables does (the library
// derives them from the model), and prints one line of `key=value` pairs: the kernel-choice flags and plant table sizes of
// dev_scenario / pack_tables, and for small scenarios the 64 plant-term coefficients of
// gpc_small_kernel's lanes (sm_coef=c0,c1,...,c63).  The row lengths of the band kernel's model tables
// follow (mz_maxa, mz_maxb, mz_maxbc), and for a band descriptor (text_descriptor.h, `band nd`) the
// per-entry lengths and first nonzero taps as comma-separated lists (mz_na, mz_nb, mz_off).  Exit status 0 on success, 1 on a malformed
// descriptor, 2 when the builder rejects it (its message is printed).
#include "text_descriptor.h"

using namespace mpct;

int main() {
  TextDescriptor t;
  if (!t.read()) return 1;
  const int my = t.my, nu = t.nu;
  const mpct_scenario_desc& d = t.d;
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
  for (int i = 0; i < my && i < (int)s->nyhi.size(); ++i) nyhi_max = std::max(nyhi_max, s->nyhi[i]);  // none on a band scenario
  for (int n = 0; n < nu && n < (int)s->dum.size(); ++n) dum_max = std::max(dum_max, s->dum[n]);
  std::printf("small=%d small_dtc=%d regpath=%d sm_ke=%d", ds.small, ds.small_dtc, ds.regpath, ds.sm_ke);
  std::printf(" ne=%d pl_maxb=%d pl_maxa=%d pl_maxbc=%d", ds.ne, ds.pl_maxb, ds.pl_maxa, ds.pl_maxbc);
  std::printf(" nx=%d nyh=%d nyhi_max=%d dum_max=%d", ds.nx, ds.nyh, nyhi_max, dum_max);
  if (ds.small) {
    std::printf(" sm_coef=");
    for (int L = 0; L < kWave; ++L) std::printf(L ? ",%.17g" : "%.17g", ds.sm_coef[L]);
  }
  std::printf(" mz_maxa=%d mz_maxb=%d mz_maxbc=%d", ds.mz_maxa, ds.mz_maxb, ds.mz_maxbc);
  if (t.band) {
    const std::pair<const char*, const std::vector<int>*> lists[] = {
        {"mz_na", &s->mz.na}, {"mz_nb", &s->mz.nb}, {"mz_off", &s->mz.off}};
    for (const auto& kv : lists) {
      std::printf(" %s=", kv.first);
      for (size_t e = 0; e < kv.second->size(); ++e) std::printf(e ? ",%d" : "%d", (int)(*kv.second)[e]);
    }
  }
  std::printf("\n");
  return 0;
}
