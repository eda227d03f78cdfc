// Stand-alone check of gpc_small_kernel's lane tables over plant variants (csrc/scenario_tables.h
// small_plant), built with the address, leak and undefined-behaviour sanitizers by
// tests/test_small_variants.py.  No GPU is used.
//   A Shell 3x3 scenario with three plant variants that differ in gain, in delay and in the number of
//   denominator taps: variant v's 64 table rows equal the rows of the single-plant scenario built
//   from plant v (its entry-ring offsets and masks restated for the common ke), ke is the maximum
//   over the variants, acol is the single-plant map, and the packed blob holds all nvar * 64 rows.
//   One variant entry outside the kernel's limits makes the whole scenario not small.
// Exit status 0 when every expectation held.
#include "check.h"

// the nominal model (tests/c_abi/mpct_c_demo.c: the saved mpc object's scaled discrete tf) and three
// plants: 0 the model itself, 1 gains x 1.2 and every delay one sample longer, 2 second-order
// entries (two numerator and two denominator taps: four terms, an entry output ring of 4)
struct Case {
  static constexpr int NIT = 40, NV = 3;
  double num[9][2] = {{0.02313052619372795, 0.06667958558934375}, {0.0, 0.013710194313372143},
                      {0.02089018186516949, 0.06022122704814364}, {0.058828715846932514, 0.0565220089046257},
                      {0.02173580108248058, 0.021023216763849436}, {0.0294987546979058, 0.08419778882992246},
                      {0.0, 0.1963360266878832},                  {0.032116113806741245, 0.03068897122230742},
                      {0.0, 0.3338832924071783}};
  double den[9][2] = {{1.0, -0.9231163463866358}, {1.0, -0.9355069850316178}, {1.0, -0.9231163463866358},
                      {1.0, -0.9231163463866358}, {1.0, -0.9355069850316178}, {1.0, -0.9048374180359595},
                      {1.0, -0.8858460329277068}, {1.0, -0.9131007162822624}, {1.0, -0.8101577349324267}};
  int32_t delay[9] = {7, 7, 7, 5, 4, 4, 5, 6, 0};
  double num1[9][2], num2[9][3], den2[9][3], num5[3] = {0.01, 0.02, 0.03};
  double umin[3] = {-1.510877401316376, -3.628338208043142, -2.4288171452857927};
  double umax[3] = {0.755438700658188, 1.814169104021571, 1.2144085726428964};
  double dumax[3] = {0.0755438700658188, 0.18141691040215713, 0.12144085726428963};
  double dumin[3];
  int32_t n1[3] = {1, 1, 1};
  mpct_dtf P[9], V[NV * 9];
  std::vector<double> yref = std::vector<double>(3 * NIT, 0.1);
  mpct_scenario_desc d{};
  Case() {
    for (int e = 0; e < 9; ++e) {
      P[e] = V[e] = {2, num[e], den[e], delay[e]};
      for (int k = 0; k < 2; ++k) num1[e][k] = 1.2 * num[e][k];
      V[9 + e] = {2, num1[e], den[e], delay[e] + 1};
      // (1 - p z^-1)(1 - 0.5 z^-1) with the numerator's first tap moved into the delay
      num2[e][0] = 0.0;
      num2[e][1] = num[e][1];
      num2[e][2] = 0.25 * num[e][1];
      den2[e][0] = 1.0;
      den2[e][1] = den[e][1] - 0.5;
      den2[e][2] = -0.5 * den[e][1];
      V[18 + e] = {3, num2[e], den2[e], delay[e]};
    }
    for (int n = 0; n < 3; ++n) dumin[n] = -dumax[n];
    d.abi_version = MPCT_ABI_VERSION;
    d.my = d.nu = 3;
    d.nit = NIT;
    d.n2_max = 30;
    d.nu_max = 5;
    d.weights_squared = 1;
    d.vns_ink = 10;
    d.n1 = n1;
    d.plant = d.model = P;
    d.du_min = dumin;
    d.du_max = dumax;
    d.u_min = umin;
    d.u_max = umax;
    d.yref = yref.data();
  }
  Case(const Case&) = delete;
};

int main() {
  Case c;
  // the single-plant scenarios, one per variant
  SmallTables one[Case::NV];
  int ke_max = 0;
  for (int v = 0; v < Case::NV; ++v) {
    mpct_scenario_desc d1 = c.d;
    d1.plant = c.V + 9 * v;
    auto s1 = build(d1);
    if (!s1) return 1;
    CHECK(s1->nvar == 1);
    CHECK(small_plant(s1.get(), &one[v]));
    CHECK(one[v].coef.size() == (size_t)kWave);
    ke_max = std::max(ke_max, one[v].ke);
  }
  CHECK(one[0].ke == 2 && one[1].ke == 2 && one[2].ke == 4);  // the variants differ in denominator taps
  CHECK(one[0].hc != one[1].hc);                              // ... in delay
  CHECK(one[0].coef != one[1].coef);                          // ... and in gain

  // the three-variant scenario
  mpct_scenario_desc dm = c.d;
  dm.nplant = Case::NV;
  dm.plant_var = c.V;
  auto sm = build(dm);
  if (!sm) return 1;
  SmallTables all;
  CHECK(sm->nvar == Case::NV);
  CHECK(small_plant(sm.get(), &all));
  CHECK(all.ke == ke_max);
  const size_t lanes = (size_t)Case::NV * kWave;
  CHECK(all.coef.size() == lanes && all.hoff.size() == lanes && all.hc.size() == lanes && all.hmask.size() == lanes);
  CHECK(all.acol == one[0].acol && all.acol == one[1].acol && all.acol == one[2].acol);
  if (g_bad) return 1;  // the sizes hold: the rows can be read
  int ataps = 0;
  for (int v = 0; v < Case::NV; ++v)
    for (int L = 0; L < kWave; ++L) {
      const size_t Li = (size_t)v * kWave + L;
      CHECK(all.coef[Li] == one[v].coef[L]);
      CHECK(all.hc[Li] == one[v].hc[L]);
      if (one[v].hoff[L] >= kSmEOff) {  // a denominator tap: the entry's own ring, laid out by ke
        const int ep = (one[v].hoff[L] - kSmEOff) / one[v].ke;
        CHECK(ep == (L & 15) && one[v].hmask[L] == one[v].ke - 1);
        CHECK(all.hoff[Li] == kSmEOff + ep * all.ke);
        CHECK(all.hmask[Li] == all.ke - 1);
        CHECK(all.hc[Li] >= 1 && all.hc[Li] < all.ke);
        ++ataps;
      } else {  // a numerator tap (an input ring) or an idle lane
        CHECK(all.hoff[Li] == one[v].hoff[L]);
        CHECK(all.hmask[Li] == one[v].hmask[L] && all.hmask[Li] == kSmU - 1);
        CHECK(all.hc[Li] >= 0 && all.hc[Li] < kSmU);
      }
    }
  CHECK(ataps == 9 * (1 + 1 + 2));

  // the blob uploads all nvar * 64 rows, and the scalars name the small kernel
  {
    const PackedTables pk = pack_tables(sm.get());
    const DevScenario ds = pk.rebased(pk.blob.data());
    CHECK(ds.small == 1 && ds.small_dtc == 0 && ds.nvar == Case::NV && ds.sm_ke == ke_max);
    size_t found = 0;
    for (const auto& t : pk.dslots)
      if (t.field == &DevScenario::sm_coef) {
        CHECK(t.bytes == lanes * 8 && t.off + t.bytes <= pk.blob.size());
        ++found;
      }
    for (const auto& t : pk.islots)
      if (t.field == &DevScenario::sm_hoff || t.field == &DevScenario::sm_hc || t.field == &DevScenario::sm_hmask) {
        CHECK(t.bytes == lanes * 4 && t.off + t.bytes <= pk.blob.size());
        ++found;
      }
    CHECK(found == 4);
    if (found == 4 && !g_bad) {
      CHECK(std::memcmp(ds.sm_coef, all.coef.data(), lanes * 8) == 0);
      CHECK(std::memcmp(ds.sm_hoff, all.hoff.data(), lanes * 4) == 0);
      CHECK(std::memcmp(ds.sm_hc, all.hc.data(), lanes * 4) == 0);
      CHECK(std::memcmp(ds.sm_hmask, all.hmask.data(), lanes * 4) == 0);
      CHECK(std::memcmp(ds.sm_acol, all.acol.data(), all.acol.size() * 4) == 0);
    }
    std::printf("valid shell3x3 x %d variants: ke %d, %zu lane rows, %zu blob bytes\n", Case::NV, all.ke, lanes,
                pk.blob.size());
  }

  // one entry of the last variant with five terms (three numerator taps): not small, for any variant
  {
    Case c5;
    c5.V[2 * 9 + 4] = {3, c5.num5, c5.den2[4], c5.delay[4]};
    mpct_scenario_desc d5 = c5.d;
    d5.nplant = Case::NV;
    d5.plant_var = c5.V;
    auto s5 = build(d5);
    if (!s5) return 1;
    SmallTables t5;
    CHECK(!small_plant(s5.get(), &t5));
    const DevScenario ds = dev_scenario(s5.get());
    CHECK(ds.small == 0 && ds.small_dtc == 0 && ds.nvar == Case::NV);
    std::printf("five-term variant entry: small %d\n", ds.small);
  }
  // the longest delay the input ring holds (nb = kSmU) is small; nothing longer can be built at all:
  // the general kernel's rings have the same length (kMaxTaps)
  {
    Case cd;
    cd.V[9 + 3].delay = kSmU - 2;
    mpct_scenario_desc dd = cd.d;
    dd.nplant = Case::NV;
    dd.plant_var = cd.V;
    auto sd = build(dd);
    if (!sd) return 1;
    SmallTables td;
    CHECK(small_plant(sd.get(), &td));
    int hcmax = 0;
    for (int L = 0; L < kWave; ++L) hcmax = std::max(hcmax, td.hc[kWave + L]);
    CHECK(hcmax == kSmU - 1);
    cd.V[9 + 3].delay = kSmU - 1;
    BuildError err;
    CHECK(!build_scenario(dd, &err) && err.code == MPCT_ERANGE);
    std::printf("delay past the rings: rejected %d \"%s\"\n", err.code, err.msg.c_str());
  }

  return finish();
}
