// Stand-alone check of the band kernel's plant-variant tables (csrc/scenario_tables.h build_scenario
// with the output-bias estimator), built with the address, leak and undefined-behaviour sanitizers by
// tests/test_band_mismatch.py.  No GPU is used.
//   A synthetic 2 x (1 MV + 1 MD) band scenario with three plant variants: 0 larger gains, 1 one
//   entry with a delay longer than any model delay, 2 one second-order entry (three numerator taps)
//   where the model is first order.  The tables are [nvar][ne], variant v's rows equal the rows of
//   the single-variant estimator scenario built from plant v, the row lengths pl_maxb / pl_maxa and
//   the compact tap length are the maxima over every variant and the model, and the packed blob
//   holds all nvar * ne rows.  A variant whose taps exceed the history rings is MPCT_ERANGE.
//   estimator = 0 is build_scenario as mpct_scenario_create calls it; what the builder still rejects,
//   the unknown estimator id and the estimator on a descriptor without mdband included.
// Exit status 0 when every expectation held.
#include "check.h"

struct Case {
  static constexpr int NIT = 60, NV = 3, NE = 4;  // entries (i, j): (0, u) (0, v) (1, u) (1, v)
  double num[NE][2] = {{0.0, 0.2}, {0.05, 0.03}, {0.0, 0.15}, {0.0, 0.1}};
  double den[NE][2] = {{1.0, -0.8}, {1.0, -0.7}, {1.0, -0.9}, {1.0, -0.6}};
  int32_t delay[NE] = {1, 0, 2, 0};
  double num0[NE][2];                                                    // variant 0: gains x 1.3
  double num2[3] = {0.1, 0.2, 0.05}, den2[3] = {1.0, -1.3, 0.4};         // variant 2's entry (0, u)
  double umin[1] = {-1.0}, umax[1] = {1.0}, dumin[1] = {-0.2}, dumax[1] = {0.2};
  double ymin[2] = {-0.3, -0.3}, ymax[2] = {0.3, 0.3}, ecr[2] = {1.0, 1.0};
  int32_t n1[2] = {1, 1};
  mpct_dtf M[NE], V[NV * NE];
  std::vector<double> yref = std::vector<double>(2 * NIT, 0.0);
  mpct_scenario_desc d{};
  Case() {
    for (int e = 0; e < NE; ++e) {
      M[e] = {2, num[e], den[e], delay[e]};
      for (int k = 0; k < 2; ++k) num0[e][k] = 1.3 * num[e][k];
      V[e] = {2, num0[e], den[e], delay[e]};
      V[NE + e] = V[2 * NE + e] = M[e];
    }
    V[NE + 2].delay = 5;                           // longer than any model delay (2)
    V[2 * NE + 0] = {3, num2, den2, delay[0]};     // second order, three taps from the first nonzero one
    d.abi_version = MPCT_ABI_VERSION;
    d.my = 2;
    d.nu = d.nd = 1;
    d.nit = NIT;
    d.n2_max = 12;
    d.nu_max = 3;
    d.weights_squared = 1;
    d.vns_ink = 10;
    d.n1 = n1;
    d.plant = d.model = M;
    d.du_min = dumin;
    d.du_max = dumax;
    d.u_min = umin;
    d.u_max = umax;
    d.yref = yref.data();
    d.mdband = 1;
    d.y_min = ymin;
    d.y_max = ymax;
    d.ecr_min = d.ecr_max = ecr;
    d.rho_ecr = 1e4;
  }
  Case(const Case&) = delete;
};

static bool same_tables(const ZTables& a, const ZTables& b) {
  return a.maxb == b.maxb && a.maxa == b.maxa && a.nb == b.nb && a.na == b.na && a.off == b.off && a.b == b.b &&
         a.a == b.a;
}

// entry ea of a equals entry eb of b: lengths, offset and every tap (the rows may differ in stride)
static bool same_entry(const ZTables& a, size_t ea, const ZTables& b, size_t eb) {
  if (a.nb[ea] != b.nb[eb] || a.na[ea] != b.na[eb] || a.off[ea] != b.off[eb]) return false;
  for (int l = 0; l < a.maxb; ++l)
    if (a.b[ea * a.maxb + l] != (l < b.maxb ? b.b[eb * b.maxb + l] : 0.0)) return false;
  for (int l = 0; l < a.maxa; ++l)
    if (a.a[ea * a.maxa + l] != (l < b.maxa ? b.a[eb * b.maxa + l] : 0.0)) return false;
  return true;
}

int main() {
  Case c;
  constexpr int NE = Case::NE, NV = Case::NV;
  // estimator 0 is the nominal builder, with or without the argument
  {
    BuildError err;
    auto a = build_scenario(c.d, &err);
    auto b = build(c.d, 0);
    if (!a || !b) return 1;
    CHECK(a->est == 0 && b->est == 0 && a->nvar == 1 && b->nvar == 1);
    CHECK(same_tables(a->pl, b->pl) && same_tables(a->mz, b->mz) && a->step == b->step && a->step_md == b->step_md);
    CHECK(same_tables(a->pl, a->mz));  // plant == model
    CHECK(a->pl.maxb == 4 && a->pl.maxa == 2 && compact_taps(a->pl) == 2);
    const DevScenario ds = dev_scenario(a.get());
    CHECK(ds.mdband == 1 && ds.est == 0 && ds.nvar == 1);
    // the estimator on the nominal plant: the same tables, the flag set
    auto e = build(c.d, MPCT_EST_OUTPUT_BIAS);
    if (!e) return 1;
    CHECK(e->est == MPCT_EST_OUTPUT_BIAS && e->nvar == 1);
    CHECK(same_tables(a->pl, e->pl) && same_tables(a->mz, e->mz) && a->step == e->step);
    CHECK(dev_scenario(e.get()).est == 1);
  }
  // single-variant estimator scenarios, one per variant
  std::unique_ptr<mpct_scenario> one[NV];
  for (int v = 0; v < NV; ++v) {
    mpct_scenario_desc d1 = c.d;
    d1.plant = c.V + NE * v;
    one[v] = build(d1, MPCT_EST_OUTPUT_BIAS);
    if (!one[v]) return 1;
    CHECK(one[v]->nvar == 1 && one[v]->ne == NE && (int)one[v]->pl.nb.size() == NE);
    CHECK(one[v]->mz.maxb == 4 && one[v]->mz.maxa == 2);  // the model's tables are the model's own
  }
  CHECK(one[0]->pl.maxb == 4 && one[0]->pl.maxa == 2 && compact_taps(one[0]->pl) == 2);
  CHECK(one[1]->pl.maxb == 7 && one[1]->pl.maxa == 2 && compact_taps(one[1]->pl) == 2);
  CHECK(one[2]->pl.maxb == 4 && one[2]->pl.maxa == 3 && compact_taps(one[2]->pl) == 3);
  // a plant shorter than the model keeps the model's row lengths: the parallel model shares the rings
  {
    Case cs;
    cs.V[2].delay = 0;
    mpct_scenario_desc ds = cs.d;
    ds.plant = cs.V;
    auto s = build(ds, MPCT_EST_OUTPUT_BIAS);
    if (!s) return 1;
    CHECK(s->pl.nb[2] == 2 && s->pl.maxb == 4 && s->pl.maxa == 2 && s->mz.maxb == 4);
  }

  // the three-variant scenario
  mpct_scenario_desc dm = c.d;
  dm.nplant = NV;
  dm.plant_var = c.V;
  auto sm = build(dm, MPCT_EST_OUTPUT_BIAS);
  if (!sm) return 1;
  CHECK(sm->nvar == NV && sm->ne == NE && sm->est == MPCT_EST_OUTPUT_BIAS);
  CHECK((int)sm->pl.nb.size() == NV * NE && (int)sm->pl.na.size() == NV * NE && (int)sm->pl.off.size() == NV * NE);
  CHECK(sm->pl.maxb == 7 && sm->pl.maxa == 3 && compact_taps(sm->pl) == 3);  // maxima over the variants
  CHECK((int)sm->pl.b.size() == NV * NE * 7 && (int)sm->pl.a.size() == NV * NE * 3);
  CHECK(same_tables(sm->mz, one[0]->mz) && compact_taps(sm->mz) == 2);
  if (g_bad) return 1;  // the sizes hold: the rows can be read
  for (int v = 0; v < NV; ++v)
    for (int e = 0; e < NE; ++e) CHECK(same_entry(sm->pl, (size_t)v * NE + e, one[v]->pl, e));
  CHECK(sm->pl.nb[NE + 2] == 7 && sm->pl.off[NE + 2] == 6);               // variant 1: delay 5, one leading zero
  CHECK(sm->pl.nb[2 * NE] == 4 && sm->pl.na[2 * NE] == 3 && sm->pl.off[2 * NE] == 1);  // variant 2: second order
  CHECK(sm->pl.b[(size_t)0 * 7 + 2] == 1.3 * 0.2);                          // variant 0: the larger gain
  {
    const PackedTables pk = pack_tables(sm.get());
    const DevScenario ds = pk.rebased(pk.blob.data());
    CHECK(ds.mdband == 1 && ds.est == 1 && ds.nvar == NV && ds.ne == NE);
    CHECK(ds.pl_maxb == 7 && ds.pl_maxa == 3 && ds.pl_maxbc == 3 && ds.mz_maxb == 4 && ds.mz_maxa == 2 &&
          ds.mz_maxbc == 2);
    size_t found = 0;
    for (const auto& t : pk.islots)
      if (t.field == &DevScenario::pl_nb || t.field == &DevScenario::pl_na || t.field == &DevScenario::pl_off) {
        CHECK(t.bytes == (size_t)NV * NE * 4 && t.off + t.bytes <= pk.blob.size());
        ++found;
      }
    for (const auto& t : pk.dslots) {
      if (t.field == &DevScenario::pl_b) {
        CHECK(t.bytes == (size_t)NV * NE * 7 * 8 && t.off + t.bytes <= pk.blob.size());
        ++found;
      }
      if (t.field == &DevScenario::pl_a) {
        CHECK(t.bytes == (size_t)NV * NE * 3 * 8 && t.off + t.bytes <= pk.blob.size());
        ++found;
      }
    }
    CHECK(found == 5);
    if (found == 5 && !g_bad) {
      CHECK(std::memcmp(ds.pl_nb, sm->pl.nb.data(), (size_t)NV * NE * 4) == 0);
      CHECK(std::memcmp(ds.pl_off, sm->pl.off.data(), (size_t)NV * NE * 4) == 0);
      CHECK(std::memcmp(ds.pl_b, sm->pl.b.data(), sm->pl.b.size() * 8) == 0);
      CHECK(std::memcmp(ds.pl_a, sm->pl.a.data(), sm->pl.a.size() * 8) == 0);
    }
    std::printf("band 2x(1+1) x %d variants: pl_maxb %d, pl_maxa %d, compact taps %d, %zu blob bytes\n", NV, ds.pl_maxb,
                ds.pl_maxa, ds.pl_maxbc, pk.blob.size());
  }

  // the longest entry the history rings hold (kMaxTaps taps) builds; one sample more does not
  {
    Case cd;
    cd.V[NE + 2].delay = kMaxTaps - 2;
    mpct_scenario_desc dd = cd.d;
    dd.nplant = NV;
    dd.plant_var = cd.V;
    auto sd = build(dd, MPCT_EST_OUTPUT_BIAS);
    if (!sd) return 1;
    CHECK(sd->pl.maxb == kMaxTaps);
    cd.V[NE + 2].delay = kMaxTaps - 1;
    expect_reject(dd, MPCT_EST_OUTPUT_BIAS, MPCT_ERANGE, "plant entry too long for the device history rings",
                  "variant past the rings");
  }
  // what stays rejected, and by which entry
  {
    mpct_scenario_desc dx = dm;
    expect_reject(dx, 0, MPCT_EINVAL, "mdband excludes dtc, plant-only disturbances and plant variants",
                  "variants without the estimator");
    dx = c.d;
    dx.plant = c.V;
    expect_reject(dx, 0, MPCT_ERANGE, "mdband: plant must equal the model (the toolbox estimator is not restated)",
                  "mismatch without the estimator");
    dx = dm;
    dx.dtc = 1;
    expect_reject(dx, MPCT_EST_OUTPUT_BIAS, MPCT_EINVAL,
                  "mdband excludes dtc, plant-only disturbances and plant variants", "estimator with dtc");
    dx = dm;
    dx.nq = 1;
    expect_reject(dx, MPCT_EST_OUTPUT_BIAS, MPCT_EINVAL,
                  "mdband excludes dtc, plant-only disturbances and plant variants", "estimator with nq");
    // the estimator argument itself, checked before anything else of the descriptor
    expect_reject(dm, 2, MPCT_EINVAL, "unknown estimator id", "unknown estimator id");
    dx = dm;
    dx.mdband = 0;
    expect_reject(dx, MPCT_EST_OUTPUT_BIAS, MPCT_EINVAL,
                  "the output-bias estimator belongs to the band kernel (mdband = 1)", "estimator without mdband");
    dx.mdband = 1;
    dx.abi_version = 2;  // a descriptor from before the band fields: mdband is not read
    expect_reject(dx, MPCT_EST_OUTPUT_BIAS, MPCT_EINVAL,
                  "the output-bias estimator belongs to the band kernel (mdband = 1)", "estimator on an ABI-2 descriptor");
    // a model longer than the rings is refused by the same length check (the rows hold it too)
    Case cl;
    cl.M[2].delay = kMaxTaps - 1;
    dx = cl.d;
    dx.nplant = NV;
    dx.plant_var = cl.V;
    expect_reject(dx, MPCT_EST_OUTPUT_BIAS, MPCT_ERANGE, "plant entry too long for the device history rings",
                  "model past the rings");
  }

  return finish();
}
