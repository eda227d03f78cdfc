// Stand-alone check of the host-only scenario precompute (csrc/scenario_tables.h), built with the
// address, leak and undefined-behaviour sanitizers by tests/test_host_tables.py.  No GPU is used.
//   valid descriptors: build, pack, every table 256-B aligned and inside the blob, destroy;
//   rejections: one mutated descriptor per error message of the two builders, each printed as
//               `rejected <code> "<message>"` (the pytest checks every message of the header is there).
// Exit status 0 when every expectation held.
#include "scenario_tables.h"

#include <cstdio>
#include <functional>
#include <limits>
#include <type_traits>

using namespace mpct;

static int g_bad = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_bad;                                                     \
    }                                                              \
  } while (0)

static const double kInf = std::numeric_limits<double>::infinity();

// build, pack, check the packed layout; returns the packed scenario's DevScenario (pointers null)
static DevScenario check_valid(const char* name, std::unique_ptr<mpct_scenario> s, const BuildError& err,
                               size_t* lanes = nullptr) {
  if (!s) {
    std::printf("FAILED %s: rejected %d \"%s\"\n", name, err.code, err.msg.c_str());
    ++g_bad;
    return DevScenario{};
  }
  const PackedTables pk = pack_tables(s.get());
  size_t tables = 0;
  auto slot_ok = [&](size_t off, size_t bytes) {
    CHECK(off % 256 == 0);
    CHECK(off + bytes <= pk.blob.size());
    ++tables;
  };
  for (const auto& t : pk.dslots) slot_ok(t.off, t.bytes);
  for (const auto& t : pk.islots) slot_ok(t.off, t.bytes);
  // the rebased pointers read the host tables back
  const DevScenario ds = pk.rebased(pk.blob.data());
  CHECK(ds.yref && std::memcmp(ds.yref, s->yref.data(), s->yref.size() * 8) == 0);
  if (!s->nmpc) {
    CHECK(std::memcmp(ds.step, s->step.data(), s->step.size() * 8) == 0);
    CHECK(std::memcmp(ds.pl_b, s->pl.b.data(), s->pl.b.size() * 8) == 0);
    CHECK(std::memcmp(ds.pl_off, s->pl.off.data(), s->pl.off.size() * 4) == 0);
    CHECK(ds.nd == s->nd + s->nq && ds.nin == s->npin);
  }
  const DevScenario q = dev_scenario(s.get());  // what the queries start from: the same scalars
  CHECK(q.small == ds.small && q.small_dtc == ds.small_dtc && q.regpath == ds.regpath && q.sm_ke == ds.sm_ke &&
        q.nd == ds.nd && q.step == nullptr);
  if (lanes)
    for (const auto& t : pk.islots)
      if (t.field == &DevScenario::sm_hoff) *lanes = t.bytes / 4;
  // the dispatch key's Gram tables: none for NMPC, band and my > 4 scenarios, and then no pointer either
  std::vector<double> gram;
  gram_tables(s.get(), gram);
  CHECK(gram.empty() == (s->nmpc || s->mdband || s->my > 4));
  CHECK((ds.gram != nullptr) == !gram.empty());
  CHECK(gram.empty() || std::memcmp(ds.gram, gram.data(), gram.size() * 8) == 0);
  std::printf("valid %s: %zu tables, %zu blob bytes, small %d small_dtc %d regpath %d, gram %zu doubles\n", name, tables,
              pk.blob.size(), ds.small, ds.small_dtc, ds.regpath, gram.size());
  return ds;
}

static void expect_reject(std::unique_ptr<mpct_scenario> s, const BuildError& err, int code, const char* msg) {
  std::printf("rejected %d \"%s\"\n", err.code, err.msg.c_str());
  CHECK(!s);
  CHECK(err.code == code);
  CHECK(err.msg == msg);
}

// ---- Shell 3x3 (tests/c_abi/mpct_c_demo.c: the saved mpc object's scaled discrete tf), abi-5 path:
// no CARIMA tables, the library derives them
struct Shell {
  static constexpr int NIT = 40;
  double num[9][2] = {{0.02313052619372795, 0.06667958558934375}, {0.0, 0.013710194313372143},
                      {0.02089018186516949, 0.06022122704814364}, {0.058828715846932514, 0.0565220089046257},
                      {0.02173580108248058, 0.021023216763849436}, {0.0294987546979058, 0.08419778882992246},
                      {0.0, 0.1963360266878832},                  {0.032116113806741245, 0.03068897122230742},
                      {0.0, 0.3338832924071783}};
  double den[9][2] = {{1.0, -0.9231163463866358}, {1.0, -0.9355069850316178}, {1.0, -0.9231163463866358},
                      {1.0, -0.9231163463866358}, {1.0, -0.9355069850316178}, {1.0, -0.9048374180359595},
                      {1.0, -0.8858460329277068}, {1.0, -0.9131007162822624}, {1.0, -0.8101577349324267}};
  int32_t delay[9] = {7, 7, 7, 5, 4, 4, 5, 6, 0};
  double umin[3] = {-1.510877401316376, -3.628338208043142, -2.4288171452857927};
  double umax[3] = {0.755438700658188, 1.814169104021571, 1.2144085726428964};
  double dumax[3] = {0.0755438700658188, 0.18141691040215713, 0.12144085726428963};
  double dumin[3];
  int32_t n1[3] = {1, 1, 1};
  mpct_dtf P[9];
  std::vector<double> yref = std::vector<double>(3 * NIT, 0.1);
  mpct_scenario_desc d{};
  Shell() {
    for (int e = 0; e < 9; ++e) P[e] = {2, num[e], den[e], delay[e]};
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
  Shell(const Shell&) = delete;
};

// ---- synthetic 2x2 first-order DTC plant: delays, infinite bounds, two plant variants, one
// plant-only disturbance, a two-tap filter; explicit CARIMA tables (rows share a denominator)
struct Dtc {
  static constexpr int NIT = 30;
  double mnum[4][2] = {{0.0, 0.10}, {0.0, 0.05}, {0.0, 0.04}, {0.0, 0.12}};
  double mden[4][2] = {{1.0, -0.9}, {1.0, -0.9}, {1.0, -0.8}, {1.0, -0.8}};
  int32_t mdelay[4] = {1, 2, 2, 1};
  double vnum[8][2] = {{0.0, 0.10}, {0.0, 0.05}, {0.0, 0.04}, {0.0, 0.12},
                       {0.0, 0.11}, {0.0, 0.06}, {0.0, 0.05}, {0.0, 0.10}};
  double vden[8][2] = {{1.0, -0.9}, {1.0, -0.9}, {1.0, -0.8}, {1.0, -0.8},
                       {1.0, -0.88}, {1.0, -0.91}, {1.0, -0.82}, {1.0, -0.79}};
  double qnum[2][2] = {{0.0, 0.05}, {0.0, 0.03}}, qden[2][2] = {{1.0, -0.8}, {1.0, -0.7}};
  double fnum[2][2] = {{0.5, -0.3}, {0.4, -0.2}}, fden[2][2] = {{1.0, -0.8}, {1.0, -0.8}};
  mpct_dtf model[4], plant_var[8], dist[2], filter[2];
  int32_t n1[2] = {2, 2};  // dmin_i + 1
  std::vector<int32_t> na = {1, 1}, nb = {0, 0, 0, 0}, dp = {0, 1, 1, 0};
  std::vector<double> A = {1.0, -0.9, 1.0, -0.8}, B = {0.10, 0.05, 0.04, 0.12};
  double dumin[2] = {-kInf, -kInf}, dumax[2] = {kInf, kInf}, umin[2] = {-kInf, -kInf}, umax[2] = {kInf, kInf};
  std::vector<double> yref = std::vector<double>(2 * NIT, 0.5);
  mpct_scenario_desc d{};
  Dtc() {
    for (int e = 0; e < 4; ++e) model[e] = {2, mnum[e], mden[e], mdelay[e]};
    for (int e = 0; e < 8; ++e) plant_var[e] = {2, vnum[e], vden[e], mdelay[e % 4]};
    for (int e = 0; e < 2; ++e) dist[e] = {2, qnum[e], qden[e], 0};
    for (int e = 0; e < 2; ++e) filter[e] = {2, fnum[e], fden[e], 0};
    d.abi_version = MPCT_ABI_VERSION;
    d.my = d.nu = 2;
    d.nit = NIT;
    d.n2_max = 10;
    d.nu_max = 4;
    d.vns_ink = 10;
    d.n1 = n1;
    d.plant = d.model = model;
    d.na = na.data();
    d.carima_A = A.data();
    d.nb = nb.data();
    d.carima_B = B.data();
    d.dp = dp.data();
    d.du_min = dumin;
    d.du_max = dumax;
    d.u_min = umin;
    d.u_max = umax;
    d.yref = yref.data();
    d.dtc = 1;
    d.filter = filter;
    d.nq = 1;
    d.dist = dist;
    d.nplant = 2;
    d.plant_var = plant_var;
  }
  Dtc(const Dtc&) = delete;
};

// ---- synthetic mdband scenario: 2 outputs, 1 MV, 1 MD, plant == model
struct Band {
  static constexpr int NIT = 30;
  double num[4][2] = {{0.0, 0.10}, {0.0, 0.05}, {0.0, 0.04}, {0.0, 0.12}};
  double den[4][2] = {{1.0, -0.9}, {1.0, -0.7}, {1.0, -0.8}, {1.0, -0.6}};
  double pnum[2] = {0.0, 0.2};  // another plant entry, for the plant != model rejection
  int32_t delay[4] = {1, 0, 2, 1};
  mpct_dtf model[4], plant[4];
  int32_t n1[2] = {1, 1};
  double dumin[1] = {-0.5}, dumax[1] = {0.5}, umin[1] = {-2.0}, umax[1] = {2.0};
  double ymin[2] = {-1.0, -kInf}, ymax[2] = {1.0, kInf}, ecrmin[2] = {1.0, 1.0}, ecrmax[2] = {1.0, 0.0};
  double yscale[2] = {1.0, 2.0}, uscale[1] = {4.0};
  std::vector<double> yref = std::vector<double>(2 * NIT, 0.5);
  mpct_scenario_desc d{};
  Band() {
    for (int e = 0; e < 4; ++e) plant[e] = model[e] = {2, num[e], den[e], delay[e]};
    d.abi_version = MPCT_ABI_VERSION;
    d.my = 2;
    d.nu = d.nd = 1;
    d.nit = NIT;
    d.n2_max = 8;
    d.nu_max = 3;
    d.weights_squared = 1;
    d.vns_ink = 10;
    d.n1 = n1;
    d.plant = plant;
    d.model = model;
    d.du_min = dumin;
    d.du_max = dumax;
    d.u_min = umin;
    d.u_max = umax;
    d.yref = yref.data();
    d.mdband = 1;
    d.y_min = ymin;
    d.y_max = ymax;
    d.ecr_min = ecrmin;
    d.ecr_max = ecrmax;
    d.y_scale = yscale;
    d.u_scale = uscale;
    d.rho_ecr = 1e5;
  }
  Band(const Band&) = delete;
};

// ---- Van de Vusse NMPC (tests/c_abi/mpct_c_demo.c: VanDeVusse_NMPC.m:54-90)
struct Vdv {
  static constexpr int NIT = 20;
  double x0[3] = {1.246290177008599, 0.9052268854543595, 134.95095689423889};
  double u0[2] = {20.0, 130.0}, umin[2] = {0.0, 40.0}, umax[2] = {150.0, 150.0};
  double xmin[3] = {0.0, 0.0, 40.0}, xmax[3] = {6.0, 1.2, 150.0};
  double ys[2] = {1.2, 110.0}, us[2] = {150.0, 110.0};
  int32_t xc[2] = {2, 3};
  std::vector<double> yref = std::vector<double>(2 * NIT, 1.0);
  mpct_nmpc_desc d{};
  Vdv() {
    d.abi_version = MPCT_ABI_VERSION;
    d.model = MPCT_NMPC_VANDEVUSSE;
    d.nx = 3;
    d.ny = d.nu = 2;
    d.xc = xc;
    d.ts = 0.05;
    d.nsub = 10;
    d.x0 = x0;
    d.u0 = u0;
    d.u_min = umin;
    d.u_max = umax;
    d.x_min = xmin;
    d.x_max = xmax;
    d.y_scale = ys;
    d.u_scale = us;
    d.n_max = 31;
    d.nu_max = 15;
    d.nit = NIT;
    d.yref = yref.data();
    d.vns_ink = 10;
  }
  Vdv(const Vdv&) = delete;
};

// a fresh base descriptor, one fault planted, the builder's answer checked
template <class Case>
static void rejects(int code, const char* msg, const std::function<void(Case&)>& plant_fault, int estimator = 0) {
  Case c;
  plant_fault(c);
  BuildError err;
  if constexpr (std::is_same<Case, Vdv>::value)
    expect_reject(build_nmpc_scenario(c.d, &err), err, code, msg);
  else
    expect_reject(build_scenario(c.d, &err, estimator), err, code, msg);
}

int main() {
  {
    Shell c;
    BuildError err;
    const DevScenario ds = check_valid("shell3x3 (derived CARIMA)", build_scenario(c.d, &err), err);
    CHECK(ds.small == 1 && ds.regpath == 1);
  }
  {
    Dtc c;
    BuildError err;
    size_t lanes = 0;
    DevScenario ds = check_valid("dtc 2x2", build_scenario(c.d, &err), err, &lanes);
    CHECK(ds.small_dtc == 1 && ds.small == 0 && ds.nvar == 2 && ds.nd == 1);
    CHECK(lanes == 2 * 64);
    c.dumax[1] = 0.25;  // one finite move bound: the QP is needed, not a small DTC plant
    ds = check_valid("dtc 2x2, bounded", build_scenario(c.d, &err), err, &lanes);
    CHECK(ds.small_dtc == 0 && ds.small == 0 && lanes == 0);
  }
  {
    Band c;
    BuildError err;
    const DevScenario ds = check_valid("mdband 2x(1+1)", build_scenario(c.d, &err), err);
    CHECK(ds.mdband == 1 && ds.nd == 1 && ds.small == 0 && ds.regpath == 0);
  }
  {
    Vdv c;
    BuildError err;
    const DevScenario ds = check_valid("van de vusse nmpc", build_nmpc_scenario(c.d, &err), err);
    CHECK(ds.nmpc == 1 && ds.my == 2 && ds.nu == 2);
    CHECK(ds.pl_maxb == 0 && ds.pl_maxa == 0 && ds.mz_maxb == 1 && ds.mz_maxa == 1);  // no entry tables
  }

  // ---- build_scenario's rejections, in the order of its checks
  rejects<Band>(MPCT_EINVAL, "unknown estimator id", [](Band&) {}, 2);
  rejects<Shell>(MPCT_EINVAL, "the output-bias estimator belongs to the band kernel (mdband = 1)", [](Shell&) {},
                 MPCT_EST_OUTPUT_BIAS);
  rejects<Shell>(MPCT_EINVAL, "bad model entry", [](Shell& c) { c.P[4].den = nullptr; });  // abi-5 derivation
  rejects<Dtc>(MPCT_EINVAL, "bad model entry", [](Dtc& c) { c.model[1].len = 0; });      // step table
  rejects<Band>(MPCT_EINVAL, "bad model entry", [](Band& c) { c.model[1].delay = -1; });  // an MD column
  rejects<Shell>(MPCT_EINVAL, "abi_version mismatch", [](Shell& c) { c.d.abi_version = MPCT_ABI_VERSION + 1; });
  rejects<Band>(MPCT_EINVAL, "mdband excludes dtc, plant-only disturbances and plant variants",
                [](Band& c) { c.d.dtc = 1; });
  rejects<Band>(MPCT_EINVAL, "mdband needs y_min, y_max, ecr_min, ecr_max", [](Band& c) { c.d.ecr_max = nullptr; });
  rejects<Dtc>(MPCT_EINVAL, "nplant > 1 needs plant_var", [](Dtc& c) { c.d.plant_var = nullptr; });
  rejects<Dtc>(MPCT_EINVAL, "nq > 0 needs dist", [](Dtc& c) { c.d.dist = nullptr; });
  rejects<Shell>(MPCT_EINVAL, "non-positive dimension", [](Shell& c) { c.d.nit = 0; });
  rejects<Dtc>(MPCT_ERANGE, "too many outputs/inputs", [](Dtc& c) { c.d.my = kMaxOut + 1; });
  rejects<Dtc>(MPCT_ERANGE, "measured disturbances (nd > 0) need the mdband kernel (mdband = 1)",
               [](Dtc& c) { c.d.nd = 1; });
  rejects<Band>(MPCT_ERANGE, "nu*nu_max (+1 eps row) > 64 (one wavefront of QP rows)", [](Band& c) { c.d.nu_max = 64; });
  rejects<Shell>(MPCT_EINVAL, "null table pointer", [](Shell& c) { c.d.u_max = nullptr; });
  rejects<Dtc>(MPCT_EINVAL, "null CARIMA table pointer", [](Dtc& c) { c.d.nb = nullptr; });
  rejects<Dtc>(MPCT_ERANGE, "too many plant inputs", [](Dtc& c) { c.d.nq = kMaxIn - 1; });
  rejects<Dtc>(MPCT_EINVAL, "n1[i] must be >= 1", [](Dtc& c) { c.n1[1] = 0; });
  rejects<Band>(MPCT_EINVAL, "mdband predicts over the toolbox window: n1[i] must be 1", [](Band& c) { c.n1[0] = 2; });
  rejects<Dtc>(MPCT_EINVAL, "na < 0", [](Dtc& c) { c.na[1] = -1; });
  rejects<Dtc>(MPCT_EINVAL, "nb/dp < 0", [](Dtc& c) { c.dp[2] = -1; });
  rejects<Dtc>(MPCT_ERANGE, "free-response state too large", [](Dtc& c) { c.dp[0] = 300; });
  rejects<Dtc>(MPCT_ERANGE, "nu*nu_max must be < 64 (one QP row per lane)", [](Dtc& c) { c.d.nu_max = 32; });
  rejects<Dtc>(MPCT_EINVAL, "carima_A[i][0] must be 1", [](Dtc& c) { c.A[2] = 2.0; });
  rejects<Dtc>(MPCT_EINVAL, "bad plant entry", [](Dtc& c) { c.dist[1].num = nullptr; });
  rejects<Dtc>(MPCT_EINVAL, "plant has direct feedthrough from an MV (algebraic loop)", [](Dtc& c) {
    c.plant_var[4].delay = 0;
    c.vnum[4][0] = 0.1;
  });
  rejects<Dtc>(MPCT_ERANGE, "past-control register longer than the device supports (16)",
               [](Dtc& c) { c.dp[1] = kMaxDum + 1; });
  rejects<Dtc>(MPCT_ERANGE, "CARIMA denominator order too high for the device (na <= 7)", [](Dtc& c) {
    c.A = {1.0, -0.9, 1.0, -0.8, 0, 0, 0, 0, 0, 0, 0};
    c.d.carima_A = c.A.data();
    c.na[1] = kYeHist;
  });
  rejects<Dtc>(MPCT_ERANGE, "plant entry too long for the device history rings",
               [](Dtc& c) { c.plant_var[5].delay = kMaxTaps; });
  rejects<Dtc>(MPCT_EINVAL, "DTC: model delay below dmin (n1 - 1)", [](Dtc& c) { c.n1[0] = 3; });
  rejects<Dtc>(MPCT_ERANGE, "DTC: model entry too long for the device history rings",
               [](Dtc& c) { c.model[1].delay = kMaxTaps; });
  rejects<Dtc>(MPCT_ERANGE, "DTC: filter order too high (len <= 8)", [](Dtc& c) { c.filter[0].len = kYeHist + 1; });
  rejects<Dtc>(MPCT_EINVAL, "DTC: bad filter entry (delay must be 0)", [](Dtc& c) { c.filter[1].delay = 1; });
  rejects<Band>(MPCT_ERANGE, "mdband: plant must equal the model (the toolbox estimator is not restated)",
                [](Band& c) { c.plant[3].num = c.pnum; });
  rejects<Band>(MPCT_EINVAL, "mdband: bad output bound / ECR / scale factor", [](Band& c) { c.ecrmin[1] = -1.0; });
  rejects<Band>(MPCT_EINVAL, "mdband: bad MV scale factor", [](Band& c) { c.uscale[0] = 0.0; });
  rejects<Band>(MPCT_EINVAL, "mdband: rho_ecr must be > 0", [](Band& c) { c.d.rho_ecr = 0.0; });
  rejects<Shell>(MPCT_EINVAL, "bounds must contain 0 (nominal u = 0 must be feasible)", [](Shell& c) { c.umin[1] = 0.5; });

  // ---- build_nmpc_scenario's rejections, in the order of its checks
  rejects<Vdv>(MPCT_EINVAL, "abi_version mismatch", [](Vdv& c) { c.d.abi_version = 3; });
  rejects<Vdv>(MPCT_EINVAL, "unknown NMPC model id", [](Vdv& c) { c.d.model = 2; });
  rejects<Vdv>(MPCT_EINVAL, "the Van de Vusse model has nx = 3, nu = 2", [](Vdv& c) { c.d.nx = 4; });
  rejects<Vdv>(MPCT_ERANGE, "ny must be 1 or 2", [](Vdv& c) { c.d.ny = 3; });
  rejects<Vdv>(MPCT_EINVAL, "non-positive dimension", [](Vdv& c) { c.d.n_max = 0; });
  rejects<Vdv>(MPCT_ERANGE, "nu*nu_max > 32", [](Vdv& c) { c.d.nu_max = 17; });
  rejects<Vdv>(MPCT_EINVAL, "ts must be > 0 and nsub >= 1", [](Vdv& c) { c.d.nsub = 0; });
  rejects<Vdv>(MPCT_EINVAL, "null table pointer", [](Vdv& c) { c.d.x_min = nullptr; });
  rejects<Vdv>(MPCT_EINVAL, "xc out of range (1-based state index)", [](Vdv& c) { c.xc[1] = 4; });
  rejects<Vdv>(MPCT_EINVAL, "u_min must be < u_max", [](Vdv& c) { c.umin[0] = 150.0; });
  rejects<Vdv>(MPCT_EINVAL, "u_scale must be > 0", [](Vdv& c) { c.us[1] = 0.0; });
  rejects<Vdv>(MPCT_EINVAL, "y_scale must be > 0", [](Vdv& c) { c.ys[0] = -1.0; });

  std::printf(g_bad ? "%d expectation(s) failed\n" : "ok\n", g_bad);
  return g_bad ? 1 : 0;
}
