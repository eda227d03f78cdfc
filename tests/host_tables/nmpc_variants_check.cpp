// Stand-alone check of the NMPC kernel's plant-variant table (csrc/scenario_tables.h
// build_nmpc_scenario with nplant >= 1), built with the address, leak and undefined-behaviour
// sanitizers by tests/test_nmpc_variants.py.  No GPU is used.
//   Three variants with their own start states: the table is [nvar][NM_NPAR + 3], parameters then x0;
//   the packed blob holds it and DevScenario::nmv points at it; the row the kernel reads for reference
//   set k is k % nvar.  Without plant_x0 every row ends with the descriptor's x0.  nplant = 0 builds the
//   nominal scenario: no table, a null pointer, nvar = 1.  (The arguments' MPCT_EINVAL checks are made by
//   the entry point, mpct_nmpc_scenario_create_var: tests/test_nmpc_variants.py drives them.)
// Exit status 0 when every expectation held.
#include "check.h"


struct Case {
  static constexpr int NIT = 12, NV = 3;
  double x0[3] = {1.235, 0.9, 134.14}, u0[2] = {20.0, 130.0};
  double umin[2] = {0.0, 40.0}, umax[2] = {150.0, 150.0};
  double xmin[3] = {0.0, 0.0, 40.0}, xmax[3] = {6.0, 1.2, 150.0};
  double sy[2] = {1.2, 110.0}, su[2] = {150.0, 110.0};
  int32_t xc[2] = {2, 3};
  std::vector<double> yref = std::vector<double>(2 * NIT, 1.0);
  double pp[NV * NM_NPAR], px0[NV * 3];
  mpct_nmpc_desc d{};
  Case() {
    for (int k = 0; k < NV; ++k) {
      for (int i = 0; i < NM_NPAR; ++i) pp[k * NM_NPAR + i] = kVdvParams[i] * (1.0 + 0.01 * k * (i + 1));
      for (int i = 0; i < 3; ++i) px0[k * 3 + i] = x0[i] + 0.1 * (k + 1) + 0.01 * i;
    }
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
    d.y_scale = sy;
    d.u_scale = su;
    d.n_max = 9;
    d.nu_max = 4;
    d.nit = NIT;
    d.yref = yref.data();
  }
  Case(const Case&) = delete;
};

static std::unique_ptr<mpct_scenario> build_var(const mpct_nmpc_desc& d, int nplant, const double* pp, const double* px0) {
  BuildError err;
  auto s = build_nmpc_scenario(d, &err, nplant, pp, px0);
  if (!s) {
    std::printf("FAILED: rejected %d \"%s\"\n", err.code, err.msg.c_str());
    ++g_bad;
  }
  return s;
}

int main() {
  (void)&build;  // check.h's linear-scenario builder: not used here
  Case c;
  constexpr int W = NM_NPAR + 3;
  // nominal: what build_nmpc_scenario built before it took variants
  auto nom = build_var(c.d, 0, nullptr, nullptr);
  if (!nom) return 1;
  CHECK(nom->nmpc == 1 && nom->nvar == 1 && nom->nmv.empty());
  {
    const PackedTables p = pack_tables(nom.get());
    const DevScenario ds = p.rebased(p.blob.data());
    CHECK(ds.nmv == nullptr && ds.nm != nullptr && ds.nvar == 1);
    for (int i = 0; i < NM_NPAR; ++i) CHECK(ds.nm[i] == kVdvParams[i]);  // params = NULL: the reference's values
  }

  // three variants with their own start states
  auto var = build_var(c.d, Case::NV, c.pp, c.px0);
  if (!var) return 1;
  CHECK(var->nvar == Case::NV && var->nmv.size() == (size_t)Case::NV * W);
  CHECK(var->nm == nom->nm);  // the controller's table does not depend on the variants
  const PackedTables p = pack_tables(var.get());
  const DevScenario ds = p.rebased(p.blob.data());
  CHECK(ds.nmv != nullptr && ds.nvar == Case::NV);
  CHECK((reinterpret_cast<const char*>(ds.nmv) - p.blob.data()) % 256 == 0);
  bool in_blob = false;
  for (const auto& t : p.dslots)
    if (t.field == &DevScenario::nmv) in_blob = t.bytes == sizeof(double) * Case::NV * W && t.off + t.bytes <= p.blob.size();
  CHECK(in_blob);
  for (int kref = 0; kref < 7; ++kref) {
    const int v = kref % Case::NV;
    const double* row = ds.nmv + (size_t)(kref % ds.nvar) * W;  // the kernel's row of reference set kref
    for (int i = 0; i < NM_NPAR; ++i) CHECK(row[i] == c.pp[v * NM_NPAR + i]);
    for (int i = 0; i < 3; ++i) CHECK(row[NM_NPAR + i] == c.px0[v * 3 + i]);
  }
  std::printf("nmpc %d variants: table [%d][%d], %zu bytes in the blob\n", Case::NV, ds.nvar, W,
              sizeof(double) * var->nmv.size());

  // plant_x0 = NULL: every variant starts at the descriptor's x0
  auto vx = build_var(c.d, Case::NV, c.pp, nullptr);
  if (!vx) return 1;
  for (int v = 0; v < Case::NV; ++v)
    for (int i = 0; i < 3; ++i) CHECK(vx->nmv[(size_t)v * W + NM_NPAR + i] == c.x0[i]);
  // one variant is a variant scenario too (not the nominal one)
  auto v1 = build_var(c.d, 1, c.pp + NM_NPAR, nullptr);
  if (!v1) return 1;
  CHECK(v1->nvar == 1 && v1->nmv.size() == (size_t)W && v1->nmv[0] == c.pp[NM_NPAR]);

  return finish();
}
