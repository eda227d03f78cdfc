// Stand-alone check of the prologue's pre-factored rows (csrc/scenario_tables.h qr_tables), built with
// the address, leak and undefined-behaviour sanitizers by tests/test_qr_tables.py.  No GPU, no HIP
// runtime.  For Shell 3x3 (n2max = 30, numax = 5) and a synthetic 2x2 plant with dead time, over every
// cell (N2, Nu) and output i, against G_i and Phi_i formed here in long double from the scenario's step
// and free-response tables:
//   R_i'R_i = G_i'G_i and R_i'T_i = G_i'Phi_i to 1e-13 of the matrices' norms (|G_i|_F^2 and
//   |G_i|_F |Phi_i|_F; the Gram check's tolerance, the same kind of host float64 arithmetic),
//   the stored row my k + i is zero left of column k,
//   the cell index: offsets in order, rows my min(N2, M), the cells N2 < M among them,
//   no table above the byte cap, for a kind the prologue does not serve, or switched off.
// Prints one line per scenario and a last line "ok"; exit status 1 when an expectation failed.
#include "scenario_tables.h"

#include <cstdio>

using namespace mpct;

static int g_bad = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_bad;                                                     \
    }                                                              \
  } while (0)

// a first-order my x nu plant (tests/host_tables/host_tables_check.cpp's Shell numbers for Shell 3x3)
struct Plant {
  int my, nu;
  std::vector<std::vector<double>> num, den;
  std::vector<int32_t> delay, n1;
  std::vector<mpct_dtf> P;
  std::vector<double> dumin, dumax, umin, umax, yref;
  mpct_scenario_desc d{};
  Plant(int my_, int nu_, const std::vector<std::vector<double>>& num_, const std::vector<double>& pole,
        const std::vector<int32_t>& delay_, int n2max, int numax)
      : my(my_), nu(nu_), num(num_), delay(delay_), n1(my_, 1) {
    for (double p : pole) den.push_back({1.0, -p});
    for (int e = 0; e < my * nu; ++e) P.push_back({2, num[e].data(), den[e].data(), delay[e]});
    dumin.assign(nu, -0.1);
    dumax.assign(nu, 0.1);
    umin.assign(nu, -1.0);
    umax.assign(nu, 1.0);
    yref.assign((size_t)my * 20, 0.1);
    d.abi_version = MPCT_ABI_VERSION;
    d.my = my;
    d.nu = nu;
    d.nit = 20;
    d.n2_max = n2max;
    d.nu_max = numax;
    d.weights_squared = 1;
    d.vns_ink = 10;
    d.n1 = n1.data();
    d.plant = d.model = P.data();
    d.du_min = dumin.data();
    d.du_max = dumax.data();
    d.u_min = umin.data();
    d.u_max = umax.data();
    d.yref = yref.data();
  }
  Plant(const Plant&) = delete;
};

static void check_scenario(const char* name, const mpct_scenario* s, long long want_doubles) {
  std::vector<double> q;
  std::vector<int> off;
  qr_tables(s, q, off);
  const int my = s->my, nu = s->nu, nx = s->nx, n2max = s->n2max, numax = s->numax;
  CHECK(!q.empty() && (int)off.size() == n2max * numax);
  if (q.empty() || (int)off.size() != n2max * numax) return;
  long long next = 0, cells = 0, short_cells = 0, zero_cols = 0, left_nonzero = 0;
  long double worst_rr = 0.0L, worst_rt = 0.0L;
  for (int N2 = 1; N2 <= n2max; ++N2)
    for (int Nu = 1; Nu <= numax; ++Nu) {
      const int o = off[(size_t)(N2 - 1) * numax + (Nu - 1)];
      if (Nu > N2) {
        CHECK(o == -1);
        continue;
      }
      const int M = nu * Nu, W = M + nx, rn = std::min(N2, M);
      CHECK(o == next);  // the closed form: cells in (N2, Nu) order, my min(N2, M) rows of M + nx
      next += (long long)my * rn * W;
      CHECK(next <= (long long)q.size());
      if (o != next - (long long)my * rn * W || next > (long long)q.size()) return;
      ++cells;
      short_cells += N2 < M;
      for (int i = 0; i < my; ++i) {
        // G_i and Phi_i as the streamed prologue forms them (gpc_prologue.h fetch)
        std::vector<long double> G((size_t)N2 * M), F((size_t)N2 * nx);
        long double g2 = 0.0L, f2 = 0.0L;
        for (int r = 0; r < N2; ++r) {
          for (int c = 0; c < M; ++c) {
            const int n = c / Nu, tt = s->n1[i] + r - (c - n * Nu);
            G[(size_t)r * M + c] = tt >= 0 ? s->step[((size_t)i * nu + n) * s->tlen + tt] : 0.0;
            g2 += G[(size_t)r * M + c] * G[(size_t)r * M + c];
          }
          for (int c = 0; c < nx; ++c) {
            F[(size_t)r * nx + c] = s->phid[((size_t)i * n2max + r) * nx + c];
            f2 += F[(size_t)r * nx + c] * F[(size_t)r * nx + c];
          }
        }
        for (int c = 0; c < M; ++c) {
          bool zero = true;
          for (int r = 0; r < N2; ++r) zero = zero && G[(size_t)r * M + c] == 0.0L;
          zero_cols += zero;
        }
        auto row = [&](int k) { return q.data() + o + ((size_t)k * my + i) * W; };
        for (int k = 0; k < rn; ++k)
          for (int c = 0; c < k; ++c) left_nonzero += row(k)[c] != 0.0;
        const long double fn = std::sqrt(g2 * f2);
        for (int a = 0; a < M; ++a) {
          for (int b = 0; b < M; ++b) {
            long double want = 0.0L, got = 0.0L;
            for (int r = 0; r < N2; ++r) want += G[(size_t)r * M + a] * G[(size_t)r * M + b];
            for (int k = 0; k < rn; ++k) got += (long double)row(k)[a] * row(k)[b];
            const long double e = std::fabs(got - want);
            if (g2 > 0.0L) worst_rr = std::max(worst_rr, e / g2);
            CHECK(e <= 1e-13L * g2);
          }
          for (int b = 0; b < nx; ++b) {
            long double want = 0.0L, got = 0.0L;
            for (int r = 0; r < N2; ++r) want += G[(size_t)r * M + a] * F[(size_t)r * nx + b];
            for (int k = 0; k < rn; ++k) got += (long double)row(k)[a] * row(k)[M + b];
            const long double e = std::fabs(got - want);
            if (fn > 0.0L) worst_rt = std::max(worst_rt, e / fn);
            CHECK(e <= 1e-13L * fn);
          }
        }
      }
    }
  CHECK(next == (long long)q.size());
  CHECK(left_nonzero == 0);
  CHECK(want_doubles < 0 || (long long)q.size() == want_doubles);
  // N2 < M: (4, 4) has four rows per output, (1, 1) one (a cell ends where the next one starts)
  auto rows_of = [&](int N2, int Nu) {
    size_t c = (size_t)(N2 - 1) * numax + (Nu - 1);
    const long long begin = off[c];
    long long end = (long long)q.size();
    for (++c; c < off.size(); ++c)
      if (off[c] >= 0) {
        end = off[c];
        break;
      }
    return (int)((end - begin) / ((long long)my * (nu * Nu + nx)));
  };
  CHECK(rows_of(1, 1) == 1);
  CHECK(numax < 4 || rows_of(4, 4) == 4);
  // one double below the table's size as the cap: no table, no index
  std::vector<double> q2;
  std::vector<int> off2;
  qr_tables(s, q2, off2, (long long)q.size() * 8 - 1);
  CHECK(q2.empty() && off2.empty());
  qr_tables(s, q2, off2, (long long)q.size() * 8);
  CHECK(q2 == q && off2 == off);
  // packed beside the other tables for a small plant; not when switched off
  PackedTables pk = pack_tables(s);
  DevScenario ds = pk.rebased(pk.blob.data());
  CHECK(ds.small == 1 && ds.qrt && ds.qrt_off);
  CHECK(ds.qrt && std::memcmp(ds.qrt, q.data(), q.size() * 8) == 0);
  CHECK(ds.qrt_off && std::memcmp(ds.qrt_off, off.data(), off.size() * 4) == 0);
  mpct_scenario without = *s;
  without.qr_tables = 0;
  pk = pack_tables(&without);
  ds = pk.rebased(pk.blob.data());
  CHECK(ds.small == 1 && !ds.qrt && !ds.qrt_off && ds.step && ds.gram);
  std::printf("%s: qr_doubles=%zu cells=%lld short_cells=%lld zero_columns=%lld worst_rr=%.3Lg worst_rt=%.3Lg\n", name,
              q.size(), cells, short_cells, zero_cols, worst_rr, worst_rt);
}

int main() {
  {  // Shell 3x3, the metric's scenario: 3 outputs, 3 MVs, delays up to 7 samples (output 0's G is zero for N2 <= 7)
    Plant c(3, 3,
            {{0.02313052619372795, 0.06667958558934375}, {0.0, 0.013710194313372143},
             {0.02089018186516949, 0.06022122704814364}, {0.058828715846932514, 0.0565220089046257},
             {0.02173580108248058, 0.021023216763849436}, {0.0294987546979058, 0.08419778882992246},
             {0.0, 0.1963360266878832}, {0.032116113806741245, 0.03068897122230742}, {0.0, 0.3338832924071783}},
            {0.9231163463866358, 0.9355069850316178, 0.9231163463866358, 0.9231163463866358, 0.9355069850316178,
             0.9048374180359595, 0.8858460329277068, 0.9131007162822624, 0.8101577349324267},
            {7, 7, 7, 5, 4, 4, 5, 6, 0}, 30, 5);
    BuildError err;
    const std::unique_ptr<mpct_scenario> s = build_scenario(c.d, &err);
    CHECK(s != nullptr);
    if (s) {
      long long want = 0;
      for (int N2 = 1; N2 <= 30; ++N2)
        for (int Nu = 1; Nu <= std::min(N2, 5); ++Nu) want += 3ll * std::min(N2, 3 * Nu) * (3 * Nu + s->nx);
      check_scenario("shell3x3", s.get(), want);
      CHECK(want * 8 <= kQrtMaxBytes);
      // the same plant over the VNS search ranges is far above the cap: nothing is built or packed
      c.d.n2_max = 127;
      c.d.nu_max = 15;
      const std::unique_ptr<mpct_scenario> big = build_scenario(c.d, &err);
      CHECK(big != nullptr);
      if (big) {
        std::vector<double> q;
        std::vector<int> off;
        qr_tables(big.get(), q, off);
        CHECK(q.empty() && off.empty());
        const PackedTables pk = pack_tables(big.get());
        const DevScenario ds = pk.rebased(pk.blob.data());
        CHECK(!ds.qrt && !ds.qrt_off);
        std::printf("shell3x3 127x15: qr_doubles=%zu\n", q.size());
      }
    }
  }
  {  // synthetic 2x2 with dead time: entry (0, 1) waits 5 samples, so its columns of G_0 are zero for N2 <= 5
    Plant c(2, 2, {{0.0, 0.10}, {0.0, 0.05}, {0.0, 0.04}, {0.0, 0.12}}, {0.9, 0.7, 0.8, 0.6}, {0, 5, 2, 0}, 12, 4);
    BuildError err;
    const std::unique_ptr<mpct_scenario> s = build_scenario(c.d, &err);
    CHECK(s != nullptr);
    if (s) check_scenario("deadtime 2x2", s.get(), -1);
  }
  std::printf(g_bad ? "%d expectation(s) failed\n" : "ok\n", g_bad);
  return g_bad ? 1 : 0;
}
