// scenario_tables.h — host-only precompute of libmpct: descriptor validation, the candidate-
// independent GPC tables and their packing into the blob a device context uploads.  No HIP call is
// made here (hip_runtime.h is included for mpct_dev.h's types alone), so the whole file runs, and is
// sanitizer-checked, on a machine without a GPU (tests/host_tables).
//
// Host tables (restating the reference's setup functions, natively):
//   step[i][n][t]     step response of model entry (i,n), t = 0..tlen-1      (MatG.m:51 step)
//   F_i rows          Diophantine free-output polynomials for the window      (diophantine.m:35-65)
//   uG_in rows        past-control coefficients, ALL zeros removed, last cp    (deltaUFree.m:13-62)
//   phi[(i,r)][s]     = [F_i row r | uG_i* row r] laid out on the state vector
//                       x = [y_1(t..t-na_1) ... | du_1(t-1..t-duM_1) ...]     (cell2mat2.m,
//                       DTC_GPC_WW.m:139-146: yf = Hp*up + S*Yd)
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../../include/mpct.h"
#include "mpct_dev.h"

struct DevCtx;  // everything a scenario keeps on one device (mpct_host.cpp)

namespace mpct {
// entries of a transfer-function matrix in z^-1 form, the delay folded into b: entry e has nb[e]
// numerator taps b[e][0..nb) (the first nonzero one at off[e]) and na[e] denominator taps a[e][0..na)
struct ZTables {
  int maxb = 0, maxa = 0;  // row lengths of b and a
  std::vector<int> nb, na, off;
  std::vector<double> b, a;
};
}  // namespace mpct

struct mpct_scenario {
  int my = 0, nu = 0, nd = 0, nin = 0, nit = 0, n2max = 0, numax = 0, wsq = 1, ink0 = 9;
  std::vector<int> n1;
  int tlen = 0;
  std::vector<double> step;  // [my][nu][tlen]
  int nx = 0, nyh = 0, nup = 0;
  std::vector<int> yoff, nyhi, upoff, dum;
  std::vector<double> phi;   // [my*n2max][nx]  reference layout (S | Hp)
  std::vector<double> phid;  // same rows on the device state basis (see build_scenario)
  int ne = 0;
  int npin = 0;  // plant input columns: nu MVs, nd MDs, nq plant-only disturbances
  int nvar = 1;  // plant variants (Monte-Carlo draws); tables are [nvar][ne]
  mpct::ZTables pl;
  // DTC-GPC predictor (abi >= 2): Pz and Gz entries (2*my*nu, z^-1 form) and the filters Fr_i
  int dtc = 0, nq = 0;
  int fr_max = 1;
  mpct::ZTables mz{1, 1};  // rows of length 1 where there is no entry (DevScenario::mz_maxb / mz_maxa)
  std::vector<double> fr_b, fr_a;
  std::vector<int> fr_n;
  std::vector<double> bnd;   // [4][nu]
  std::vector<double> yref;  // [my][nit]
  // MD feed-forward + soft output bands (abi >= 3): model entries of all nin columns in the mz
  // tables, MD step responses, output bounds, weight scales
  int mdband = 0;
  // output-feedback estimator of the band kernel (mpct_scenario_create_est): 0 none (plant == model),
  // MPCT_EST_OUTPUT_BIAS the deadbeat output-disturbance observer
  int est = 0;
  double rho = 0.0;
  std::vector<double> step_md;  // [my][nd][tlen]
  std::vector<double> obnd;     // [4][my]
  std::vector<double> wscale;   // [my + nu]
  // nonlinear MPC (abi >= 4, build_nmpc_scenario): my = ny outputs, nu MVs
  int nmpc = 0, nsub = 10, sqp_max = 100;
  double ts = 0.0, sqp_tol = 1e-8;
  std::vector<int> xc;      // [ny] 0-based output states
  std::vector<double> nm;   // see DevScenario::nm
  std::vector<double> nmv;  // plant variants [nvar][NM_NPAR + 3] (DevScenario::nmv); empty: plant = model
  // 0: no pre-factored prologue rows are packed (qr_tables), the prologue streams [G | Phi] as it
  // does for a scenario over kQrtMaxBytes (mpct_scenario_create: environment MPCT_NO_QR_TABLES)
  int qr_tables = 1;
  // slots of an ordered metric launch that run on gpc_small_wide_kernel: -1 = the rule
  // (mpct_dev.h wide_slot_rule), n >= 0 from the environment (MPCT_WIDE_SLOTS=n; 0: one launch)
  long long wide_slots = -1;
  // device state, one context per device ordinal (created on first use, kept until destroy):
  // a scenario can be evaluated on several GPUs of one process (mpct_eval_batch_multi)
  std::vector<DevCtx*> ctx;
  // further contexts of a device listed more than once in one mpct_eval_batch_multi call:
  // extra[dev][j] serves its (j+2)-th occurrence (own stream, scratch and order buffers)
  std::vector<std::vector<DevCtx*>> extra;
};

namespace mpct {

// why a builder returned no scenario
struct BuildError {
  int code = MPCT_OK;
  std::string msg;
};
// what a failed check returns: no scenario (the builders) or false (nmpc_dims_ok)
struct Rejected {
  operator std::unique_ptr<mpct_scenario>() const { return nullptr; }
  operator bool() const { return false; }
};
inline Rejected reject(BuildError* err, int code, const char* msg) {
  err->code = code;
  err->msg = msg;
  return {};
}

inline bool valid_dtf(const mpct_dtf& m) { return m.len >= 1 && m.num && m.den && m.den[0] != 0.0 && m.delay >= 0; }

inline std::vector<double> conv(const std::vector<double>& a, const std::vector<double>& b) {
  if (a.empty() || b.empty()) return {};
  std::vector<double> c(a.size() + b.size() - 1, 0.0);
  for (size_t i = 0; i < a.size(); ++i)
    for (size_t j = 0; j < b.size(); ++j) c[i + j] += a[i] * b[j];
  return c;
}

// direct-form discrete filter of a unit step: z^-delay num(z)/den(z) (tfdata form)
inline void step_response(const mpct_dtf& d, int T, double* s) {
  const int len = d.len;
  std::vector<double> b(d.delay + len, 0.0), a(len);
  for (int k = 0; k < len; ++k) {
    b[d.delay + k] = d.num[k] / d.den[0];
    a[k] = d.den[k] / d.den[0];
  }
  std::vector<double> y(T, 0.0);
  for (int t = 0; t < T; ++t) {
    double acc = 0.0;
    for (int l = 0; l < (int)b.size(); ++l)
      if (t - l >= 0) acc += b[l];  // unit step input
    for (int l = 1; l < len; ++l)
      if (t - l >= 0) acc -= a[l] * y[t - l];
    y[t] = acc;
  }
  std::copy(y.begin(), y.end(), s);
}

// descompMPC.m:19-43 followed by the exact-LCM CARIMA form (BA_MIMO.m:20-71 with the row's
// DISTINCT denominator polynomials multiplied, instead of the rounded-roots LCM): what a host that
// passes na = carima_A = nb = carima_B = dp = NULL gets (abi >= 5; the MATLAB MEX host builds its
// descriptor from the mpc object's tfdata alone).  Same arithmetic as mpct/lti.py descomp + carima
// (exact=True), checked against it in tests/test_abi.py.
struct CarimaTables {
  std::vector<int32_t> na, nb, dp;
  std::vector<double> A, B;
};

inline void derive_carima(const mpct_dtf* model, int my, int nin, CarimaTables& c) {
  c.na.assign(my, 0);
  c.nb.assign((size_t)my * nin, 0);
  c.dp.assign((size_t)my * nin, 0);
  c.A.clear();
  c.B.clear();
  std::vector<std::vector<double>> Bs((size_t)my * nin);
  for (int i = 0; i < my; ++i) {
    int dmax = 0;
    for (int j = 0; j < nin; ++j) dmax = std::max(dmax, model[i * nin + j].delay);
    for (int j = 0; j < nin; ++j) {
      const mpct_dtf& m = model[i * nin + j];
      std::vector<double> b(m.num, m.num + m.len);
      int dd = m.delay;
      if (b[0] != 0.0) {  // descompMPC.m:35-38: d = d - 1, B = [0 B]
        dd -= 1;
        b.insert(b.begin(), 0.0);
      }
      double sn = 0.0, sd = 0.0;
      for (int k = 0; k < m.len; ++k) {
        sn += m.num[k];
        sd += m.den[k];
      }
      if (sd != 0.0 && sn / sd == 0.0) dd = dmax;  // descompMPC.m:39-41: zero dcgain
      c.dp[i * nin + j] = dd;
      if (b[0] == 0.0) b.erase(b.begin());  // BA_MIMO.m:22-24: one leading zero stripped
      Bs[i * nin + j] = b;
    }
  }
  for (int i = 0; i < my; ++i) {
    std::vector<std::vector<double>> uniq;
    auto den = [&](int j) { return std::vector<double>(model[i * nin + j].den, model[i * nin + j].den + model[i * nin + j].len); };
    for (int j = 0; j < nin; ++j) {
      const std::vector<double> a = den(j);
      if (std::find(uniq.begin(), uniq.end(), a) == uniq.end()) uniq.push_back(a);
    }
    std::vector<double> Ai{1.0};
    for (const auto& u : uniq) Ai = conv(Ai, u);
    c.na[i] = (int)Ai.size() - 1;
    for (double x : Ai) c.A.push_back(x / Ai[0]);
    for (int j = 0; j < nin; ++j) {
      std::vector<double> b = Bs[i * nin + j];
      const std::vector<double> a = den(j);
      for (const auto& u : uniq)
        if (u != a) b = conv(b, u);
      c.nb[i * nin + j] = (int)b.size() - 1;
      for (double x : b) c.B.push_back(x / Ai[0]);
    }
  }
}

// the z^-1 tables of a list of valid entries, each with its effective delay (>= 0) folded into b and
// normalised by den[0]; false (the tables then hold lengths only) when an entry is longer than the
// device history rings
struct ZEntry {
  const mpct_dtf* tf;
  int delay;
};
inline bool z_tables(const std::vector<ZEntry>& entries, ZTables& t) {
  const size_t n = entries.size();
  t.nb.resize(n);
  t.na.resize(n);
  for (size_t e = 0; e < n; ++e) {
    t.nb[e] = entries[e].delay + entries[e].tf->len;
    t.na[e] = entries[e].tf->len;
    t.maxb = std::max(t.maxb, t.nb[e]);
    t.maxa = std::max(t.maxa, t.na[e]);
  }
  if (t.maxb > kMaxTaps || t.maxa > kYeHist) return false;
  t.b.assign(n * t.maxb, 0.0);
  t.a.assign(n * t.maxa, 0.0);
  t.off.assign(n, 0);
  for (size_t e = 0; e < n; ++e) {
    const mpct_dtf& m = *entries[e].tf;
    for (int k = 0; k < m.len; ++k) {
      t.b[e * t.maxb + entries[e].delay + k] = m.num[k] / m.den[0];
      t.a[e * t.maxa + k] = m.den[k] / m.den[0];
    }
    int o = 0;
    while (o < t.nb[e] && t.b[e * t.maxb + o] == 0.0) ++o;
    t.off[e] = o;
  }
  return true;
}

// validate a linear scenario descriptor and precompute its tables (no device needed).  estimator:
// 0 (mpct_scenario_create) or MPCT_EST_OUTPUT_BIAS on a band descriptor (mpct_scenario_create_est;
// both checked first, here: the plant, and every plant variant, may then differ from the model)
inline std::unique_ptr<mpct_scenario> build_scenario(const mpct_scenario_desc& d_in, BuildError* err,
                                                     int estimator = 0) {
  if (estimator != 0 && estimator != MPCT_EST_OUTPUT_BIAS) return reject(err, MPCT_EINVAL, "unknown estimator id");
  if (estimator && !(d_in.abi_version >= 3 && d_in.mdband))
    return reject(err, MPCT_EINVAL, "the output-bias estimator belongs to the band kernel (mdband = 1)");
  mpct_scenario_desc dcopy = d_in;
  const mpct_scenario_desc* d = &dcopy;
  CarimaTables derived;
  if (d_in.abi_version >= 5 && !(d_in.mdband) && d_in.dtc == 0 && !d_in.na && !d_in.carima_A && !d_in.nb &&
      !d_in.carima_B && !d_in.dp && d_in.model && d_in.my >= 1 && d_in.nu >= 1 && d_in.nd >= 0 &&
      d_in.my <= kMaxOut && d_in.nu + d_in.nd <= kMaxIn) {
    const int nin = d_in.nu + d_in.nd;
    for (int e = 0; e < d_in.my * nin; ++e)
      if (!valid_dtf(d_in.model[e])) return reject(err, MPCT_EINVAL, "bad model entry");
    derive_carima(d_in.model, d_in.my, nin, derived);
    dcopy.na = derived.na.data();
    dcopy.nb = derived.nb.data();
    dcopy.dp = derived.dp.data();
    dcopy.carima_A = derived.A.data();
    dcopy.carima_B = derived.B.data();
  }
  if (d->abi_version < 1 || d->abi_version > MPCT_ABI_VERSION) return reject(err, MPCT_EINVAL, "abi_version mismatch");
  const int dtc = d->abi_version >= 2 ? (d->dtc ? 1 : 0) : 0;
  const int nq = d->abi_version >= 2 ? d->nq : 0;
  const int nplant = (d->abi_version >= 2 && d->nplant > 1) ? d->nplant : 1;
  const int mdband = d->abi_version >= 3 ? (d->mdband ? 1 : 0) : 0;
  if (mdband && (dtc || nq > 0 || (nplant > 1 && !estimator)))
    return reject(err, MPCT_EINVAL, "mdband excludes dtc, plant-only disturbances and plant variants");
  if (mdband && (!d->y_min || !d->y_max || !d->ecr_min || !d->ecr_max))
    return reject(err, MPCT_EINVAL, "mdband needs y_min, y_max, ecr_min, ecr_max");
  if (nplant > 1 && !d->plant_var) return reject(err, MPCT_EINVAL, "nplant > 1 needs plant_var");
  if (nq < 0 || (nq > 0 && !d->dist)) return reject(err, MPCT_EINVAL, "nq > 0 needs dist");
  if (d->my < 1 || d->nu < 1 || d->nd < 0 || d->nit < 1 || d->n2_max < 1 || d->nu_max < 1)
    return reject(err, MPCT_EINVAL, "non-positive dimension");
  if (d->my > kMaxOut || d->nu + d->nd > kMaxIn) return reject(err, MPCT_ERANGE, "too many outputs/inputs");
  if (d->nd > 0 && !mdband)
    return reject(err, MPCT_ERANGE, "measured disturbances (nd > 0) need the mdband kernel (mdband = 1)");
  if (d->nu * d->nu_max + mdband > 64)
    return reject(err, MPCT_ERANGE, "nu*nu_max (+1 eps row) > 64 (one wavefront of QP rows)");
  if (!d->n1 || !d->plant || !d->model || !d->du_min || !d->du_max || !d->u_min || !d->u_max || !d->yref)
    return reject(err, MPCT_EINVAL, "null table pointer");
  if (!mdband && (!d->na || !d->carima_A || !d->nb || !d->carima_B || !d->dp))
    return reject(err, MPCT_EINVAL, "null CARIMA table pointer");
  auto s = std::make_unique<mpct_scenario>();
  s->my = d->my;
  s->nu = d->nu;
  s->nd = d->nd;
  s->nin = d->nu + d->nd;
  s->dtc = dtc;
  s->nq = nq;
  s->npin = s->nin + nq;
  s->nvar = nplant;
  s->mdband = mdband;
  s->est = mdband ? estimator : 0;
  if (s->npin > kMaxIn) return reject(err, MPCT_ERANGE, "too many plant inputs");
  s->nit = d->nit;
  s->n2max = d->n2_max;
  s->numax = d->nu_max;
  s->wsq = d->weights_squared ? 1 : 0;
  s->ink0 = d->vns_ink - 1;
  const int my = s->my, nu = s->nu, nin = s->nin, N = s->n2max;
  s->n1.assign(d->n1, d->n1 + my);
  int n1max = 0;
  for (int i = 0; i < my; ++i) {
    if (s->n1[i] < 1) return reject(err, MPCT_EINVAL, "n1[i] must be >= 1");
    n1max = std::max(n1max, s->n1[i]);
  }
  // ---- step table (MatG.m:51): enough samples for s(n1 + r - c), r < n2max
  s->tlen = n1max + N;
  s->step.assign((size_t)my * nu * s->tlen, 0.0);
  for (int i = 0; i < my; ++i)
    for (int n = 0; n < nu; ++n) {
      const mpct_dtf& m = d->model[i * nin + n];
      if (!valid_dtf(m)) return reject(err, MPCT_EINVAL, "bad model entry");
      step_response(m, s->tlen, &s->step[((size_t)i * nu + n) * s->tlen]);
    }
  if (mdband) {
    for (int i = 0; i < my; ++i)
      if (s->n1[i] != 1)
        return reject(err, MPCT_EINVAL, "mdband predicts over the toolbox window: n1[i] must be 1");
  } else {
  // ---- CARIMA offsets
  std::vector<int> aoff(my + 1, 0), boff(my * nin + 1, 0);
  for (int i = 0; i < my; ++i) {
    if (d->na[i] < 0) return reject(err, MPCT_EINVAL, "na < 0");
    aoff[i + 1] = aoff[i] + d->na[i] + 1;
  }
  for (int e = 0; e < my * nin; ++e) {
    if (d->nb[e] < 0 || d->dp[e] < 0) return reject(err, MPCT_EINVAL, "nb/dp < 0");
    boff[e + 1] = boff[e] + d->nb[e] + 1;
  }
  // ---- state layout
  s->yoff.resize(my);
  s->nyhi.resize(my);
  int o = 0;
  for (int i = 0; i < my; ++i) {
    s->yoff[i] = o;
    s->nyhi[i] = d->na[i] + 1;
    o += d->na[i] + 1;
  }
  s->nyh = o;
  // cp(i,n) = dp + length(B) - 1  (deltaUFree.m:25-29)
  std::vector<int> cp(my * nu);
  s->dum.assign(nu, 0);
  for (int i = 0; i < my; ++i)
    for (int n = 0; n < nu; ++n) {
      int c = d->dp[i * nin + n] + (d->nb[i * nin + n] + 1) - 1;
      if (c < 1) c = 1;
      cp[i * nu + n] = c;
      s->dum[n] = std::max(s->dum[n], c);
    }
  s->upoff.resize(nu);
  for (int n = 0; n < nu; ++n) {
    s->upoff[n] = o;
    o += s->dum[n];
  }
  s->nx = o;
  s->nup = o - s->nyh;
  if (s->nx + my > 256) return reject(err, MPCT_ERANGE, "free-response state too large");
  if (nu * s->numax > kWave - 1) return reject(err, MPCT_ERANGE, "nu*nu_max must be < 64 (one QP row per lane)");
  // ---- Diophantine + deltaUFree per output (window rows j = n1_i .. n1_i + N - 1)
  s->phi.assign((size_t)my * N * s->nx, 0.0);
  for (int i = 0; i < my; ++i) {
    const int na = d->na[i];
    const double* A = d->carima_A + aoff[i];
    if (A[0] != 1.0) return reject(err, MPCT_EINVAL, "carima_A[i][0] must be 1");
    // diophantine(A, N, d): N1 = d+1; DTC-GPC predicts from the delay-free yp (d = 0,
    // DTC_GPC_WW.m:80) while MatG keeps the dmin+1 window
    const int dd = s->dtc ? 0 : s->n1[i] - 1;
    std::vector<double> Ai(A, A + na + 1);
    std::vector<double> AD = conv(Ai, {1.0, -1.0});  // A~ = A*Delta (diophantine.m:35)
    const int nAD = (int)AD.size();                 // na + 2
    const int rows = dd + N + 1;
    std::vector<double> f((size_t)rows * (nAD - 1), 0.0);
    auto F = [&](int j, int k) -> double& { return f[(size_t)j * (nAD - 1) + k]; };
    F(0, 0) = 1.0;
    for (int j = 0; j < dd + N; ++j) {  // diophantine.m:55-63
      for (int k = 0; k < nAD - 2; ++k) F(j + 1, k) = F(j, k + 1) - F(j, 0) * AD[k + 1];
      F(j + 1, nAD - 2) = -F(j, 0) * AD[nAD - 1];
    }
    for (int r = 0; r < N; ++r) {
      const int j = dd + 1 + r;  // prediction step of this row (1-based)
      double* prow = &s->phi[((size_t)i * N + r) * s->nx];
      for (int k = 0; k <= na; ++k) prow[s->yoff[i] + k] = F(j, k);
      // E_j = [1, f(1,0), ..., f(j-1,0)]  (diophantine.m:69-77)
      std::vector<double> E(j);
      E[0] = 1.0;
      for (int k = 1; k < j; ++k) E[k] = F(k, 0);
      for (int n = 0; n < nu; ++n) {
        const int e = i * nin + n;
        std::vector<double> B(d->carima_B + boff[e], d->carima_B + boff[e + 1]);
        std::vector<double> aux = conv(E, B);
        std::vector<double> BE;
        for (double v : aux)
          if (v != 0.0) BE.push_back(v);  // deltaUFree.m:40-45: every zero removed
        const int c = cp[i * nu + n];
        const int lBE = (int)BE.size();
        double* dst = prow + s->upoff[n];  // left-aligned block (cell2mat2.m:56)
        if (lBE < c) {
          for (int k = 0; k < c - lBE; ++k) dst[k] = 0.0;
          for (int k = 0; k < lBE; ++k) dst[c - lBE + k] = BE[k];
        } else {
          for (int k = 0; k < c; ++k) dst[k] = BE[lBE - c + k];
        }
      }
    }
  }
  // ---- device copy of phi in a well-conditioned basis.  The F rows have
  // large alternating coefficients (|F| ~ 3e3 for Shell 3x3) that cancel on the slowly varying
  // y history; folded into the gain matrix they amplify rounding ~1e4x.  Rewrite the y part on
  // backward differences, y(t-l) = sum_k (-1)^k C(l,k) nabla^k y(t), and use the identity
  // F_j(1) = 1 (Atilde(1) = 0 in 1 = E_j Atilde + z^-j F_j) to make the nabla^0 column exactly
  // 1: the device state is [y_i(t) - r_i(t), nabla y_i(t), ..., nabla^na y_i(t) | du history].
  s->phid = s->phi;
  for (int i = 0; i < my; ++i) {
    const int n = d->na[i] + 1;
    std::vector<double> binom((size_t)n * n, 0.0);
    for (int l = 0; l < n; ++l) {
      binom[(size_t)l * n] = 1.0;
      for (int k = 1; k <= l; ++k) binom[(size_t)l * n + k] = binom[(size_t)(l - 1) * n + k - 1] +
                                                           (k <= l - 1 ? binom[(size_t)(l - 1) * n + k] : 0.0);
    }
    for (int r = 0; r < N; ++r) {
      const double* src = &s->phi[((size_t)i * N + r) * s->nx + s->yoff[i]];
      double* dst = &s->phid[((size_t)i * N + r) * s->nx + s->yoff[i]];
      for (int k = 0; k < n; ++k) {
        double a = 0.0;
        for (int l = k; l < n; ++l) a += src[l] * ((k & 1) ? -binom[(size_t)l * n + k] : binom[(size_t)l * n + k]);
        dst[k] = a;
      }
      dst[0] = 1.0;
    }
  }
  }  // !mdband
  // ---- plant entries in z^-1 form (delay folded into b); plant-only disturbance paths appended
  // as columns nin..npin-1 of each output row; entries over all variants: ev = variant*ne + e
  const int npin = s->npin;
  s->ne = my * npin;
  std::vector<ZEntry> entries;
  for (int ev = 0; ev < s->nvar * s->ne; ++ev) {
    const int v = ev / s->ne, e = ev % s->ne, i = e / npin, j = e % npin;
    const mpct_dtf& p = j >= nin        ? d->dist[i * nq + (j - nin)]
                        : s->nvar > 1 ? d->plant_var[(size_t)v * my * nin + i * nin + j]
                                      : d->plant[i * nin + j];
    if (!valid_dtf(p)) return reject(err, MPCT_EINVAL, "bad plant entry");
    if (j < nu && p.delay == 0 && p.num[0] != 0.0)
      return reject(err, MPCT_EINVAL, "plant has direct feedthrough from an MV (algebraic loop)");
    entries.push_back({&p, p.delay});
  }
  for (int n = 0; n < (mdband ? 0 : nu); ++n)
    if (s->dum[n] > kMaxDum)
      return reject(err, MPCT_ERANGE, "past-control register longer than the device supports (16)");
  for (int i = 0; i < (mdband ? 0 : my); ++i)
    if (s->nyhi[i] > kYeHist)
      return reject(err, MPCT_ERANGE, "CARIMA denominator order too high for the device (na <= 7)");
  // the model of every column (MV and MD) of a band scenario, z^-1 form with its delay: the window
  // extension and, with the estimator, the parallel model (mdband_kernel.hip)
  std::vector<ZEntry> mentries;
  for (int e = 0; e < (mdband ? my * nin : 0); ++e) {
    if (!valid_dtf(d->model[e])) return reject(err, MPCT_EINVAL, "bad model entry");
    mentries.push_back({&d->model[e], d->model[e].delay});
  }
  // the parallel model runs through the plant copies' rings and row strides: with the estimator the
  // plant tables' row lengths are the maxima over every variant and the model, and the one length
  // check below covers the model too
  for (const ZEntry& m : mentries) {
    if (!s->est) break;
    s->pl.maxb = std::max(s->pl.maxb, m.delay + m.tf->len);
    s->pl.maxa = std::max(s->pl.maxa, m.tf->len);
  }
  if (!z_tables(entries, s->pl)) return reject(err, MPCT_ERANGE, "plant entry too long for the device history rings");
  if (s->dtc) {
    // Pz entries (e < my*nu, real delays) and Gz entries (delays minus dmin_i = n1_i - 1,
    // DTC_GPC_WW.m:40-46) in z^-1 form; filters Fr_i (mimofilter.m) with delay 0
    entries.clear();
    for (int e = 0; e < 2 * my * nu; ++e) {
      const int k = e % (my * nu), i = k / nu, j = k % nu;
      const mpct_dtf& m = d->model[i * nin + j];
      const int del = e < my * nu ? m.delay : m.delay - (s->n1[i] - 1);
      if (del < 0) return reject(err, MPCT_EINVAL, "DTC: model delay below dmin (n1 - 1)");
      entries.push_back({&m, del});
    }
    if (!z_tables(entries, s->mz))
      return reject(err, MPCT_ERANGE, "DTC: model entry too long for the device history rings");
    s->fr_n.assign(my, 1);
    for (int i = 0; i < my; ++i)
      if (d->filter) s->fr_n[i] = d->filter[i].len;
    for (int i = 0; i < my; ++i) s->fr_max = std::max(s->fr_max, s->fr_n[i]);
    if (s->fr_max > kYeHist) return reject(err, MPCT_ERANGE, "DTC: filter order too high (len <= 8)");
    s->fr_b.assign((size_t)my * s->fr_max, 0.0);
    s->fr_a.assign((size_t)my * s->fr_max, 0.0);
    for (int i = 0; i < my; ++i) {
      if (!d->filter) {
        s->fr_b[(size_t)i * s->fr_max] = 1.0;
        s->fr_a[(size_t)i * s->fr_max] = 1.0;
        continue;
      }
      const mpct_dtf& f = d->filter[i];
      if (!valid_dtf(f) || f.delay != 0) return reject(err, MPCT_EINVAL, "DTC: bad filter entry (delay must be 0)");
      for (int q2 = 0; q2 < f.len; ++q2) {
        s->fr_b[(size_t)i * s->fr_max + q2] = f.num[q2] / f.den[0];
        s->fr_a[(size_t)i * s->fr_max + q2] = f.den[q2] / f.den[0];
      }
    }
  }
  if (mdband) {
    // without an estimator plant == model (closedloop_toolbox.m:50 sims the controller's model)
    for (int e = 0; e < (s->est ? 0 : my * nin); ++e) {
      const mpct_dtf& m = d->model[e];
      const mpct_dtf& p = d->plant[e];
      bool same = p.len == m.len && p.delay == m.delay;
      for (int k = 0; same && k < m.len; ++k) same = p.num[k] == m.num[k] && p.den[k] == m.den[k];
      if (!same)
        return reject(err, MPCT_ERANGE, "mdband: plant must equal the model (the toolbox estimator is not restated)");
    }
    z_tables(mentries, s->mz);  // they fit the history rings: no longer than the plant tables' rows, which did
    const int nd = s->nd;
    s->step_md.assign((size_t)my * std::max(nd, 1) * s->tlen, 0.0);
    for (int i = 0; i < my; ++i)
      for (int j = 0; j < nd; ++j)
        step_response(d->model[i * nin + nu + j], s->tlen, &s->step_md[((size_t)i * nd + j) * s->tlen]);
    s->obnd.assign(4 * my, 0.0);
    s->wscale.assign(my + nu, 1.0);
    for (int i = 0; i < my; ++i) {
      const double sy = d->y_scale ? d->y_scale[i] : 1.0;
      if (!(sy > 0.0) || !(d->ecr_min[i] >= 0.0) || !(d->ecr_max[i] >= 0.0) || !(d->y_min[i] <= d->y_max[i]))
        return reject(err, MPCT_EINVAL, "mdband: bad output bound / ECR / scale factor");
      s->obnd[i] = d->y_min[i];
      s->obnd[my + i] = d->y_max[i];
      s->obnd[2 * my + i] = d->ecr_min[i] * sy;
      s->obnd[3 * my + i] = d->ecr_max[i] * sy;
      s->wscale[i] = 1.0 / sy;
    }
    for (int n = 0; n < nu; ++n) {
      const double su = d->u_scale ? d->u_scale[n] : 1.0;
      if (!(su > 0.0)) return reject(err, MPCT_EINVAL, "mdband: bad MV scale factor");
      s->wscale[my + n] = 1.0 / su;
    }
    s->rho = d->rho_ecr;
    if (!(s->rho > 0.0)) return reject(err, MPCT_EINVAL, "mdband: rho_ecr must be > 0");
  }
  s->bnd.resize(4 * nu);
  for (int n = 0; n < nu; ++n) {
    s->bnd[n] = d->du_min[n];
    s->bnd[nu + n] = d->du_max[n];
    s->bnd[2 * nu + n] = d->u_min[n];
    s->bnd[3 * nu + n] = d->u_max[n];
    if (!(s->bnd[n] <= 0.0 && s->bnd[nu + n] >= 0.0 && s->bnd[2 * nu + n] <= 0.0 && s->bnd[3 * nu + n] >= 0.0))
      return reject(err, MPCT_EINVAL, "bounds must contain 0 (nominal u = 0 must be feasible)");
  }
  s->yref.assign(d->yref, d->yref + (size_t)my * s->nit);
  return s;
}

// ------------------------------------------------------------------------------------------
// nonlinear MPC scenario (closedloop_toolbox_nmpc.m; VanDeVusse_NMPC.m)
constexpr double kVdvParams[NM_NPAR] = {  // nmpc_vandevusse_state.m:43-58
    1.287e12, 1.287e12, 9.043e9, -9758.3, -9758.3, -8560.0, -4.20, 11.00, 41.85,
    0.9342,   3.01,     4032.0,  0.215,   10.0,    130.00,  5.10};

// the checks that come before the LDS-size check of the caller (mpct_nmpc_scenario_create: it needs
// nmpc_kernel.hip's layout); build_nmpc_scenario repeats them, so a caller may run them first, then
// its own check, then the builder, and a descriptor with several faults reports them in that order
inline bool nmpc_dims_ok(const mpct_nmpc_desc& d, BuildError* err) {
  if (d.abi_version < 4 || d.abi_version > MPCT_ABI_VERSION) return reject(err, MPCT_EINVAL, "abi_version mismatch");
  if (d.model != MPCT_NMPC_VANDEVUSSE) return reject(err, MPCT_EINVAL, "unknown NMPC model id");
  if (d.nx != 3 || d.nu != 2) return reject(err, MPCT_EINVAL, "the Van de Vusse model has nx = 3, nu = 2");
  if (d.ny < 1 || d.ny > 2) return reject(err, MPCT_ERANGE, "ny must be 1 or 2");
  if (d.nit < 1 || d.n_max < 1 || d.nu_max < 1) return reject(err, MPCT_EINVAL, "non-positive dimension");
  if (d.nu * d.nu_max > 32) return reject(err, MPCT_ERANGE, "nu*nu_max > 32");
  return true;
}

// nplant plant variants (mpct_nmpc_scenario_create_var, which validates them: finite values,
// rho*cp*V != 0, no table with nplant = 0): plant_params [nplant][NM_NPAR] in the params order,
// plant_x0 [nplant][nx] or NULL (every variant starts at d.x0).  nplant = 0: the plant is the model
inline std::unique_ptr<mpct_scenario> build_nmpc_scenario(const mpct_nmpc_desc& d, BuildError* err, int nplant = 0,
                                                          const double* plant_params = nullptr,
                                                          const double* plant_x0 = nullptr) {
  if (!nmpc_dims_ok(d, err)) return nullptr;
  if (!(d.ts > 0.0) || d.nsub < 1) return reject(err, MPCT_EINVAL, "ts must be > 0 and nsub >= 1");
  if (!d.xc || !d.x0 || !d.u0 || !d.u_min || !d.u_max || !d.x_min || !d.x_max || !d.y_scale || !d.u_scale || !d.yref)
    return reject(err, MPCT_EINVAL, "null table pointer");
  for (int j = 0; j < d.ny; ++j)
    if (d.xc[j] < 1 || d.xc[j] > d.nx) return reject(err, MPCT_EINVAL, "xc out of range (1-based state index)");
  for (int n = 0; n < d.nu; ++n) {
    if (!(d.u_min[n] < d.u_max[n])) return reject(err, MPCT_EINVAL, "u_min must be < u_max");
    if (!(d.u_scale[n] > 0.0)) return reject(err, MPCT_EINVAL, "u_scale must be > 0");
  }
  for (int j = 0; j < d.ny; ++j)
    if (!(d.y_scale[j] > 0.0)) return reject(err, MPCT_EINVAL, "y_scale must be > 0");
  auto s = std::make_unique<mpct_scenario>();
  s->nmpc = 1;
  s->my = d.ny;
  s->nu = d.nu;
  s->nd = 0;
  s->npin = d.nu;
  s->nit = d.nit;
  s->n2max = d.n_max;
  s->numax = d.nu_max;
  s->ink0 = d.vns_ink > 0 ? d.vns_ink - 1 : 9;
  s->nsub = d.nsub;
  s->ts = d.ts;
  s->sqp_max = d.sqp_max > 0 ? d.sqp_max : 100;
  s->sqp_tol = d.sqp_tol > 0.0 ? d.sqp_tol : 1e-8;
  for (int j = 0; j < d.ny; ++j) s->xc.push_back(d.xc[j] - 1);
  const double* p = d.params ? d.params : kVdvParams;
  s->nm.assign(p, p + NM_NPAR);
  auto app_to = [](std::vector<double>& t, const double* a, int n) { t.insert(t.end(), a, a + n); };
  auto app = [&](const double* a, int n) { app_to(s->nm, a, n); };
  app(d.x0, 3);
  app(d.u0, d.nu);
  app(d.u_min, d.nu);
  app(d.u_max, d.nu);
  app(d.x_min, 3);
  app(d.x_max, 3);
  app(d.y_scale, d.ny);
  app(d.u_scale, d.nu);
  s->yref.assign(d.yref, d.yref + (size_t)d.ny * d.nit);
  if (nplant > 0 && plant_params) {
    s->nvar = nplant;
    for (int k = 0; k < nplant; ++k) {
      app_to(s->nmv, plant_params + (size_t)k * NM_NPAR, NM_NPAR);
      app_to(s->nmv, plant_x0 ? plant_x0 + (size_t)k * d.nx : d.x0, 3);
    }
  }
  return s;
}

// ------------------------------------------------------------------------------------------
// every per-lane history / coefficient set fits gpc_kernel.hip's register caps (kReg*)
inline int regpath(const mpct_scenario* s) {
  bool rp = !s->mdband && !s->nmpc && s->pl.maxa - 1 <= kRegA;  // gpc_kernel.hip only
  for (int e = 0; e < s->nvar * s->ne; ++e) rp = rp && (s->pl.nb[e] - s->pl.off[e] <= kRegB);
  for (int n = 0; rp && n < s->nu; ++n) rp = rp && (s->dum[n] <= kRegDu);
  for (int i = 0; rp && i < s->my; ++i) rp = rp && (s->nyhi[i] <= kRegY);
  return rp ? 1 : 0;
}

// lane tables of gpc_small_kernel and dtc_small_kernel: the plant / model term of lane 16 k + ep
// (coefficient, history ring offset in the kernel's history region, delay, ring mask), the state
// column -> A column map, and dtc_small_kernel's filters
struct SmallTables {
  int ke = 2;  // entry output ring: a power of two above the denominator taps
  std::vector<double> coef;
  std::vector<int> hoff, hc, hmask, acol;
  std::vector<double> fr;
  void init(size_t lanes, int na_max) {
    ke = na_max < 2 ? 2 : 4;
    coef.assign(lanes, 0.0);
    hoff.assign(lanes, 0);
    hc.assign(lanes, 0);
    hmask.assign(lanes, kSmU - 1);
  }
  // lane Li holds term k of entry e of z, which reads input ring j and entry output ring ep (the
  // entry rings start at eoff): b taps from the first nonzero one, then the a taps, then nothing
  void tap(size_t Li, int k, const ZTables& z, size_t e, int j, int ep, int eoff) {
    const int off = z.off[e], nbz = z.nb[e] - off, na1 = z.na[e] - 1;
    if (k < nbz) {  // b tap: u_j(t - off - k)
      coef[Li] = z.b[e * z.maxb + off + k];
      hoff[Li] = j * kSmU;
      hc[Li] = off + k;
    } else if (k < nbz + na1) {  // a tap jj: -a_jj y_e(t - jj)
      const int jj = k - nbz + 1;
      coef[Li] = -z.a[e * z.maxa + jj];
      hoff[Li] = eoff + ep * ke;
      hc[Li] = jj;
      hmask[Li] = ke - 1;
    }
  }
  // A's columns: y part in state order, then MV n's past-control register (age k) at
  // kSmY + kSmR n + k
  void map_columns(const mpct_scenario* s) {
    acol.assign(s->nx, 0);
    for (int c = 0; c < s->nyh; ++c) acol[c] = c;
    for (int n = 0; n < s->nu; ++n)
      for (int k = 0; k < s->dum[n]; ++k) acol[s->upoff[n] + k] = kSmY + kSmR * n + k;
  }
};

// gpc_small_kernel's lane tables (gpc_small.hip; lane L = 16 k + 4 i + j), or false when the scenario
// is not a small plant: my <= 4 outputs, nu <= 3 MVs, no MD / plant-only inputs, GPC mode, y difference
// state <= kSmY entries (<= 4 per output), past-control registers <= kSmR, and every entry of every
// plant variant <= 4 plant terms with rings the kernel holds (one variant outside the limits and the
// whole scenario is not small).  Tables: coef / hoff / hc / hmask [nvar][64], variant v's lane L at
// v * 64 + L (dtc_small_plant's convention); ke, and with it the LDS layout, is one per scenario: the
// maximum over the variants
inline bool small_plant(const mpct_scenario* s, SmallTables* tb) {
  if (s->mdband || s->nmpc || s->dtc || s->nd || s->nq || s->nvar < 1) return false;
  if (s->my > 4 || s->nu > 3 || s->npin != s->nu || s->nyh > kSmY) return false;
  for (int i = 0; i < s->my; ++i)
    if (s->nyhi[i] > 4) return false;
  for (int n = 0; n < s->nu; ++n)
    if (s->dum[n] > kSmR) return false;
  int na_max = 0;
  for (int e = 0; e < s->nvar * s->ne; ++e) {
    const int nbz = s->pl.nb[e] - s->pl.off[e], na1 = s->pl.na[e] - 1;
    if (nbz + na1 > 4 || na1 >= kSmE || s->pl.nb[e] > kSmU) return false;
    na_max = std::max(na_max, na1);
  }
  tb->init((size_t)s->nvar * kWave, na_max);
  for (int v = 0; v < s->nvar; ++v)
    for (int L = 0; L < kWave; ++L) {
      const int k = L >> 4, ep = L & 15, i = ep >> 2, j = ep & 3;
      if (i < s->my && j < s->nu)
        tb->tap((size_t)v * kWave + L, k, s->pl, (size_t)v * s->ne + i * s->npin + j, j, ep, kSmEOff);
    }
  tb->map_columns(s);
  return true;
}

// dtc_small_kernel's lane tables (dtc_small.hip), or false when the scenario is not a DTC-GPC small
// plant: DTC mode with every move bound infinite (DTC_GPC_WW.m's unconstrained loop: no QP), my <= 2,
// nu <= 2, nu + nq <= 4 ring-fed inputs (no MDs), every entry of every plant variant, of Pz and of Gz
// <= 4 terms with rings the kernel holds, filters of <= 4 taps, y difference state <= 4 per output,
// past-control registers <= kSmR.  Tables: coef / hoff / hc / hmask [nvar][64] (lane L = 16 k + 4 q
// + p: quads q < my the plant entries (i = q, input p), quads 2 + i: p < 2 Pz(i, p), p >= 2
// Gz(i, p - 2)), the acol map as for gpc_small, filters fr [my][8] = fb 0..3 | fa 0..3
inline bool dtc_small_plant(const mpct_scenario* s, SmallTables* tb) {
  if (!s->dtc || s->mdband || s->nmpc || s->nd || s->my > 2 || s->nu > 2 || s->npin > 4) return false;
  for (int n = 0; n < s->nu; ++n)
    if (!(std::isinf(s->bnd[n]) && std::isinf(s->bnd[s->nu + n]) && std::isinf(s->bnd[2 * s->nu + n]) &&
          std::isinf(s->bnd[3 * s->nu + n])))
      return false;
  if (s->nyh > kSmY) return false;
  for (int i = 0; i < s->my; ++i)
    if (s->nyhi[i] > 4 || s->fr_n[i] > 4) return false;
  for (int n = 0; n < s->nu; ++n)
    if (s->dum[n] > kSmR) return false;
  int na_max = 0;
  for (const ZTables* z : {&s->pl, &s->mz})
    for (size_t e = 0; e < z->nb.size(); ++e) {
      na_max = std::max(na_max, z->na[e] - 1);
      if ((z->nb[e] - z->off[e]) + (z->na[e] - 1) > 4 || z->na[e] - 1 >= kSmE || z->nb[e] > kSmU) return false;
    }
  tb->init((size_t)s->nvar * kWave, na_max);
  for (int v = 0; v < s->nvar; ++v)
    for (int L = 0; L < kWave; ++L) {
      const int k = L >> 4, ep = L & 15, q = ep >> 2, pp = ep & 3;
      const size_t Li = (size_t)v * kWave + L;
      if (q < 2) {  // plant entry (q, pp) of variant v
        if (q < s->my && pp < s->npin) tb->tap(Li, k, s->pl, (size_t)v * s->ne + q * s->npin + pp, pp, ep, kDtcEOff);
      } else {  // Pz (pp < 2) / Gz (pp >= 2) entry (q - 2, pp & 1): the controller's own inputs
        const int i = q - 2, j = pp & 1;
        if (i < s->my && j < s->nu)
          tb->tap(Li, k, s->mz, (pp >= 2 ? s->my * s->nu : 0) + i * s->nu + j, j, ep, kDtcEOff);
      }
    }
  tb->map_columns(s);
  tb->fr.assign((size_t)s->my * 8, 0.0);
  for (int i = 0; i < s->my; ++i)
    for (int l = 0; l < s->fr_n[i]; ++l) {
      tb->fr[(size_t)i * 8 + l] = s->fr_b[(size_t)i * s->fr_max + l];
      tb->fr[(size_t)i * 8 + 4 + l] = s->fr_a[(size_t)i * s->fr_max + l];
    }
  return true;
}

// the dispatch key's Gram tables (DevScenario::gram): for every horizon pair (N2, Nu) with
// nu Nu <= kGramM and every output o, G_o'G_o and G_o'1 of the forced-response matrix
// G_o(r, n Nu + l) = s_on(n1_o + r - l), r < N2 (MatG.m; zero where the step index is negative).
// They depend on the scenario alone, so the key forms H = sum_o q_o G_o'G_o + Lambda per candidate
// from them instead of re-correlating the step table in every workgroup.  Empty when the scenario
// has no step table, more than 4 outputs, or the tables would exceed kGramMaxBytes
inline void gram_tables(const mpct_scenario* s, std::vector<double>& g) {
  g.clear();
  const int my = s->my, nu = s->nu, n2max = s->n2max, numax = s->numax, tlen = s->tlen;
  if (s->nmpc || s->mdband || my > 4 || nu < 1 || nu > kGramM || s->step.empty()) return;
  const size_t blk = (size_t)my * kGramOut;
  if ((long long)((size_t)n2max * numax * blk * 8) > kGramMaxBytes) return;
  g.assign((size_t)n2max * numax * blk, 0.0);
  for (int N2 = 1; N2 <= n2max; ++N2)
    for (int Nu = 1; Nu <= std::min(N2, numax) && nu * Nu <= kGramM; ++Nu) {
      const int M = nu * Nu;
      double* b = g.data() + ((size_t)(N2 - 1) * numax + (Nu - 1)) * blk;
      for (int o = 0; o < my; ++o) {
        double* go = b + (size_t)o * kGramOut;
        const int n1 = s->n1[o];
        const double* so = s->step.data() + (size_t)o * nu * tlen;
        for (int a = 0; a < M; ++a) {
          const int na = a / Nu, la = a - na * Nu;
          const double* sa = so + (size_t)na * tlen + n1 - la;  // sa[r] = s_o,na(n1 + r - la)
          double cs = 0.0;
          for (int r = std::max(la - n1, 0); r < N2; ++r) cs += sa[r];
          go[kGramM * kGramM + a] = cs;
          for (int bb = a; bb < M; ++bb) {
            const int nb = bb / Nu, lb = bb - nb * Nu;
            const double* sb = so + (size_t)nb * tlen + n1 - lb;
            double h = 0.0;
            for (int r = std::max(std::max(la, lb) - n1, 0); r < N2; ++r) h += sa[r] * sb[r];
            go[a * kGramM + bb] = h;
            go[bb * kGramM + a] = h;
          }
        }
      }
    }
}

// the prologue's pre-factored rows (DevScenario::qrt, gpc_prologue.h).  Output i contributes the rows
// sqrt(delta_i) [G_i | Phi_i] to the prologue's QR, with G_i (N2 x M, M = nu Nu, the entries of
// gram_tables' G_o) and Phi_i (N2 x nx, the device basis phid) depending on the scenario and the
// horizon pair alone.  With the Householder QR G_i = Q_i R_i and T_i = Q_i' Phi_i,
//   W'W = sum_i delta_i R_i'R_i + Lambda   and   W'V = sum_i delta_i R_i'T_i,
// so the QR of the stacked rows sqrt(delta_i) [R_i | T_i], seeded with Lambda^1/2, gives the
// prologue's R and T = Q1'V; no normal equations are formed.  For every pair N2 <= n2max,
// Nu <= min(N2, numax) the table holds the first min(N2, M) rows of every [R_i | T_i], width M + nx,
// interleaved over the outputs: row my k + i is row k of output i, which is zero left of column k, so
// a block of the kernel's row stream is one contiguous read whose first nonzero column is known.  A
// column that is already zero below its diagonal (dead time; the last row) takes no reflection.
// off[(N2 - 1) numax + Nu - 1] is the cell's offset in doubles, -1 where there is no cell.  Both
// stay empty when the scenario has no free-response table (band, NMPC) or the rows would exceed
// max_bytes
inline void qr_tables(const mpct_scenario* s, std::vector<double>& q, std::vector<int>& off,
                      long long max_bytes = kQrtMaxBytes) {
  q.clear();
  off.clear();
  const int my = s->my, nu = s->nu, nx = s->nx, n2max = s->n2max, numax = s->numax, tlen = s->tlen;
  if (s->nmpc || s->mdband || nu < 1 || s->step.empty() || s->phid.empty()) return;
  std::vector<int> o((size_t)n2max * numax, -1);
  long long total = 0;
  for (int N2 = 1; N2 <= n2max; ++N2)
    for (int Nu = 1; Nu <= std::min(N2, numax); ++Nu) {
      const int M = nu * Nu;
      o[(size_t)(N2 - 1) * numax + (Nu - 1)] = (int)total;
      total += (long long)my * std::min(N2, M) * (M + nx);
      if (total * 8 > max_bytes) return;
    }
  q.assign((size_t)total, 0.0);
  std::vector<double> a;  // [G_i | Phi_i], N2 x (M + nx), factored in place
  for (int N2 = 1; N2 <= n2max; ++N2)
    for (int Nu = 1; Nu <= std::min(N2, numax); ++Nu) {
      const int M = nu * Nu, W = M + nx, rn = std::min(N2, M);
      double* cell = q.data() + o[(size_t)(N2 - 1) * numax + (Nu - 1)];
      for (int i = 0; i < my; ++i) {
        a.assign((size_t)N2 * W, 0.0);
        for (int r = 0; r < N2; ++r) {
          double* row = &a[(size_t)r * W];
          for (int c = 0; c < M; ++c) {
            const int n = c / Nu, tt = s->n1[i] + r - (c - n * Nu);
            row[c] = tt >= 0 ? s->step[((size_t)i * nu + n) * tlen + tt] : 0.0;
          }
          std::copy_n(&s->phid[((size_t)i * n2max + r) * nx], nx, row + M);
        }
        for (int k = 0; k < rn; ++k) {
          double sig = 0.0;
          for (int r = k + 1; r < N2; ++r) sig += a[(size_t)r * W + k] * a[(size_t)r * W + k];
          if (sig == 0.0) continue;
          const double x0 = a[(size_t)k * W + k], nrm = std::sqrt(x0 * x0 + sig);
          const double alpha = x0 > 0.0 ? -nrm : nrm, v0 = x0 - alpha;  // same signs: no cancellation
          const double tau = 2.0 / (v0 * v0 + sig);
          for (int c = k + 1; c < W; ++c) {
            double dot = v0 * a[(size_t)k * W + c];
            for (int r = k + 1; r < N2; ++r) dot += a[(size_t)r * W + k] * a[(size_t)r * W + c];
            dot *= tau;
            a[(size_t)k * W + c] -= dot * v0;
            for (int r = k + 1; r < N2; ++r) a[(size_t)r * W + c] -= dot * a[(size_t)r * W + k];
          }
          a[(size_t)k * W + k] = alpha;
          for (int r = k + 1; r < N2; ++r) a[(size_t)r * W + k] = 0.0;
        }
        for (int k = 0; k < rn; ++k) std::copy_n(&a[(size_t)k * W], W, cell + ((size_t)k * my + i) * W);
      }
    }
  off = std::move(o);
}

// longest run of numerator taps from an entry's first nonzero one (mdband_kernel.hip keeps only
// those in LDS: the delay's leading zeros are skipped by pl_off / mz_off anyway)
inline int compact_taps(const ZTables& z) {
  int m = 1;
  for (size_t e = 0; e < z.nb.size(); ++e) m = std::max(m, z.nb[e] - z.off[e]);
  return m;
}

// the scenario as the device code sees it: every scalar field and kernel-choice flag set, every
// table pointer null (the layout, LDS-size and kernel-instance queries need no more; pack_tables
// adds the tables).  tb, when given, receives the small kernels' lane tables
inline DevScenario dev_scenario(const mpct_scenario* s, SmallTables* tb = nullptr) {
  SmallTables local;
  if (!tb) tb = &local;
  DevScenario ds{};
  ds.my = s->my;
  ds.nu = s->nu;
  ds.nd = s->nd + s->nq;  // ring-fed plant inputs (their signals are v's rows)
  ds.nin = s->npin;       // plant input columns
  ds.nit = s->nit;
  ds.n2max = s->n2max;
  ds.numax = s->numax;
  ds.tlen = s->tlen;
  ds.nx = s->nx;
  ds.nyh = s->nyh;
  ds.nup = s->nup;
  ds.wsq = s->wsq;
  ds.ink0 = s->ink0;
  ds.ne = s->ne;
  ds.pl_maxb = s->pl.maxb;
  ds.pl_maxa = s->pl.maxa;
  ds.regpath = regpath(s);
  ds.small = small_plant(s, tb) ? 1 : 0;
  ds.small_dtc = !ds.small && dtc_small_plant(s, tb) ? 1 : 0;
  ds.sm_ke = tb->ke;
  ds.dtc = s->dtc;
  ds.nvar = s->nvar;
  ds.mz_maxb = s->mz.maxb;
  ds.mz_maxa = s->mz.maxa;
  ds.fr_max = s->fr_max;
  ds.mdband = s->mdband;
  ds.est = s->est;
  ds.rho = s->rho;
  ds.pl_maxbc = compact_taps(s->pl);
  ds.mz_maxbc = compact_taps(s->mz);
  ds.nmpc = s->nmpc;
  ds.nsub = s->nsub;
  ds.sqp_max = s->sqp_max;
  ds.ts = s->ts;
  ds.sqp_tol = s->sqp_tol;
  return ds;
}

// every table of a scenario in one blob of 256-B-aligned pieces, and the DevScenario that goes with
// it: ds holds the scalars, slots name each table pointer of ds with its place in the blob
struct PackedTables {
  template <class T>
  struct Slot {
    const T* DevScenario::*field;
    size_t off, bytes;
  };
  std::vector<char> blob;
  DevScenario ds{};
  std::vector<Slot<double>> dslots;
  std::vector<Slot<int>> islots;
  // ds with its table pointers set for a copy of the blob at base
  DevScenario rebased(const void* base) const {
    DevScenario r = ds;
    const char* b = static_cast<const char*>(base);
    for (const auto& t : dslots) r.*t.field = reinterpret_cast<const double*>(b + t.off);
    for (const auto& t : islots) r.*t.field = reinterpret_cast<const int*>(b + t.off);
    return r;
  }
};

inline PackedTables pack_tables(const mpct_scenario* s) {
  PackedTables p;
  SmallTables smt;
  p.ds = dev_scenario(s, &smt);
  std::vector<double> gram;
  gram_tables(s, gram);
  auto place = [&p](const void* src, size_t bytes) {
    const size_t off = (p.blob.size() + 255) & ~(size_t)255;
    p.blob.resize(off + bytes);
    if (bytes) std::memcpy(p.blob.data() + off, src, bytes);
    return off;
  };
  auto putd = [&](const double* DevScenario::*f, const std::vector<double>& v) {
    p.dslots.push_back({f, place(v.data(), v.size() * 8), v.size() * 8});
  };
  auto puti = [&](const int* DevScenario::*f, const std::vector<int>& v) {
    p.islots.push_back({f, place(v.data(), v.size() * 4), v.size() * 4});
  };
  // one line per table; the order is the blob's layout
  putd(&DevScenario::step, s->step);
  putd(&DevScenario::phi, s->phid);
  puti(&DevScenario::n1, s->n1);
  puti(&DevScenario::yoff, s->yoff);
  puti(&DevScenario::nyhi, s->nyhi);
  puti(&DevScenario::upoff, s->upoff);
  puti(&DevScenario::dum, s->dum);
  puti(&DevScenario::pl_nb, s->pl.nb);
  puti(&DevScenario::pl_na, s->pl.na);
  puti(&DevScenario::pl_off, s->pl.off);
  putd(&DevScenario::pl_b, s->pl.b);
  putd(&DevScenario::pl_a, s->pl.a);
  putd(&DevScenario::bnd, s->bnd);
  putd(&DevScenario::yref, s->yref);
  puti(&DevScenario::mz_nb, s->mz.nb);
  puti(&DevScenario::mz_na, s->mz.na);
  puti(&DevScenario::mz_off, s->mz.off);
  putd(&DevScenario::mz_b, s->mz.b);
  putd(&DevScenario::mz_a, s->mz.a);
  puti(&DevScenario::fr_n, s->fr_n);
  putd(&DevScenario::fr_b, s->fr_b);
  putd(&DevScenario::fr_a, s->fr_a);
  putd(&DevScenario::step_md, s->step_md);
  putd(&DevScenario::obnd, s->obnd);
  putd(&DevScenario::wscale, s->wscale);
  puti(&DevScenario::xc, s->xc);
  putd(&DevScenario::nm, s->nm);
  putd(&DevScenario::nmv, s->nmv);
  if (s->nmv.empty()) p.dslots.pop_back();  // plant = model: the pointer stays null
  putd(&DevScenario::gram, gram);
  if (gram.empty()) p.dslots.pop_back();  // not built: the pointer stays null (its padding stays in the blob)
  // the prologue's pre-factored rows, for the kernel that reads them (gpc_small_kernel); not built,
  // over kQrtMaxBytes or switched off: both pointers stay null and the prologue streams its rows
  std::vector<double> qrt;
  std::vector<int> qoff;
  if (p.ds.small && s->qr_tables) qr_tables(s, qrt, qoff);
  if (!qrt.empty()) {
    putd(&DevScenario::qrt, qrt);
    puti(&DevScenario::qrt_off, qoff);
  }
  putd(&DevScenario::sm_coef, smt.coef);
  puti(&DevScenario::sm_hoff, smt.hoff);
  puti(&DevScenario::sm_hc, smt.hc);
  puti(&DevScenario::sm_hmask, smt.hmask);
  puti(&DevScenario::sm_acol, smt.acol);
  putd(&DevScenario::sm_fr, smt.fr);
  return p;
}

}  // namespace mpct
