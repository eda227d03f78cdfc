// mpct_host.cpp — C ABI of libmpct: everything that touches HIP (device contexts, table upload,
// launch wrappers, the multi-GPU fan-out).  Descriptor validation and the host precompute of the
// candidate-independent tables are scenario_tables.h.  See include/mpct.h.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstring>
#include <string>
#include <vector>
#include <cstdio>
#include <thread>

#include "scenario_tables.h"
#include "launch_fan.h"
#include "work_order.h"
#include "dtc_robust.h"
#include "pareto.h"
#include "goal_attain.h"
#include "hv_select.h"
#include "hypervolume.h"
#include "hypervolume_exact.h"
#include "traj_indices.h"
#include "limit_indices.h"
#include "osc_indices.h"
#include "segment_indices.h"
#include "draw_stats.h"
#include "envelope.h"

namespace mpct {
// defined in gpc_kernel_launch.hip
int launch_closed_loop(const DevScenario& sc, long long C, int nref, const int* N2, const int* Nu,
                       const double* delta, const double* lambda, const double* r,
                       const double* v, const DevOpts& o, const DevResult& out, int maxM,
                       WorkOrder* wo, LaunchFan* fan, long long wide, int ncu, hipStream_t stream, std::string* err);
long long lds_bytes_for(const DevScenario& sc, int N2, int Nu, bool ext);
std::string closed_loop_instance(const DevScenario& sc, int maxM, bool ext);
// defined in mdband_kernel.hip
int launch_mdband(const DevScenario& sc, long long C, int nref, const int* N2, const int* Nu, const double* delta,
                  const double* lambda, const double* r, const double* v, const DevOpts& o, const DevResult& out,
                  hipStream_t stream, LaunchFan* fan, std::string* err);
long long mdband_lds_bytes(const DevScenario& sc, int N2, int Nu, int ncopy);
// defined in nmpc_kernel.hip
int launch_nmpc(const DevScenario& sc, long long C, int nref, const int* N, const int* Nu, const double* delta,
                const double* lambda, const double* r, const DevOpts& o, const DevResult& out, hipStream_t stream,
                LaunchFan* fan, WorkOrder* wo, std::string* err);
long long nmpc_lds_bytes(int M, int N);
}  // namespace mpct

using namespace mpct;

static thread_local std::string g_err;

static int fail(int code, const std::string& msg) {
  g_err = msg;
  return code;
}

// The batch arguments of the scenario-taking entries: C candidates (N2, Nu, delta [C][my], lambda [C][nu])
// against nref signal sets r | v.  An entry builds one from its arguments, host or device pointers as it
// takes them; HostStage::upload() turns a host one into its device-side twin.
struct Batch {
  int64_t C;
  const int32_t *N2, *Nu;
  const double *delta, *lambda;
  int32_t nref;
  const double *r, *v;
  // the candidates [c0, c0 + n) against the same signals
  Batch sub(int64_t c0, int64_t n, int my, int nu) const {
    return Batch{n, N2 + c0, Nu + c0, delta + c0 * my, lambda + c0 * nu, nref, r, v};
  }
};

// A grow-only device buffer that the calls of one context share across streams.  mark() records the event
// behind the last launch that uses the buffer; acquire() orders the next call's stream after it before the
// buffer is rewritten.  A regrow waits on the host for that event and then for `stream` before the old
// buffer is freed.
struct EventScratch {
  void* buf = nullptr;
  size_t bytes = 0;
  hipEvent_t used = nullptr;
  bool pending = false;

  int acquire(size_t need, hipStream_t stream, const char* what, char** out) {
    if (!used && hipEventCreateWithFlags(&used, hipEventDisableTiming) != hipSuccess)
      return fail(MPCT_EDEVICE, "hipEventCreate failed");
    if (need > bytes) {
      if (pending) (void)hipEventSynchronize(used);
      pending = false;
      if (buf) {
        (void)hipStreamSynchronize(stream);
        (void)hipFree(buf);
      }
      buf = nullptr;
      bytes = 0;
      if (hipMalloc(&buf, need) != hipSuccess) return fail(MPCT_ENOMEM, std::string("hipMalloc(") + what + ") failed");
      bytes = need;
    }
    if (pending && hipStreamWaitEvent(stream, used, 0) != hipSuccess) return fail(MPCT_EDEVICE, "hipStreamWaitEvent failed");
    *out = static_cast<char*>(buf);
    return MPCT_OK;
  }
  void mark(hipStream_t stream) { pending = hipEventRecord(used, stream) == hipSuccess; }
  void release() {
    if (pending) (void)hipEventSynchronize(used);
    if (buf) (void)hipFree(buf);
    if (used) (void)hipEventDestroy(used);
  }
};

// Everything a scenario keeps on one device.  The host-pointer entries run on the library-owned
// stream `stream` and synchronise only it (not the device), so other streams, host threads and
// the contexts of other devices proceed concurrently.
struct DevCtx {
  int dev = -1;
  void* dtab = nullptr;  // the scenario's tables, one 256-B-aligned blob
  DevScenario ds{};
  void* dscratch = nullptr;  // host-API input/result buffers (grow only)
  size_t dscratch_bytes = 0;
  // host-API reference / disturbance signals r | v: the last upload stays on the device and a
  // call whose signals are byte-identical skips the copy (the drop-in's scalar calls pass the
  // same Xsp every time: GAM_fun.m:81, VNS2.m:153)
  void* dsig = nullptr;
  size_t dsig_bytes = 0;
  std::vector<char> sig_host;  // bytes of the signals dsig holds
  hipStream_t stream = nullptr;
  LaunchFan fan;    // auxiliary streams of the class launches (band / NMPC kernels)
  WorkOrder order;  // dispatch-order sort buffers (GPC and NMPC kernels)
  // robust scoring: per-simulation J1 / status of the generic path, candidate lists (and the tail's J1
  // sample) of the fused one
  EventScratch robust;
  int ncu = 0;  // compute units (grid of the fused robust kernel)
  // the index entries: the trajectories y | u of one chunk of candidates (at most MPCT_INDEX_SCRATCH_BYTES or
  // one candidate's) and, for the robust indices, the chunk's J1, status, alive and index records
  EventScratch index;
};

// the return of a launch wrapper whose device function reports 0, -2 (no memory) or another failure
static int32_t launch_rc(int rc, const std::string& err) {
  return rc ? fail(rc == -2 ? MPCT_ENOMEM : MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_abi_version(void) { return MPCT_ABI_VERSION; }
extern "C" const char* mpct_last_error(void) { return g_err.c_str(); }

// hand a builder's scenario to the caller, or report why there is none
static int32_t created(std::unique_ptr<mpct_scenario> s, const BuildError& err, mpct_scenario** out) {
  if (!s) return fail(err.code, err.msg);
  // MPCT_NO_QR_TABLES=1 at creation: this scenario's prologue streams its rows (scenario_tables.h
  // qr_tables are not packed), so both row sources can be run and timed in one process
  const char* e = getenv("MPCT_NO_QR_TABLES");
  if (e && *e && atoi(e) != 0) s->qr_tables = 0;
  // MPCT_WIDE_SLOTS=n at creation: this scenario's ordered metric launches run their first n slots on
  // the wide instance (0: the single launch) instead of the rule's count, for A/B runs and tests
  const char* w = getenv("MPCT_WIDE_SLOTS");
  if (w && *w && atoll(w) >= 0) s->wide_slots = atoll(w);
  *out = s.release();
  g_err.clear();
  return MPCT_OK;
}

extern "C" int32_t mpct_scenario_create(const mpct_scenario_desc* d, mpct_scenario** out) {
  if (!d || !out) return fail(MPCT_EINVAL, "null argument");
  *out = nullptr;
  BuildError err;
  return created(build_scenario(*d, &err), err, out);
}

extern "C" int32_t mpct_scenario_create_est(const mpct_scenario_desc* d, int32_t estimator, mpct_scenario** out) {
  if (!d || !out) return fail(MPCT_EINVAL, "null argument");
  *out = nullptr;
  BuildError err;
  return created(build_scenario(*d, &err, estimator), err, out);
}

extern "C" int32_t mpct_nmpc_scenario_create(const mpct_nmpc_desc* d, mpct_scenario** out) {
  return mpct_nmpc_scenario_create_var(d, 0, nullptr, nullptr, out);
}

extern "C" int32_t mpct_nmpc_scenario_create_var(const mpct_nmpc_desc* d, int32_t nplant, const double* plant_params,
                                                 const double* plant_x0, mpct_scenario** out) {
  if (!d || !out) return fail(MPCT_EINVAL, "null argument");
  *out = nullptr;
  BuildError err;
  if (!nmpc_dims_ok(*d, &err)) return fail(err.code, err.msg);
  // the LDS of every (M, N) a candidate may use (not monotone in N: nm_groups), as the launch checks
  long long lds_all = 0;
  for (int m = 1; m <= d->nu * d->nu_max; ++m)
    for (int n = 1; n <= d->n_max; ++n) lds_all = std::max(lds_all, nmpc_lds_bytes(m, n));
  if (lds_all > 64 * 1024) return fail(MPCT_ERANGE, "n_max x nu*nu_max needs more than 64 KiB of LDS per simulation");
  // the plant variants (nx = 3 holds: nmpc_dims_ok)
  if (nplant < 0) return fail(MPCT_EINVAL, "nplant must be >= 0");
  if (nplant == 0 && (plant_params || plant_x0))
    return fail(MPCT_EINVAL, "nplant = 0 takes no plant_params and no plant_x0");
  if (nplant > 0 && !plant_params) return fail(MPCT_EINVAL, "nplant >= 1 needs plant_params");
  for (int k = 0; k < nplant; ++k) {
    const double* q = plant_params + (size_t)k * NM_NPAR;
    for (int i = 0; i < NM_NPAR; ++i)
      if (!std::isfinite(q[i])) return fail(MPCT_EINVAL, "non-finite plant parameter");
    if (q[NM_RHO] * q[NM_CP] * q[NM_V] == 0.0) return fail(MPCT_EINVAL, "plant variant with rho*cp*V = 0");
    for (int i = 0; plant_x0 && i < d->nx; ++i)
      if (!std::isfinite(plant_x0[(size_t)k * d->nx + i])) return fail(MPCT_EINVAL, "non-finite plant_x0");
  }
  return created(build_nmpc_scenario(*d, &err, nplant, plant_params, plant_x0), err, out);
}

static void ctx_release(DevCtx* c) {
  (void)hipSetDevice(c->dev);
  if (c->stream) (void)hipStreamSynchronize(c->stream);
  if (c->dtab) (void)hipFree(c->dtab);
  if (c->dscratch) (void)hipFree(c->dscratch);
  if (c->dsig) (void)hipFree(c->dsig);
  c->robust.release();
  c->index.release();
  order_release(c->order);
  c->fan.release();
  if (c->stream) (void)hipStreamDestroy(c->stream);
  delete c;
}

extern "C" void mpct_scenario_destroy(mpct_scenario* s) {
  if (!s) return;
  int cur = -1;
  bool any = std::any_of(s->ctx.begin(), s->ctx.end(), [](DevCtx* c) { return c != nullptr; });
  for (auto& v : s->extra) any = any || !v.empty();
  if (any && hipGetDevice(&cur) != hipSuccess) cur = -1;
  for (DevCtx* c : s->ctx)
    if (c) ctx_release(c);
  for (auto& v : s->extra)
    for (DevCtx* c : v) ctx_release(c);
  if (cur >= 0) (void)hipSetDevice(cur);
  delete s;
}

extern "C" int64_t mpct_scenario_table(const mpct_scenario* s, int32_t which, double* buf, int64_t cap) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  std::vector<double> dims;
  const std::vector<double>* src = nullptr;
  if (which == 0)
    src = &s->step;
  else if (which == 1)
    src = &s->phi;
  else if (which == 3)
    src = &s->phid;
  else if (which == 2) {
    dims = {(double)s->my, (double)s->nu, (double)s->nd, (double)s->n2max, (double)s->numax,
            (double)s->tlen, (double)s->nx, (double)s->nyh, (double)s->nup, (double)s->nit, (double)s->nq};
    src = &dims;
  } else if (which == 4) {  // what pack_tables packs: the rows of a small plant unless switched off
    std::vector<int> off;
    if (s->qr_tables && dev_scenario(s).small) qr_tables(s, dims, off);
    src = &dims;
  } else
    return fail(MPCT_EINVAL, "unknown table");
  int64_t n = (int64_t)src->size();
  if (buf && cap > 0) std::memcpy(buf, src->data(), sizeof(double) * (size_t)std::min<int64_t>(n, cap));
  return n;
}

// a new context on device dev (current): the scenario's tables uploaded, its own stream
static int build_ctx(mpct_scenario* s, int dev, DevCtx** out) {
  const PackedTables pk = pack_tables(s);
  void* dp = nullptr;
  if (hipMalloc(&dp, pk.blob.size()) != hipSuccess) return fail(MPCT_ENOMEM, "hipMalloc(tables) failed");
  if (hipMemcpy(dp, pk.blob.data(), pk.blob.size(), hipMemcpyHostToDevice) != hipSuccess) {
    (void)hipFree(dp);
    return fail(MPCT_EDEVICE, "hipMemcpy(tables) failed");
  }
  DevCtx* cx = new DevCtx();
  if (hipStreamCreateWithFlags(&cx->stream, hipStreamNonBlocking) != hipSuccess) {
    (void)hipFree(dp);
    delete cx;
    return fail(MPCT_EDEVICE, "hipStreamCreate failed");
  }
  cx->ds = pk.rebased(dp);
  cx->dtab = dp;
  cx->dev = dev;
  if (!cx->fan.init(dev)) cx->fan.release();  // class launches over streams; no fan: one stream, still correct
  *out = cx;
  return MPCT_OK;
}

// the context of device want_dev (-1: the calling thread's current device), created and its
// tables uploaded on first use; makes that device current for the calling thread.
// occurrence j of device want_dev in one call (0: the primary context; j >= 1: extra[dev][j-1])
static int device_ctx(mpct_scenario* s, int want_dev, DevCtx** out, int occurrence = 0) {
  int dev = want_dev;
  if (dev < 0) {
    if (hipGetDevice(&dev) != hipSuccess) return fail(MPCT_EDEVICE, "hipGetDevice failed (no GPU?)");
  }
  int cnt = 0;
  if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0) return fail(MPCT_EDEVICE, "no HIP device");
  if (dev >= cnt) return fail(MPCT_EINVAL, "device ordinal out of range");
  if (hipSetDevice(dev) != hipSuccess) return fail(MPCT_EDEVICE, "hipSetDevice failed");
  if ((int)s->ctx.size() < cnt) s->ctx.resize(cnt, nullptr);
  if ((int)s->extra.size() < cnt) s->extra.resize(cnt);
  DevCtx** slot = nullptr;
  if (occurrence == 0) {
    slot = &s->ctx[dev];
  } else {
    auto& ex = s->extra[dev];
    if ((int)ex.size() < occurrence) ex.resize(occurrence, nullptr);
    slot = &ex[occurrence - 1];
  }
  if (!*slot) {
    const int rc = build_ctx(s, dev, slot);
    if (rc) return rc;
  }
  *out = *slot;
  return MPCT_OK;
}

// the primary context of the device the call's options name
static int ctx_for(mpct_scenario* s, const mpct_opts* opts, DevCtx** out) {
  return device_ctx(s, opts ? opts->device : -1, out);
}

static DevOpts make_opts(const mpct_opts* o) {
  DevOpts d{};
  d.open_loop = o ? o->open_loop : 0;
  d.want_traj = o ? o->want_traj : 0;
  d.max_qp_iter = o ? o->max_qp_iter : 0;
  d.feas_tol = (o && o->feas_tol > 0) ? o->feas_tol : 1e-10;
#ifdef MPCT_DIAG
  const char* e = getenv("MPCT_DIAG_SKIP_WARM_DROP");
  d.diag = (e && *e && atoi(e) != 0) ? kDiagSkipWarmDrop : 0;
#endif
  return d;
}

// the argument checks of the three eval entries; devlist_ok: mpct_eval_batch_multi's device list
static int check_args(mpct_scenario* s, const Batch& b, const mpct_opts* opts, const mpct_result* out,
                      bool devlist_ok = true) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (b.C < 0 || b.nref < 1) return fail(MPCT_EINVAL, "C < 0 or nref < 1");
  if (b.C * (int64_t)b.nref > 0x7fffffffLL) return fail(MPCT_ERANGE, "too many simulations in one call");
  if (b.C > 0 && (!b.N2 || !b.Nu || !b.delta || !b.lambda || !b.r)) return fail(MPCT_EINVAL, "null input pointer");
  if (s->nd + s->nq > 0 && !b.v) return fail(MPCT_EINVAL, "v required when nd + nq > 0");
  if (!out) return fail(MPCT_EINVAL, "null result");
  if (!devlist_ok) return fail(MPCT_EINVAL, "ndev must be 1..64 with a device list");
  if (s->dtc && opts && opts->open_loop) return fail(MPCT_EINVAL, "DTC mode has no open-loop prediction");
  // the parallel model of the output-bias estimator runs in the open-loop leg's plant copy
  if (s->est && opts && opts->open_loop)
    return fail(MPCT_EINVAL, "estimator scenarios are closed-loop only: open_loop must be 0");
  return MPCT_OK;
}

// enqueue one batch with device pointers on `stream` (ctx's device is current)
static int launch_batch(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const mpct_result* out,
                        hipStream_t stream) {
  if (b.C == 0) return MPCT_OK;
  DevOpts dop = make_opts(opts);
  DevResult dr{out->J1, out->j21, out->j22, out->Jnu, out->status, out->qp_iters,
                out->y, out->u, out->ys, out->uopt, nullptr};
#ifdef MPCT_PROFILE
  // diagnostic build: per-simulation section cycle sums, summarised on stderr
  const long long S = b.C * b.nref;
  unsigned long long* dprof = nullptr;
  (void)hipMalloc(&dprof, sizeof(unsigned long long) * S * PROF_N);
  dr.prof = dprof;
#endif
#ifdef MPCT_TIMELINE
  // diagnostic build: [slot][t0, t1, HW_ID << 32 | XCC_ID, sim] -> $MPCT_TIMELINE_OUT
  const long long S = b.C * b.nref;
  unsigned long long* dprof = nullptr;
  (void)hipMalloc(&dprof, sizeof(unsigned long long) * S * 4);
  (void)hipMemset(dprof, 0, sizeof(unsigned long long) * S * 4);
  dr.prof = dprof;
#endif
  std::string err;
  int rc = 0;
  // no class launch writes the trajectories of a skipped or bad-horizon simulation: NaN, like its costs
  if (dop.want_traj)
    rc = fill_unrun_trajectories(dr, b.C, b.nref, b.N2, b.Nu, cx->ds.n2max, cx->ds.numax, s->my, s->nu, s->nit,
                                 dop.open_loop != 0, stream, &err);
  if (rc) return fail(rc, err);
  if (s->nmpc)
    rc = launch_nmpc(cx->ds, b.C, b.nref, b.N2, b.Nu, b.delta, b.lambda, b.r, dop, dr, stream, &cx->fan, &cx->order, &err);
  else if (s->mdband)
    rc = launch_mdband(cx->ds, b.C, b.nref, b.N2, b.Nu, b.delta, b.lambda, b.r, b.v, dop, dr, stream, &cx->fan, &err);
  else {
    if (cx->ncu == 0 &&
        (hipDeviceGetAttribute(&cx->ncu, hipDeviceAttributeMultiprocessorCount, cx->dev) != hipSuccess || cx->ncu < 1))
      cx->ncu = 0;
    rc = launch_closed_loop(cx->ds, b.C, b.nref, b.N2, b.Nu, b.delta, b.lambda, b.r, b.v, dop, dr, s->nu * s->numax,
                            &cx->order, &cx->fan, s->wide_slots, cx->ncu, stream, &err);
  }
  if (rc) return fail(rc, err);
#ifdef MPCT_TIMELINE
  {
    std::vector<unsigned long long> hp(S * 4);
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(hp.data(), dprof, sizeof(unsigned long long) * S * 4, hipMemcpyDeviceToHost);
    (void)hipFree(dprof);
    const char* path = getenv("MPCT_TIMELINE_OUT");
    if (path) {
      FILE* f = fopen(path, "wb");
      if (f) {
        fwrite(hp.data(), sizeof(unsigned long long), hp.size(), f);
        fclose(f);
      }
    }
  }
#endif
#ifdef MPCT_PROFILE
  {
    std::vector<unsigned long long> hp(S * PROF_N);
    (void)hipStreamSynchronize(stream);
    (void)hipMemcpy(hp.data(), dprof, sizeof(unsigned long long) * S * PROF_N, hipMemcpyDeviceToHost);
    (void)hipFree(dprof);
    // low 40 bits: cycles, high 24: executions of the section (wave_ops.h PSTAMP, kProfCountShift)
    constexpr int kProfCountShift = 40;
    const unsigned long long cmask = (1ull << kProfCountShift) - 1;
    double sum[PROF_N] = {0}, mx[PROF_N] = {0}, cnt[PROF_N] = {0};
    for (long long i = 0; i < S; ++i)
      for (int k = 0; k < PROF_N; ++k) {
        sum[k] += (double)(hp[i * PROF_N + k] & cmask);
        cnt[k] += (double)(hp[i * PROF_N + k] >> kProfCountShift);
        mx[k] = std::max(mx[k], (double)(hp[i * PROF_N + k] & cmask));
      }
    if (const char* po = getenv("MPCT_PROF_OUT")) {  // per simulation, raw (tools/latency_model.py)
      FILE* f = fopen(po, "wb");
      if (f) {
        fwrite(hp.data(), sizeof(unsigned long long), hp.size(), f);
        fclose(f);
      }
    }
    const char* gpc_nm[PROF_N] = {"prologue", "plant", "y_update", "unconstrained", "qp(rest)", "u_update",
                                  "open_loop", "qp.check", "qp.d+z", "qp.r+t1", "qp.add", "qp.drop", "qp.warm",
                                  "qp.rotations", "qp.w.entry", "qp.w.rebuild", "qp.w.gather", "qp.w.solve",
                                  "qp.w.drop", "qp.w.rotations", "qp.w.readds"};
    const char* nmpc_nm[PROF_N] = {"full_pass", "rinv+step", "qp", "anderson_pass", "ls_full_pass", "ls_trials",
                                   "plant_rk4", "other", "n.passes", "n.points", "n.used", "n.rows", "-", "-", "-",
                                   "-", "-", "-", "-", "-", "-"};
    const char** nm = s->nmpc ? nmpc_nm : gpc_nm;
    fprintf(stderr, "[mpct profile] mean / max cycles and mean executions per simulation over %lld sims\n", S);
    for (int k = 0; k < PROF_N; ++k)
      fprintf(stderr, "  %-14s %12.0f %12.0f %10.1f\n", nm[k], sum[k] / (double)S, mx[k], cnt[k] / (double)S);
  }
#endif
  return MPCT_OK;
}

extern "C" int32_t mpct_eval_batch_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                          const double* delta, const double* lambda, int32_t nref,
                                          const double* r, const double* v, const mpct_opts* opts,
                                          mpct_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_args(s, b, opts, out);
  if (rc) return rc;
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_batch(s, cx, b, opts, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_rank_device(const double* costs, int64_t C, int32_t k, const double* w, int32_t* perm,
                                    void* stream) {
  if (C < 0 || C > 2147483647LL) return fail(MPCT_ERANGE, "C out of range for the ranking sort");
  if (k < 1) return fail(MPCT_EINVAL, "k < 1");
  if (C > 0 && (!costs || !w || !perm)) return fail(MPCT_EINVAL, "null pointer");
  std::string err;
  return launch_rc(rank_device(costs, C, k, w, perm, static_cast<hipStream_t>(stream), &err), err);
}

// Host-pointer staging of one call of a scenario-free entry (mpct_pareto, mpct_hypervolume, mpct_hv_select,
// mpct_hypervolume_exact, mpct_indices, mpct_draw_stats), the per-call counterpart of HostStage below: a
// stream and one device blob of this call's own, so the call needs no context and waits for nothing else.
// An entry reserves its slots before anything touches a device -- in(): a host array to upload, out(): a
// buffer of the caller's to fill -- then open()s, launches on `st` with at<T>(slot) as the device addresses
// and close()s with the launch's return code, whatever open() returned.
// A slot with a NULL host pointer or no bytes reserves nothing and its device address is NULL: a result
// field that is not asked for, members == NULL, alive == NULL and the trajectories mpct_indices has no use
// for reach the launch as NULL.
namespace {
struct CallStage {
  // the entry's words in the messages: "<entry> failed on the device", "hipMalloc failed (<staging>)",
  // "hipMemcpyAsync failed (<inputs>)", "hipMemcpyAsync failed (<results>)"
  const char *entry, *staging, *inputs, *results;
  static constexpr int kMaxSlots = 27;  // mpct_envelope, the widest entry: y, u, alive, two records of 9 and two spreads of 3
  struct Slot {
    void* host;  // NULL: nothing reserved
    size_t bytes, off;
    bool in;
  } slots[kMaxSlots] = {};
  int nslots = 0;
  size_t off = 0;  // bytes reserved so far
  hipStream_t st = nullptr;
  char* blob = nullptr;
  int cur = -1;           // the caller's device
  bool switched = false;  // open() made another device current
  bool staged = false;    // open() got its stream and blob: close() has work to wait for

  // reserve a 256-B-aligned slot of the blob; its address holds after open()
  int slot(const void* host, size_t bytes, bool in) {
    assert(nslots < kMaxSlots);
    Slot& s = slots[nslots];
    if (host && bytes) {
      s = Slot{const_cast<void*>(host), bytes, off, in};
      off += (bytes + 255) & ~(size_t)255;
    }
    return nslots++;
  }
  int in(const void* host, size_t bytes) { return slot(host, bytes, true); }
  int out(void* host, size_t bytes) { return slot(host, bytes, false); }
  template <class T>
  T* at(int i) const { return slots[i].host ? reinterpret_cast<T*>(blob + slots[i].off) : nullptr; }

  // make `device` (< 0: the current one) current, create the stream and the blob, enqueue the H2D copies
  int open(int device) {
    int cnt = 0;
    if (hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0 || hipGetDevice(&cur) != hipSuccess)
      return fail(MPCT_EDEVICE, std::string("no HIP device (") + entry + " needs a GPU)");
    const int dev = device < 0 ? cur : device;
    if (dev >= cnt) return fail(MPCT_EINVAL, "device ordinal out of range");
    if (dev != cur && hipSetDevice(dev) != hipSuccess) return fail(MPCT_EDEVICE, "hipSetDevice failed");
    switched = dev != cur;
    if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) return fail(MPCT_EDEVICE, "hipStreamCreate failed");
    if (hipMalloc(reinterpret_cast<void**>(&blob), off) != hipSuccess)
      return fail(MPCT_ENOMEM, std::string("hipMalloc failed (") + staging + ")");
    staged = true;
    for (int i = 0; i < nslots; ++i) {
      const Slot& s = slots[i];
      if (s.host && s.in && hipMemcpyAsync(blob + s.off, s.host, s.bytes, hipMemcpyHostToDevice, st) != hipSuccess)
        return fail(MPCT_EDEVICE, std::string("hipMemcpyAsync failed (") + inputs + ")");
    }
    return MPCT_OK;
  }

  // rc: what open() or the launch returned.  MPCT_OK: enqueue the D2H copies of the out() slots.  Always: wait
  // for this call's stream, free what open() got and give the caller's device back.  The first error wins
  int close(int rc) {
    if (staged) {
      for (int i = 0; rc == MPCT_OK && i < nslots; ++i) {
        const Slot& s = slots[i];
        if (s.host && !s.in && hipMemcpyAsync(s.host, blob + s.off, s.bytes, hipMemcpyDeviceToHost, st) != hipSuccess)
          rc = fail(MPCT_EDEVICE, std::string("hipMemcpyAsync failed (") + results + ")");
      }
      // this call's stream only, also after an error: the blob is freed below
      const hipError_t se = hipStreamSynchronize(st);
      if (rc == MPCT_OK && se != hipSuccess)
        rc = fail(MPCT_EDEVICE, std::string(entry) + " failed on the device: " + hipGetErrorString(se));
    }
    if (blob) (void)hipFree(blob);
    if (st) (void)hipStreamDestroy(st);
    if (switched) (void)hipSetDevice(cur);
    return rc;
  }
};
}  // namespace

// ---- Pareto front, domination counts and layers (pareto.hip).  The argument checks of both entries,
// in the order include/mpct.h states, before any device is touched
static int pareto_check(const double* costs, int64_t C, int32_t k, int32_t max_layers, const mpct_pareto_result* out) {
  if (k < 1 || k > MPCT_PARETO_MAX_OBJ) return fail(MPCT_EINVAL, "k must be 1 .. MPCT_PARETO_MAX_OBJ");
  if (C < 0) return fail(MPCT_EINVAL, "C < 0");
  if (C > MPCT_PARETO_MAX_C) return fail(MPCT_ERANGE, "C exceeds MPCT_PARETO_MAX_C");
  if (C > 0 && !costs) return fail(MPCT_EINVAL, "costs is NULL");
  if (!out || !(out->dom_count || out->layer || out->front || out->n_front))
    return fail(MPCT_EINVAL, "no output pointer in mpct_pareto_result");
  if (out->front && !out->n_front) return fail(MPCT_EINVAL, "front needs n_front");
  if (max_layers < 0 || max_layers > MPCT_PARETO_MAX_LAYERS || (out->layer && max_layers < 1))
    return fail(MPCT_EINVAL, "max_layers must be 1 .. MPCT_PARETO_MAX_LAYERS when layer is asked for (0 without)");
  return MPCT_OK;
}

static int32_t pareto_launch(const double* costs, int64_t C, int32_t k, int32_t max_layers, const mpct_pareto_result* out,
                             hipStream_t stream, int tile, int split) {
  std::string err;
  const ParetoOut po{out->dom_count, out->layer, out->front, out->n_front};
  return launch_rc(pareto_device(costs, C, k, max_layers, po, stream, &err, tile, split), err);
}

extern "C" int32_t mpct_pareto_device(const double* costs, int64_t C, int32_t k, int32_t max_layers,
                                      const mpct_pareto_result* out, void* stream) {
  const int rc = pareto_check(costs, C, k, max_layers, out);
  if (rc) return rc;
  return pareto_launch(costs, C, k, max_layers, out, static_cast<hipStream_t>(stream), 0, 0);
}

// the device entry with the tile length (128 or 256) and the number of a-chunks forced: the A/B of
// tools/pareto_bench.py and the empty-chunk test; a hook, not part of include/mpct.h
extern "C" int32_t mpct_internal_pareto_tuned(const double* costs, int64_t C, int32_t k, int32_t max_layers,
                                              const mpct_pareto_result* out, void* stream, int32_t tile, int32_t split) {
  const int rc = pareto_check(costs, C, k, max_layers, out);
  if (rc) return rc;
  if (split < 0 || split > 1024) return fail(MPCT_EINVAL, "split must be 0 .. 1024");
  return pareto_launch(costs, C, k, max_layers, out, static_cast<hipStream_t>(stream), tile, split);
}

// the grid the device entry launches for C candidates: {tile, chunks along a, competitors per chunk}
extern "C" int32_t mpct_internal_pareto_grid(int64_t C, int32_t* tile_split_chunk) {
  if (C < 0 || C > MPCT_PARETO_MAX_C || !tile_split_chunk) return fail(MPCT_EINVAL, "bad argument");
  int split = 1, chunk = kParetoTile;
  pareto_grid(C, kParetoTile, 0, &split, &chunk);
  tile_split_chunk[0] = kParetoTile;
  tile_split_chunk[1] = split;
  tile_split_chunk[2] = chunk;
  return MPCT_OK;
}

extern "C" int32_t mpct_pareto(const double* costs, int64_t C, int32_t k, int32_t max_layers, int32_t device,
                               const mpct_pareto_result* out) {
  int rc = pareto_check(costs, C, k, max_layers, out);
  if (rc) return rc;
  if (C == 0) {  // nothing to stage
    if (out->n_front) out->n_front[0] = 0;
    return MPCT_OK;
  }
  CallStage cs{"mpct_pareto", "Pareto staging", "costs", "Pareto results"};
  const size_t bi = (size_t)C * sizeof(int32_t);
  const int s_costs = cs.in(costs, (size_t)C * k * sizeof(double));
  const int s_dom = cs.out(out->dom_count, bi), s_layer = cs.out(out->layer, bi), s_front = cs.out(out->front, bi),
            s_nfront = cs.out(out->n_front, sizeof(int32_t));
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    mpct_pareto_result d{};
    d.dom_count = cs.at<int32_t>(s_dom);
    d.layer = cs.at<int32_t>(s_layer);
    d.front = cs.at<int32_t>(s_front);
    d.n_front = cs.at<int32_t>(s_nfront);
    rc = pareto_launch(cs.at<double>(s_costs), C, k, max_layers, &d, cs.st, 0, 0);
  }
  return cs.close(rc);
}

// ---- Goal-attainment selection (goal_attain.hip).  The argument checks of both entries, in the order
// include/mpct.h states, before any device is touched; nothing is dereferenced
static int goal_check(const double* costs, int64_t C, int32_t k, const double* goals, const double* weights, int64_t G,
                      int32_t n_best, const mpct_goal_result* out) {
  if (k < 1 || k > MPCT_PARETO_MAX_OBJ) return fail(MPCT_EINVAL, "k must be 1 .. MPCT_PARETO_MAX_OBJ");
  if (C < 0 || G < 0) return fail(MPCT_EINVAL, "C < 0 or G < 0");
  if (C > MPCT_PARETO_MAX_C || G > MPCT_GOAL_MAX_G) return fail(MPCT_ERANGE, "C exceeds MPCT_PARETO_MAX_C or G exceeds MPCT_GOAL_MAX_G");
  if (n_best < 0) return fail(MPCT_EINVAL, "n_best < 0");
  if (n_best > MPCT_GOAL_MAX_BEST) return fail(MPCT_ERANGE, "n_best exceeds MPCT_GOAL_MAX_BEST");
  if (C > 0 && !costs) return fail(MPCT_EINVAL, "costs is NULL");
  if (G > 0 && (!goals || !weights)) return fail(MPCT_EINVAL, "goals or weights is NULL");
  if (!out || !(out->best || out->gamma || out->active || out->n_feasible || out->n_attained || out->wins))
    return fail(MPCT_EINVAL, "no output pointer in mpct_goal_result");
  if (n_best == 0 && (out->best || out->gamma || out->active))
    return fail(MPCT_EINVAL, "best, gamma and active need n_best >= 1");
  return MPCT_OK;
}

// the number of chunks of the candidate range (0: the default, else 1 .. 1024) and the tile length (0: the
// default, 128 or 256) of goal_pair_kernel.  A test hook, not part of include/mpct.h: the tests reach the
// merge stage, partial and empty chunks at small shapes with it
static int32_t g_goal_split = 0, g_goal_tile = 0;
extern "C" int32_t mpct_internal_goal_grid(int32_t split, int32_t tile) {
  if (split < 0 || split > kGoalMaxSplit || (tile != 0 && tile != 128 && tile != 256))
    return fail(MPCT_EINVAL, "split must be 0 .. 1024, tile 0, 128 or 256");
  g_goal_split = split;
  g_goal_tile = tile;
  return MPCT_OK;
}

// the grid the device entry launches for G goal vectors and C candidates under the hook's current setting:
// {tile, chunks of the candidate range, candidates per chunk}
extern "C" int32_t mpct_internal_goal_geometry(int64_t G, int64_t C, int32_t* tile_split_chunk) {
  if (C < 0 || C > MPCT_PARETO_MAX_C || G < 0 || G > MPCT_GOAL_MAX_G || !tile_split_chunk) return fail(MPCT_EINVAL, "bad argument");
  const int tile = g_goal_tile ? g_goal_tile : kGoalTile;
  int split = 1, chunk = tile;
  goal_grid(G, C, tile, g_goal_split, &split, &chunk);
  tile_split_chunk[0] = tile;
  tile_split_chunk[1] = split;
  tile_split_chunk[2] = chunk;
  return MPCT_OK;
}

static int32_t goal_launch(const double* costs, int64_t C, int32_t k, const double* goals, const double* weights, int64_t G,
                           int32_t n_best, const mpct_goal_result* out, hipStream_t stream) {
  std::string err;
  const GoalOut go{out->best, out->gamma, out->active, out->n_feasible, out->n_attained, out->wins};
  return launch_rc(goal_attain_device(costs, C, k, goals, weights, G, n_best, go, stream, &err, g_goal_tile, g_goal_split), err);
}

extern "C" int32_t mpct_goal_attain_device(const double* costs, int64_t C, int32_t k, const double* goals,
                                           const double* weights, int64_t G, int32_t n_best, const mpct_goal_result* out,
                                           void* stream) {
  const int rc = goal_check(costs, C, k, goals, weights, G, n_best, out);
  if (rc) return rc;
  return goal_launch(costs, C, k, goals, weights, G, n_best, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_goal_attain(const double* costs, int64_t C, int32_t k, const double* goals, const double* weights,
                                    int64_t G, int32_t n_best, int32_t device, const mpct_goal_result* out) {
  int rc = goal_check(costs, C, k, goals, weights, G, n_best, out);
  if (rc) return rc;
  // the check that reads the caller's arrays, which only this entry can make: the validity rule of include/mpct.h
  for (int64_t g = 0; g < G; ++g) {
    bool ok = true, soft = false;
    for (int j = 0; j < k; ++j) {
      const double w = weights[g * k + j], gl = goals[g * k + j];
      if (w == 0.0) {
        ok = ok && !std::isnan(gl);
      } else if (w > 0.0 && std::isfinite(w)) {
        ok = ok && std::isfinite(1.0 / w) && std::isfinite(gl);
        soft = true;
      } else {
        ok = false;
      }
    }
    if (!ok || !soft)
      return fail(MPCT_EINVAL, "goal vector " + std::to_string(g) + " is invalid: a weight is 0 or finite and positive with a "
                  "finite reciprocal, one weight at least is positive, a goal is finite (not NaN where the weight is 0)");
  }
  if (G == 0) {  // nothing to stage: wins is all there is to write.  Otherwise the device zeroes it, so a call
                 // that fails to open its device has written to none of the caller's buffers
    if (out->wins) std::memset(out->wins, 0, (size_t)C * sizeof(int32_t));
    return MPCT_OK;
  }
  if (C == 0) {  // nothing to stage either (wins has no entry): no candidate is feasible for the (valid) goal vectors
    const double nan = std::nan("");
    for (int64_t e = 0; e < G * n_best; ++e) {
      if (out->best) out->best[e] = -1;
      if (out->gamma) out->gamma[e] = nan;
      if (out->active) out->active[e] = -1;
    }
    for (int64_t g = 0; g < G; ++g) {
      if (out->n_feasible) out->n_feasible[g] = 0;
      if (out->n_attained) out->n_attained[g] = 0;
    }
    return MPCT_OK;
  }
  CallStage cs{"mpct_goal_attain", "goal-attainment staging", "costs, goals and weights", "goal-attainment results"};
  const size_t rows = (size_t)G * n_best;
  const int s_costs = cs.in(costs, (size_t)C * k * sizeof(double));
  const int s_goals = cs.in(goals, (size_t)G * k * sizeof(double)), s_w = cs.in(weights, (size_t)G * k * sizeof(double));
  const int s_best = cs.out(out->best, rows * sizeof(int32_t)), s_gamma = cs.out(out->gamma, rows * sizeof(double)),
            s_active = cs.out(out->active, rows * sizeof(int32_t)), s_nf = cs.out(out->n_feasible, (size_t)G * sizeof(int32_t)),
            s_na = cs.out(out->n_attained, (size_t)G * sizeof(int32_t)), s_wins = cs.out(out->wins, (size_t)C * sizeof(int32_t));
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    mpct_goal_result d{};
    d.best = cs.at<int32_t>(s_best);
    d.gamma = cs.at<double>(s_gamma);
    d.active = cs.at<int32_t>(s_active);
    d.n_feasible = cs.at<int32_t>(s_nf);
    d.n_attained = cs.at<int32_t>(s_na);
    d.wins = cs.at<int32_t>(s_wins);
    rc = goal_launch(cs.at<double>(s_costs), C, k, cs.at<double>(s_goals), cs.at<double>(s_w), G, n_best, &d, cs.st);
  }
  return cs.close(rc);
}

// ---- Hypervolume of a front and per-member contributions (hypervolume.hip).  The argument checks of both
// entries, in the order include/mpct.h states, before any device is touched; nothing is dereferenced
// (mpct_hv_select puts its n_pick checks between the sizes and the pointers)
static int hv_check_sizes(int64_t C, int32_t k, int64_t M, int64_t N) {
  if (k < 1 || k > MPCT_PARETO_MAX_OBJ) return fail(MPCT_EINVAL, "k must be 1 .. MPCT_PARETO_MAX_OBJ");
  if (C < 0 || M < 0) return fail(MPCT_EINVAL, "C < 0 or M < 0");
  if (C > MPCT_PARETO_MAX_C || M > MPCT_PARETO_MAX_C) return fail(MPCT_ERANGE, "C or M exceeds MPCT_PARETO_MAX_C");
  if (N > MPCT_HV_MAX_SAMPLES) return fail(MPCT_ERANGE, "n_samples exceeds MPCT_HV_MAX_SAMPLES");
  if (N < 1) return fail(MPCT_EINVAL, "n_samples < 1");
  return MPCT_OK;
}

static int hv_check_inputs(const double* costs, int64_t C, const int32_t* members, int64_t M, const double* lo,
                           const double* ref) {
  if (M > 0 && !costs) return fail(MPCT_EINVAL, "costs is NULL");
  if (!members && M != C) return fail(MPCT_EINVAL, "members is NULL: M must equal C");
  if (!lo || !ref) return fail(MPCT_EINVAL, "lo or ref is NULL");
  return MPCT_OK;
}

static int hv_check(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                    const double* ref, int64_t N, const mpct_hv_result* out) {
  int rc = hv_check_sizes(C, k, M, N);
  if (rc == MPCT_OK) rc = hv_check_inputs(costs, C, members, M, lo, ref);
  if (rc) return rc;
  if (!out || !(out->n_covered || out->excl || out->depth_hist || out->hv))
    return fail(MPCT_EINVAL, "no output pointer in mpct_hv_result");
  return MPCT_OK;
}

// the checks that read the caller's arrays, which only the host entries can make: the box and the entries of
// members (mpct_hypervolume, mpct_hv_select, mpct_hypervolume_exact).  *vol, where asked for: the box volume
static int hv_check_box_members(int32_t k, const double* lo, const double* ref, const int32_t* members, int64_t M, int64_t C,
                                double* vol = nullptr) {
  double v = 1.0;
  for (int j = 0; j < k; ++j) {
    if (!std::isfinite(lo[j]) || !std::isfinite(ref[j]) || !(lo[j] < ref[j]))
      return fail(MPCT_EINVAL, "the box needs finite lo and ref with lo[j] < ref[j]");
    v *= ref[j] - lo[j];
  }
  for (int64_t m = 0; members && m < M; ++m)
    if (members[m] < -1 || members[m] >= C) return fail(MPCT_EINVAL, "an entry of members is below -1 or >= C");
  if (vol) *vol = v;
  return MPCT_OK;
}

// tile length (128 or 256; 0: the default) and the largest grid in workgroups (0: the default) of
// hv_count_kernel.  A test hook, not part of include/mpct.h: the tests reach the multi-tile and striding
// paths at small shapes with it, tools/hv_bench.py runs its A/B with it
static int32_t g_hv_tile = 0, g_hv_blocks = 0;
extern "C" int32_t mpct_internal_hv_tuned(int32_t tile, int32_t max_blocks) {
  if ((tile != 0 && tile != 128 && tile != 256) || max_blocks < 0) return fail(MPCT_EINVAL, "tile must be 0, 128 or 256, max_blocks >= 0");
  g_hv_tile = tile;
  g_hv_blocks = max_blocks;
  return MPCT_OK;
}

static int32_t hv_launch(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                         const double* ref, int64_t N, uint64_t seed, const mpct_hv_result* out, hipStream_t stream) {
  std::string err;
  const HvOut ho{reinterpret_cast<long long*>(out->n_covered), reinterpret_cast<long long*>(out->excl),
                 reinterpret_cast<long long*>(out->depth_hist), out->hv};
  return launch_rc(hypervolume_device(costs, C, k, members, M, lo, ref, N, seed, ho, stream, &err, g_hv_tile, g_hv_blocks), err);
}

extern "C" int32_t mpct_hypervolume_device(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                           const double* lo, const double* ref, int64_t n_samples, uint64_t seed,
                                           const mpct_hv_result* out, void* stream) {
  const int rc = hv_check(costs, C, k, members, M, lo, ref, n_samples, out);
  if (rc) return rc;
  return hv_launch(costs, C, k, members, M, lo, ref, n_samples, seed, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_hypervolume(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                    const double* lo, const double* ref, int64_t n_samples, uint64_t seed, int32_t device,
                                    const mpct_hv_result* out) {
  int rc = hv_check(costs, C, k, members, M, lo, ref, n_samples, out);
  if (rc) return rc;
  double vol = 1.0;
  rc = hv_check_box_members(k, lo, ref, members, M, C, &vol);
  if (rc) return rc;
  if (M == 0) {  // nothing to stage
    if (out->n_covered) out->n_covered[0] = 0;
    for (int b = 0; out->depth_hist && b < MPCT_HV_BINS; ++b) out->depth_hist[b] = b ? 0 : n_samples;
    if (out->hv) out->hv[0] = (0.0 / (double)n_samples) * vol;
    return MPCT_OK;
  }
  CallStage cs{"mpct_hypervolume", "hypervolume staging", "hypervolume inputs", "hypervolume results"};
  const int s_costs = cs.in(costs, (size_t)C * k * sizeof(double)), s_mem = cs.in(members, (size_t)M * sizeof(int32_t)),
            s_lo = cs.in(lo, (size_t)k * sizeof(double)), s_ref = cs.in(ref, (size_t)k * sizeof(double));
  const int s_excl = cs.out(out->excl, (size_t)M * sizeof(int64_t)), s_ncov = cs.out(out->n_covered, sizeof(int64_t)),
            s_hist = cs.out(out->depth_hist, MPCT_HV_BINS * sizeof(int64_t)), s_hv = cs.out(out->hv, sizeof(double));
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    mpct_hv_result d{};
    d.n_covered = cs.at<int64_t>(s_ncov);
    d.excl = cs.at<int64_t>(s_excl);
    d.depth_hist = cs.at<int64_t>(s_hist);
    d.hv = cs.at<double>(s_hv);
    rc = hv_launch(cs.at<double>(s_costs), C, k, cs.at<int32_t>(s_mem), M, cs.at<double>(s_lo), cs.at<double>(s_ref), n_samples,
                   seed, &d, cs.st);
  }
  return cs.close(rc);
}

// ---- Greedy hypervolume subset selection (hv_select.hip).  The argument checks of both entries, in the
// order include/mpct.h states, before any device is touched; nothing is dereferenced
static int hvsel_check(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                       const double* ref, int64_t N, int32_t n_pick, const mpct_hv_select_result* out) {
  int rc = hv_check_sizes(C, k, M, N);
  if (rc) return rc;
  if (n_pick < 1) return fail(MPCT_EINVAL, "n_pick < 1");
  if (n_pick > MPCT_HVSEL_MAX_PICKS) return fail(MPCT_ERANGE, "n_pick exceeds MPCT_HVSEL_MAX_PICKS");
  rc = hv_check_inputs(costs, C, members, M, lo, ref);
  if (rc) return rc;
  if (!out || !(out->n_picked || out->pos || out->index || out->gain || out->covered || out->hv || out->ties ||
                out->n_covered_all))
    return fail(MPCT_EINVAL, "no output pointer in mpct_hv_select_result");
  return MPCT_OK;
}

// tile length (128 or 256; 0: the default) and the largest grid in workgroups (0: the default) of
// hvsel_gain_kernel, as mpct_internal_hv_tuned; and the tools' round timing (a host array of n floats that the
// NEXT call alone fills, waiting for its stream, when its n_pick <= n; NULL: off).  Test and tool hooks, not
// part of include/mpct.h
static int32_t g_hvsel_tile = 0, g_hvsel_blocks = 0;
static float* g_hvsel_round_ms = nullptr;
static int32_t g_hvsel_round_n = 0;
extern "C" int32_t mpct_internal_hvsel_tuned(int32_t tile, int32_t max_blocks) {
  if ((tile != 0 && tile != 128 && tile != 256) || max_blocks < 0) return fail(MPCT_EINVAL, "tile must be 0, 128 or 256, max_blocks >= 0");
  g_hvsel_tile = tile;
  g_hvsel_blocks = max_blocks;
  return MPCT_OK;
}
extern "C" int32_t mpct_internal_hvsel_round_ms(float* ms, int32_t n) {
  if (ms && n < 1) return fail(MPCT_EINVAL, "the round-time array needs n >= 1");
  g_hvsel_round_ms = ms;
  g_hvsel_round_n = ms ? n : 0;
  return MPCT_OK;
}

static int32_t hvsel_launch(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                            const double* ref, int64_t N, uint64_t seed, int32_t n_pick, const mpct_hv_select_result* out,
                            hipStream_t stream) {
  std::string err;
  const HvSelOut so{reinterpret_cast<long long*>(out->n_picked), out->pos, out->index, reinterpret_cast<long long*>(out->gain),
                    reinterpret_cast<long long*>(out->covered), out->hv, out->ties,
                    reinterpret_cast<long long*>(out->n_covered_all)};
  float* round_ms = n_pick <= g_hvsel_round_n ? g_hvsel_round_ms : nullptr;  // never past the tool's array
  g_hvsel_round_ms = nullptr;                                                // one call only
  g_hvsel_round_n = 0;
  return launch_rc(hv_select_device(costs, C, k, members, M, lo, ref, N, seed, n_pick, so, stream, &err, g_hvsel_tile,
                                    g_hvsel_blocks, round_ms),
                   err);
}

extern "C" int32_t mpct_hv_select_device(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                         const double* lo, const double* ref, int64_t n_samples, uint64_t seed,
                                         int32_t n_pick, const mpct_hv_select_result* out, void* stream) {
  const int rc = hvsel_check(costs, C, k, members, M, lo, ref, n_samples, n_pick, out);
  if (rc) return rc;
  return hvsel_launch(costs, C, k, members, M, lo, ref, n_samples, seed, n_pick, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_hv_select(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                  const double* lo, const double* ref, int64_t n_samples, uint64_t seed, int32_t n_pick,
                                  int32_t device, const mpct_hv_select_result* out) {
  int rc = hvsel_check(costs, C, k, members, M, lo, ref, n_samples, n_pick, out);
  if (rc) return rc;
  double vol = 1.0;
  rc = hv_check_box_members(k, lo, ref, members, M, C, &vol);
  if (rc) return rc;
  if (M == 0) {  // nothing to stage: the end-of-selection fill from slot 0
    if (out->n_picked) out->n_picked[0] = 0;
    if (out->n_covered_all) out->n_covered_all[0] = 0;
    for (int r = 0; r < n_pick; ++r) {
      if (out->pos) out->pos[r] = -1;
      if (out->index) out->index[r] = -1;
      if (out->gain) out->gain[r] = 0;
      if (out->covered) out->covered[r] = 0;
      if (out->hv) out->hv[r] = (0.0 / (double)n_samples) * vol;
      if (out->ties) out->ties[r] = 0;
    }
    return MPCT_OK;
  }
  CallStage cs{"mpct_hv_select", "hv_select staging", "hv_select inputs", "hv_select results"};
  const size_t b4 = (size_t)n_pick * sizeof(int32_t), b8 = (size_t)n_pick * sizeof(int64_t);
  const int s_costs = cs.in(costs, (size_t)C * k * sizeof(double)), s_mem = cs.in(members, (size_t)M * sizeof(int32_t)),
            s_lo = cs.in(lo, (size_t)k * sizeof(double)), s_ref = cs.in(ref, (size_t)k * sizeof(double));
  const int s_pos = cs.out(out->pos, b4), s_index = cs.out(out->index, b4), s_ties = cs.out(out->ties, b4),
            s_gain = cs.out(out->gain, b8), s_covered = cs.out(out->covered, b8), s_hv = cs.out(out->hv, b8),
            s_npicked = cs.out(out->n_picked, sizeof(int64_t)), s_nall = cs.out(out->n_covered_all, sizeof(int64_t));
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    mpct_hv_select_result d{};
    d.n_picked = cs.at<int64_t>(s_npicked);
    d.pos = cs.at<int32_t>(s_pos);
    d.index = cs.at<int32_t>(s_index);
    d.gain = cs.at<int64_t>(s_gain);
    d.covered = cs.at<int64_t>(s_covered);
    d.hv = cs.at<double>(s_hv);
    d.ties = cs.at<int32_t>(s_ties);
    d.n_covered_all = cs.at<int64_t>(s_nall);
    rc = hvsel_launch(cs.at<double>(s_costs), C, k, cs.at<int32_t>(s_mem), M, cs.at<double>(s_lo), cs.at<double>(s_ref),
                      n_samples, seed, n_pick, &d, cs.st);
  }
  return cs.close(rc);
}

// ---- Exact hypervolume and contributions for k <= 3 (hypervolume_exact.hip).  The argument checks of both
// entries, in the order include/mpct.h states, before any device is touched; nothing is dereferenced
static int hvx_check(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                     const double* ref, const mpct_hvx_result* out) {
  if (k < 1) return fail(MPCT_EINVAL, "k < 1");
  if (k > MPCT_HVX_MAX_OBJ) return fail(MPCT_ERANGE, "k exceeds MPCT_HVX_MAX_OBJ (the exact hypervolume serves k <= 3)");
  if (C < 0 || M < 0) return fail(MPCT_EINVAL, "C < 0 or M < 0");
  if (C > MPCT_PARETO_MAX_C) return fail(MPCT_ERANGE, "C exceeds MPCT_PARETO_MAX_C");
  if (M > MPCT_HVX_MAX_M) return fail(MPCT_ERANGE, "M exceeds MPCT_HVX_MAX_M");
  const int rc = hv_check_inputs(costs, C, members, M, lo, ref);
  if (rc) return rc;
  if (!out || !(out->hv || out->excl || out->n_active)) return fail(MPCT_EINVAL, "no output pointer in mpct_hvx_result");
  return MPCT_OK;
}

static int32_t hvx_launch(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M, const double* lo,
                          const double* ref, const mpct_hvx_result* out, hipStream_t stream) {
  std::string err;
  const HvxOut ho{out->hv, out->excl, reinterpret_cast<long long*>(out->n_active)};
  return launch_rc(hypervolume_exact_device(costs, C, k, members, M, lo, ref, ho, stream, &err), err);
}

extern "C" int32_t mpct_hypervolume_exact_device(const double* costs, int64_t C, int32_t k, const int32_t* members,
                                                 int64_t M, const double* lo, const double* ref,
                                                 const mpct_hvx_result* out, void* stream) {
  const int rc = hvx_check(costs, C, k, members, M, lo, ref, out);
  if (rc) return rc;
  return hvx_launch(costs, C, k, members, M, lo, ref, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_hypervolume_exact(const double* costs, int64_t C, int32_t k, const int32_t* members, int64_t M,
                                          const double* lo, const double* ref, int32_t device,
                                          const mpct_hvx_result* out) {
  int rc = hvx_check(costs, C, k, members, M, lo, ref, out);
  if (rc) return rc;
  rc = hv_check_box_members(k, lo, ref, members, M, C);
  if (rc) return rc;
  if (M == 0) {  // nothing to stage
    if (out->hv) out->hv[0] = 0.0;
    if (out->n_active) out->n_active[0] = 0;
    return MPCT_OK;
  }
  CallStage cs{"mpct_hypervolume_exact", "hypervolume_exact staging", "hypervolume_exact inputs", "hypervolume_exact results"};
  const int s_costs = cs.in(costs, (size_t)C * k * sizeof(double)), s_mem = cs.in(members, (size_t)M * sizeof(int32_t)),
            s_lo = cs.in(lo, (size_t)k * sizeof(double)), s_ref = cs.in(ref, (size_t)k * sizeof(double));
  const int s_excl = cs.out(out->excl, (size_t)M * sizeof(double)), s_hv = cs.out(out->hv, sizeof(double)),
            s_nactive = cs.out(out->n_active, sizeof(int64_t));
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    mpct_hvx_result d{};
    d.hv = cs.at<double>(s_hv);
    d.excl = cs.at<double>(s_excl);
    d.n_active = cs.at<int64_t>(s_nactive);
    rc = hvx_launch(cs.at<double>(s_costs), C, k, cs.at<int32_t>(s_mem), M, cs.at<double>(s_lo), cs.at<double>(s_ref), &d, cs.st);
  }
  return cs.close(rc);
}

// Host-pointer staging of one call on the context's own stream, shared by the scenario-taking host
// entries: the candidates go into the grow-only scratch blob, the signals r | v through
// the context's signal cache, the results come back from slots of the same blob.  An entry
// declares each result field once, before upload(): keep() for a field the launch always writes
// (or writes when `on`), which is copied back where the caller gave a pointer, want() for a field
// that exists only where the caller asked for it (CallStage's rule: no pointer, no bytes, and the
// launch gets NULL).  Slots are numbered from 0 in the order they are declared.  After upload()
// `dev` is the device-side batch and at<T>(slot) a field's device address; the entry launches on
// `st` and finish()es, which enqueues the D2H copy of every declared field and waits.
namespace {
struct HostStage {
  DevCtx* cx;
  hipStream_t st;
  int my, nu;
  size_t off = 0;
  size_t o_N2, o_Nu, o_d, o_l;  // the candidates' slots
  Batch dev{};                  // the candidates and signals on the device, after upload()
  static constexpr int kMaxSlots = 29;  // mpct_eval_robust_envelope, the widest entry: a base of 5, two records of 9, two spreads of 3
  struct Slot {
    void* host;  // NULL: nothing to copy back
    size_t bytes, off;
    bool on;  // false: nothing reserved, its device address is NULL
  } slots[kMaxSlots] = {};
  int nslots = 0;

  HostStage(const mpct_scenario* s, DevCtx* c, int64_t C) : cx(c), st(c->stream), my(s->my), nu(s->nu) {
    o_N2 = reserve(C * 4), o_Nu = reserve(C * 4), o_d = reserve(C * my * 8), o_l = reserve(C * nu * 8);
  }
  // reserve 256-B-aligned bytes of the blob; the address holds after upload()
  size_t reserve(size_t bytes) {
    const size_t o = off;
    off += (bytes + 255) & ~(size_t)255;
    return o;
  }
  int keep(void* host, size_t bytes, bool on = true) {
    assert(nslots < kMaxSlots);
    slots[nslots] = Slot{host, bytes, on ? reserve(bytes) : 0, on};
    return nslots++;
  }
  int want(void* host, size_t bytes) { return keep(host, bytes, host != nullptr); }
  template <class T>
  T* at(int i) const { return slots[i].on ? reinterpret_cast<T*>(static_cast<char*>(cx->dscratch) + slots[i].off) : nullptr; }
  template <class T>
  void bind(int i, T*& p) const { p = at<T>(i); }

  // `*buf` holds at least `bytes`: a regrow waits for the stream's work on the old buffer first
  int ensure(void** buf, size_t* have, size_t bytes, const char* what) {
    if (bytes <= *have) return MPCT_OK;
    if (*buf) {
      (void)hipStreamSynchronize(st);
      (void)hipFree(*buf);
    }
    *buf = nullptr;
    *have = 0;
    if (hipMalloc(buf, bytes) != hipSuccess) return fail(MPCT_ENOMEM, std::string("hipMalloc(") + what + ") failed");
    *have = bytes;
    return MPCT_OK;
  }

  // every slot reserved: size the blob and enqueue the H2D copies of the candidates and signals
  int upload(const mpct_scenario* s, const Batch& h) {
    int rc = ensure(&cx->dscratch, &cx->dscratch_bytes, off, "scratch");
    if (rc) return rc;
    // signals r | v: uploaded only when they differ from what the context's signal buffer holds
    const char *hr = reinterpret_cast<const char*>(h.r), *hv = reinterpret_cast<const char*>(h.v);
    const size_t rb = (size_t)h.nref * my * s->nit * 8, vb = (size_t)h.nref * (s->nd + s->nq) * s->nit * 8;
    const bool same_sig = cx->sig_host.size() == rb + vb && std::memcmp(cx->sig_host.data(), hr, rb) == 0 &&
                          (vb == 0 || std::memcmp(cx->sig_host.data() + rb, hv, vb) == 0);
    if (!same_sig) {
      if (rb + vb > cx->dsig_bytes) cx->sig_host.clear();
      rc = ensure(&cx->dsig, &cx->dsig_bytes, rb + vb, "signals");
      if (rc) return rc;
      cx->sig_host.assign(hr, hr + rb);
      if (vb) cx->sig_host.insert(cx->sig_host.end(), hv, hv + vb);
    }
    char* blob = static_cast<char*>(cx->dscratch);
    const char* sig = static_cast<const char*>(cx->dsig);
    dev = Batch{h.C, reinterpret_cast<int32_t*>(blob + o_N2), reinterpret_cast<int32_t*>(blob + o_Nu),
                reinterpret_cast<double*>(blob + o_d), reinterpret_cast<double*>(blob + o_l), h.nref,
                reinterpret_cast<const double*>(sig), vb ? reinterpret_cast<const double*>(sig + rb) : nullptr};
    auto h2d = [&](const void* dst, const void* p, size_t bytes) {
      return bytes == 0 || hipMemcpyAsync(const_cast<void*>(dst), p, bytes, hipMemcpyHostToDevice, st) == hipSuccess;
    };
    // the signals are copied from the context's own host copy (the caller's buffers may change
    // after the call returns; an earlier launch reading dsig is ordered before this copy on st)
    if (!h2d(dev.N2, h.N2, h.C * 4) || !h2d(dev.Nu, h.Nu, h.C * 4) || !h2d(dev.delta, h.delta, h.C * my * 8) ||
        !h2d(dev.lambda, h.lambda, h.C * nu * 8) || (!same_sig && !h2d(cx->dsig, cx->sig_host.data(), rb + vb))) {
      // copies enqueued before the failing one may still read the caller's buffers
      (void)hipStreamSynchronize(st);
      cx->sig_host.clear();
      return fail(MPCT_EDEVICE, "hipMemcpyAsync(inputs) failed");
    }
    return MPCT_OK;
  }

  // a failed launch: nothing of this call stays in flight
  int abandon(int rc) {
    (void)hipStreamSynchronize(st);
    return rc;
  }
  // enqueue the D2H copy of every declared field the caller gave a pointer for, then wait for the stream
  int finish() {
    bool fetched = true;
    for (int i = 0; i < nslots; ++i) {
      const Slot& f = slots[i];
      if (f.on && f.host && f.bytes)
        fetched = hipMemcpyAsync(f.host, at<char>(i), f.bytes, hipMemcpyDeviceToHost, st) == hipSuccess && fetched;
    }
    const hipError_t se = hipStreamSynchronize(st);
    if (se != hipSuccess) return fail(MPCT_EDEVICE, std::string("kernel execution failed: ") + hipGetErrorString(se));
    if (!fetched) return fail(MPCT_EDEVICE, "hipMemcpyAsync(results) failed");
    return MPCT_OK;
  }
};
}  // namespace

// the ten fields of an mpct_result in the struct's order, each with its elements per simulation
template <class R, class F>
static void each_field(R& res, int64_t my, int64_t nu, int64_t nit, F f) {
  f(res.J1, my);
  f(res.j21, my);
  f(res.j22, my);
  f(res.Jnu, nu);
  f(res.status, 1);
  f(res.qp_iters, 1);
  f(res.y, my * nit);
  f(res.u, nu * nit);
  f(res.ys, my * nit);
  f(res.uopt, nu * nit);
}

// host buffers in, host buffers out, on the context's own stream: H2D of the candidates and
// signals, the launch, D2H of the results, then a wait on that stream only
static int eval_host(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, mpct_result* out) {
  if (hipSetDevice(cx->dev) != hipSuccess) return fail(MPCT_EDEVICE, "hipSetDevice failed");
  if (b.C == 0) return MPCT_OK;
  const size_t S = (size_t)(b.C * b.nref);
  const bool traj = opts && opts->want_traj;
  const bool ol = traj && opts->open_loop;
  HostStage hs(s, cx, b.C);
  // slots 0..9: the six cost fields always live on the device, y | u with want_traj, ys | uopt with open_loop too
  int k = 0;
  each_field(*out, s->my, s->nu, s->nit, [&](auto* host, int64_t w) {
    hs.keep(host, S * w * sizeof(*host), k < 6 || (k < 8 ? traj : ol));
    ++k;
  });
  int rc = hs.upload(s, b);
  if (rc) return rc;
  mpct_result dres{};
  k = 0;
  each_field(dres, s->my, s->nu, s->nit, [&](auto*& dev, int64_t) { hs.bind(k++, dev); });
  rc = launch_batch(s, cx, hs.dev, opts, &dres, hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

extern "C" int32_t mpct_eval_batch(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                   const double* delta, const double* lambda, int32_t nref, const double* r,
                                   const double* v, const mpct_opts* opts, mpct_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_args(s, b, opts, out);
  if (rc) return rc;
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return eval_host(s, cx, b, opts, out);
}

extern "C" int64_t mpct_shard_candidates(int64_t C, int32_t ndev, int32_t k, int64_t* idx, int64_t cap) {
  if (C < 0 || ndev < 1 || k < 0 || k >= ndev) return fail(MPCT_EINVAL, "bad shard arguments");
  const int64_t n = C > k ? (C - k + ndev - 1) / ndev : 0;
  if (idx)
    for (int64_t j = 0; j < std::min(n, cap); ++j) idx[j] = k + j * ndev;
  return n;
}

// copy `width` elements per simulation between the caller's order and a shard's packed order:
// simulation s = c*nref + q of candidate c = k + j*ndev <-> packed row j*nref + q
template <class T>
static void strided_copy(T* caller, T* packed, int64_t n, int32_t ndev, int32_t k, int32_t nref, int64_t width,
                         bool to_caller) {
  if (!caller || !packed) return;
  for (int64_t j = 0; j < n; ++j) {
    T* a = caller + (k + j * ndev) * (int64_t)nref * width;
    T* b = packed + j * (int64_t)nref * width;
    const size_t bytes = sizeof(T) * (size_t)nref * (size_t)width;
    if (to_caller)
      std::memcpy(a, b, bytes);
    else
      std::memcpy(b, a, bytes);
  }
}

extern "C" int32_t mpct_eval_batch_multi(mpct_scenario* s, int32_t ndev, const int32_t* devices, int64_t C,
                                         const int32_t* N2, const int32_t* Nu, const double* delta,
                                         const double* lambda, int32_t nref, const double* r, const double* v,
                                         const mpct_opts* opts, mpct_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_args(s, b, opts, out, ndev >= 1 && ndev <= 64 && devices);
  if (rc) return rc;
  int cur = -1, cnt = 0;
  if (hipGetDevice(&cur) != hipSuccess || hipGetDeviceCount(&cnt) != hipSuccess || cnt == 0)
    return fail(MPCT_EDEVICE, "hipGetDevice failed (no GPU?)");
  // every ordinal is checked before any context exists or any device is made current
  for (int k = 0; k < ndev; ++k)
    if (devices[k] < 0 || devices[k] >= cnt) return fail(MPCT_EINVAL, "device ordinal out of range");
  // contexts (table uploads) serially on this thread, before any worker starts; a device listed
  // again gets a further context of its own
  std::vector<DevCtx*> cxs(ndev, nullptr);
  for (int k = 0; k < ndev; ++k) {
    int occ = 0;
    for (int j = 0; j < k; ++j) occ += devices[j] == devices[k];
    rc = device_ctx(s, devices[k], &cxs[k], occ);
    if (rc) {
      (void)hipSetDevice(cur);
      return rc;
    }
  }
  const int my = s->my, nu = s->nu, nit = s->nit;
  std::vector<int> rcs(ndev, MPCT_OK);
  std::vector<std::string> errs(ndev);
  auto shard = [&](int k) {
    const int64_t n = mpct_shard_candidates(C, ndev, k, nullptr, 0);
    if (n <= 0) {
      rcs[k] = hipSetDevice(cxs[k]->dev) == hipSuccess ? MPCT_OK : MPCT_EDEVICE;
      return;
    }
    if (ndev == 1) {  // the identity split: no gather / scatter
      rcs[k] = eval_host(s, cxs[k], b, opts, out);
      if (rcs[k]) errs[k] = g_err;
      return;
    }
    // gather this slot's candidates (k, k+ndev, ...) and give it a packed buffer per field the caller asked for
    std::vector<int32_t> n2(n), nuv(n);
    std::vector<double> dl((size_t)n * my), lm((size_t)n * nu);
    strided_copy(const_cast<int32_t*>(N2), n2.data(), n, ndev, k, 1, 1, false);
    strided_copy(const_cast<int32_t*>(Nu), nuv.data(), n, ndev, k, 1, 1, false);
    strided_copy(const_cast<double*>(delta), dl.data(), n, ndev, k, 1, my, false);
    strided_copy(const_cast<double*>(lambda), lm.data(), n, ndev, k, 1, nu, false);
    std::vector<std::vector<char>> packed(10);
    mpct_result o = *out;
    int f = 0;
    each_field(o, my, nu, nit, [&](auto*& p, int64_t w) {
      std::vector<char>& buf = packed[f++];
      if (!p) return;
      buf.resize(sizeof(*p) * (size_t)(n * nref * w));
      p = reinterpret_cast<std::remove_reference_t<decltype(p)>>(buf.data());
    });
    rcs[k] = eval_host(s, cxs[k], Batch{n, n2.data(), nuv.data(), dl.data(), lm.data(), nref, r, v}, opts, &o);
    if (rcs[k]) {
      errs[k] = g_err;  // g_err is thread-local: carry it to the caller
      return;
    }
    // scatter into the caller's order (slots write disjoint candidates)
    f = 0;
    each_field(*out, my, nu, nit, [&](auto* p, int64_t w) {
      strided_copy(p, reinterpret_cast<decltype(p)>(packed[f++].data()), n, ndev, k, nref, w, true);
    });
  };
  if (ndev == 1) {
    shard(0);
  } else {
    std::vector<std::thread> th;
    for (int k = 1; k < ndev; ++k) th.emplace_back(shard, k);
    shard(0);
    for (auto& t : th) t.join();
  }
  (void)hipSetDevice(cur);
  for (int k = 0; k < ndev; ++k)
    if (rcs[k]) return fail(rcs[k], "device " + std::to_string(devices[k]) + ": " + errs[k]);
  return MPCT_OK;
}

// ------------------------------------------------------------------------------------------
// robust scoring over plant draws (include/mpct.h)

// the argument checks of the robust entries, on top of check_args
static int check_robust(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                        const mpct_robust_result* out, bool need_out = true) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (opts && (opts->open_loop || opts->want_traj))
    return fail(MPCT_EINVAL, "robust scoring is cost-only: open_loop and want_traj must be 0");
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: robust scoring needs at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  if (need_out) {
    if (!out) return fail(MPCT_EINVAL, "null result");
    if (!out->mean && !out->worst && !out->n_failed && !out->worst_draw && !out->status && !out->J1)
      return fail(MPCT_EINVAL, "every output pointer of the robust result is NULL");
  }
  const mpct_result any{};
  return check_args(s, b, opts, &any);
}

// the tail statistics a robust call adds (mpct_eval_robust_tail): the levels on the host, the
// outputs on the device
struct TailReq {
  int nlev;
  const double* levels;
  TailOut out;
};

// the argument checks the tail entries add, in the header's order; then check_robust's, then the
// draw cap.  Nothing here touches a device
static int check_tail(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts, int32_t nlev,
                      const double* levels, const mpct_robust_result* out, const mpct_robust_tail* tail) {
  if (nlev < 1 || nlev > MPCT_TAIL_MAX_LEVELS) return fail(MPCT_EINVAL, "nlev must be 1 .. MPCT_TAIL_MAX_LEVELS (8)");
  if (!levels) return fail(MPCT_EINVAL, "null levels");
  for (int j = 0; j < nlev; ++j)
    if (!(levels[j] > 0.0 && levels[j] <= 1.0)) return fail(MPCT_EINVAL, "every level must lie in (0, 1], not NaN");
  const bool any_tail = tail && (tail->quantile || tail->cvar || tail->q_draw);
  const bool any_out = out && (out->mean || out->worst || out->n_failed || out->worst_draw || out->status || out->J1);
  if (!any_tail && !any_out) return fail(MPCT_EINVAL, "every output pointer of the robust result and of the tail is NULL");
  const int rc = check_robust(s, b, j_bound, opts, out, false);
  if (rc) return rc;
  if (b.nref > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "nref > MPCT_TAIL_MAX_DRAWS (4096): the tail kernel's LDS holds no more draws");
  return MPCT_OK;
}

// enqueue one robust batch with device pointers on `stream` (ctx's device is current); with `tail`,
// robust_tail_kernel follows on the same stream, on the J1 sample of the same launch
static int launch_robust(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                         const mpct_robust_result* out, hipStream_t stream, const TailReq* tail = nullptr) {
  if (b.C == 0) return MPCT_OK;
  const int64_t C = b.C;
  const int32_t nref = b.nref;
  const double bound = j_bound == 0.0 ? kRobustDefaultBound : j_bound;
  const RobustOut ro{out->mean, out->worst, out->n_failed, out->worst_draw, out->status};
  const int64_t S = C * nref;
  std::string err;
  int rc;
  char* scr = nullptr;
  if (dtc_robust_eligible(cx->ds, nref)) {
    if (cx->ncu == 0 &&
        (hipDeviceGetAttribute(&cx->ncu, hipDeviceAttributeMultiprocessorCount, cx->dev) != hipSuccess || cx->ncu < 1))
      return fail(MPCT_EDEVICE, "hipDeviceGetAttribute(MultiprocessorCount) failed");
    // the candidate lists, and the J1 sample where a tail is asked for and the caller keeps none
    const size_t lb = (sizeof(int) * (size_t)(2 * C + 2) + 255) & ~(size_t)255;
    const bool own_j1 = tail && !out->J1;
    rc = cx->robust.acquire(own_j1 ? lb + (size_t)S * s->my * 8 : sizeof(int) * (size_t)(2 * C + 2), stream,
                            "robust scratch", &scr);
    if (rc) return rc;
    double* j1 = own_j1 ? reinterpret_cast<double*>(scr + lb) : out->J1;
    const int* perm = nullptr;
    rc = order_candidates(kOrderGpc, s->my, s->nu, C, b.N2, b.Nu, b.delta, b.lambda, cx->order, &perm, stream, &err,
                          &cx->ds, nref, b.r);
    if (rc == 0)
      rc = launch_dtc_robust(cx->ds, C, nref, b.N2, b.Nu, b.delta, b.lambda, b.r, b.v, perm, reinterpret_cast<int*>(scr),
                             bound, ro, j1, cx->ncu, &cx->fan, stream, &err);
    if (perm) order_mark_used(cx->order, stream);
    // the fused kernel keeps no per-simulation status: a failed draw of it has a non-finite J1, and a
    // candidate that was never simulated an all-NaN sample (robust_classify_kernel)
    if (rc == 0 && tail)
      rc = launch_robust_tail(C, nref, s->my, bound, j1, nullptr, tail->nlev, tail->levels, tail->out, stream, &err);
    if (rc) return fail(rc, err);
  } else {
    // the per-simulation instance, unchanged, into the caller's J1 or the scenario's scratch
    const size_t jb = out->J1 ? 0 : ((size_t)S * s->my * 8 + 255) & ~(size_t)255;
    rc = cx->robust.acquire(jb + (size_t)S * 4, stream, "robust scratch", &scr);
    if (rc) return rc;
    mpct_result per{};
    per.J1 = out->J1 ? out->J1 : reinterpret_cast<double*>(scr);
    per.status = reinterpret_cast<int32_t*>(scr + jb);
    rc = launch_batch(s, cx, b, opts, &per, stream);
    if (rc) return rc;
    rc = launch_robust_reduce(C, nref, s->my, bound, per.J1, per.status, ro, stream, &err);
    if (rc == 0 && tail)
      rc = launch_robust_tail(C, nref, s->my, bound, per.J1, per.status, tail->nlev, tail->levels, tail->out, stream,
                              &err);
    if (rc) return fail(rc, err);
  }
  cx->robust.mark(stream);
  return MPCT_OK;
}

extern "C" int32_t mpct_eval_robust_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                           const double* delta, const double* lambda, int32_t nref,
                                           const double* r, const double* v, double j_bound, const mpct_opts* opts,
                                           mpct_robust_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_robust(s, b, j_bound, opts, out);
  if (rc) return rc;
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_robust(s, cx, b, j_bound, opts, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_robust_tail_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                const double* delta, const double* lambda, int32_t nref,
                                                const double* r, const double* v, double j_bound,
                                                const mpct_opts* opts, int32_t nlev, const double* levels,
                                                mpct_robust_result* out, mpct_robust_tail* tail, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_tail(s, b, j_bound, opts, nlev, levels, out, tail);
  if (rc) return rc;
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const mpct_robust_result base = out ? *out : mpct_robust_result{};
  const TailReq tq{nlev, levels, tail ? TailOut{tail->quantile, tail->cvar, tail->q_draw} : TailOut{}};
  return launch_robust(s, cx, b, j_bound, opts, &base, static_cast<hipStream_t>(stream), &tq);
}

// Test hook, deliberately not declared in include/mpct.h: robust_tail_kernel alone, on per-simulation
// records the caller supplies (device pointers, status may be NULL and is then read as 0; levels on
// the host; enqueued on `stream`).
extern "C" int32_t mpct_internal_robust_tail(int64_t C, int32_t D, int32_t my, double j_bound, const double* J1,
                                             const int32_t* status, int32_t nlev, const double* levels,
                                             double* quantile, double* cvar, int32_t* q_draw, void* stream) {
  if (C < 0 || D < 1 || my < 1 || !J1 || !(j_bound >= 0.0) || nlev < 1 || nlev > kTailMaxLevels || !levels)
    return fail(MPCT_EINVAL, "bad argument");
  for (int j = 0; j < nlev; ++j)
    if (!(levels[j] > 0.0 && levels[j] <= 1.0)) return fail(MPCT_EINVAL, "every level must lie in (0, 1], not NaN");
  if (D > kTailMaxDraws) return fail(MPCT_ERANGE, "D > MPCT_TAIL_MAX_DRAWS");
  std::string err;
  const int rc = launch_robust_tail(C, D, my, j_bound == 0.0 ? kRobustDefaultBound : j_bound, J1, status, nlev, levels,
                                    TailOut{quantile, cvar, q_draw}, static_cast<hipStream_t>(stream), &err);
  return rc ? fail(rc, err) : MPCT_OK;
}

// Test hook, deliberately not declared in include/mpct.h: the generic path's reduction alone, on
// per-simulation records the caller supplies (device pointers, enqueued on `stream`).  The tests
// reduce the fused kernel's own J1 sample with it to pin that both paths share one robust_reduce.
extern "C" int32_t mpct_internal_robust_reduce(int64_t C, int32_t D, int32_t my, double j_bound, const double* J1,
                                               const int32_t* status, const mpct_robust_result* out, void* stream) {
  if (C < 0 || D < 1 || my < 1 || !J1 || !status || !out || !(j_bound >= 0.0)) return fail(MPCT_EINVAL, "bad argument");
  const RobustOut ro{out->mean, out->worst, out->n_failed, out->worst_draw, out->status};
  std::string err;
  const int rc = launch_robust_reduce(C, D, my, j_bound == 0.0 ? kRobustDefaultBound : j_bound, J1, status, ro,
                                      static_cast<hipStream_t>(stream), &err);
  return rc ? fail(rc, err) : MPCT_OK;
}

// the host-pointer robust entries after their argument checks; nlev = 0: no tail
static int eval_robust_host(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                            const mpct_robust_result* out, int32_t nlev, const double* levels,
                            const mpct_robust_tail* tail) {
  DevCtx* cx = nullptr;
  int rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  if (b.C == 0) return MPCT_OK;
  // host buffers in, host buffers out on the context's own stream, staged as eval_host does.  The record is
  // always written on the device, the sample J1 where asked for, the tail arrays whenever there are levels
  const size_t C = (size_t)b.C, S = C * b.nref, cm = C * s->my * 8, cl = C * nlev;
  const mpct_robust_tail ht = tail ? *tail : mpct_robust_tail{};
  HostStage hs(s, cx, b.C);
  const int s_mean = hs.keep(out->mean, cm), s_worst = hs.keep(out->worst, cm), s_nf = hs.keep(out->n_failed, C * 4),
            s_wd = hs.keep(out->worst_draw, C * 4), s_st = hs.keep(out->status, C * 4), s_J1 = hs.want(out->J1, S * s->my * 8);
  const int s_q = hs.keep(ht.quantile, cl * 8, nlev > 0), s_cv = hs.keep(ht.cvar, cl * 8, nlev > 0),
            s_qd = hs.keep(ht.q_draw, cl * 4, nlev > 0);
  rc = hs.upload(s, b);
  if (rc) return rc;
  const mpct_robust_result dres{hs.at<double>(s_mean), hs.at<double>(s_worst), hs.at<int32_t>(s_nf),
                                hs.at<int32_t>(s_wd),  hs.at<int32_t>(s_st),   hs.at<double>(s_J1)};
  const TailReq tq{nlev, levels, TailOut{hs.at<double>(s_q), hs.at<double>(s_cv), hs.at<int32_t>(s_qd)}};
  rc = launch_robust(s, cx, hs.dev, j_bound, opts, &dres, hs.st, nlev ? &tq : nullptr);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

extern "C" int32_t mpct_eval_robust(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                    const double* delta, const double* lambda, int32_t nref, const double* r,
                                    const double* v, double j_bound, const mpct_opts* opts, mpct_robust_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  const int rc = check_robust(s, b, j_bound, opts, out);
  if (rc) return rc;
  return eval_robust_host(s, b, j_bound, opts, out, 0, nullptr, nullptr);
}

extern "C" int32_t mpct_eval_robust_tail(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                         const double* delta, const double* lambda, int32_t nref, const double* r,
                                         const double* v, double j_bound, const mpct_opts* opts, int32_t nlev,
                                         const double* levels, mpct_robust_result* out, mpct_robust_tail* tail) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  const int rc = check_tail(s, b, j_bound, opts, nlev, levels, out, tail);
  if (rc) return rc;
  const mpct_robust_result base = out ? *out : mpct_robust_result{};
  return eval_robust_host(s, b, j_bound, opts, &base, nlev, levels, tail);
}

// ------------------------------------------------------------------------------------------
// closed-loop performance indices per simulation (traj_indices.hip; include/mpct.h)

static IndexOut index_out(const mpct_index_result* o) {
  return IndexOut{o->iae, o->ise, o->itae, o->emax, o->t_emax, o->over, o->e_final, o->settle,
                  o->tv,  o->du2, o->dumax, o->u_lo, o->u_hi};
}

// the checks on the parameters and the record from t0 on, in the header's order (shared by the four
// entries; have_y / have_u: the trajectories behind the fields exist)
static int index_check_params(int32_t nit, const mpct_index_params* p) {
  if (p->t0 < 0 || p->t0 >= nit) return fail(MPCT_EINVAL, "t0 must be 0 .. nit-1");
  if (!(p->band_rel >= 0.0 && p->band_rel <= 1.7976931348623157e308 && p->band_abs >= 0.0 &&
        p->band_abs <= 1.7976931348623157e308))
    return fail(MPCT_EINVAL, "band_rel and band_abs must be finite and >= 0, not NaN");
  return MPCT_OK;
}

static int index_check_tail(int64_t S, int32_t my, int32_t nu, int32_t nit, const mpct_index_params* p,
                            const mpct_index_result* out, bool have_y, bool have_u) {
  const int rc = index_check_params(nit, p);
  if (rc) return rc;
  if (!out) return fail(MPCT_EINVAL, "no output pointer in mpct_index_result");
  const IndexOut io = index_out(out);
  if (!io.any_y() && !io.any_u()) return fail(MPCT_EINVAL, "no output pointer in mpct_index_result");
  if (io.any_y() && (my < 1 || (S > 0 && !have_y)))
    return fail(MPCT_EINVAL, "an output-row field needs my >= 1 and the trajectories y and r");
  if (io.any_u() && (nu < 1 || (S > 0 && !have_u)))
    return fail(MPCT_EINVAL, "an input-row field needs nu >= 1 and the trajectory u");
  if (S * (int64_t)my > kIndexMaxRows || S * (int64_t)nu > kIndexMaxRows)
    return fail(MPCT_ERANGE, "S*my or S*nu exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int index_check(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my, int32_t nu,
                       int32_t nit, const mpct_index_params* p, const mpct_index_result* out) {
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (S < 0 || my < 0 || nu < 0 || nit < 1) return fail(MPCT_EINVAL, "bad shape: S < 0, my < 0, nu < 0 or nit < 1");
  if (nref < 1) return fail(MPCT_EINVAL, "nref < 1");
  if (S % nref != 0) return fail(MPCT_EINVAL, "S must be a multiple of nref");
  return index_check_tail(S, my, nu, nit, p, out, y && r, u != nullptr);
}

static int32_t index_launch(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                            int32_t nu, int32_t nit, const mpct_index_params* p, const IndexOut& io, hipStream_t stream) {
  if (S == 0) return MPCT_OK;
  std::string err;
  const int rc = launch_traj_indices(y, u, r, S, nref, my, nu, nit, IndexParams{p->t0, p->band_rel, p->band_abs}, io,
                                     stream, &err);
  return rc ? fail(MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                       int32_t my, int32_t nu, int32_t nit, const mpct_index_params* params,
                                       const mpct_index_result* out, void* stream) {
  const int rc = index_check(y, u, r, S, nref, my, nu, nit, params, out);
  if (rc) return rc;
  return index_launch(y, u, r, S, nref, my, nu, nit, params, index_out(out), static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                                int32_t nu, int32_t nit, const mpct_index_params* params, int32_t device,
                                const mpct_index_result* out) {
  int rc = index_check(y, u, r, S, nref, my, nu, nit, params, out);
  if (rc) return rc;
  if (S == 0) return MPCT_OK;  // nothing to stage
  const IndexOut ho = index_out(out);
  CallStage cs{"mpct_indices", "index staging", "trajectories", "index records"};
  // y and r travel only behind an output-row field, u only behind an input-row field
  const int s_y = cs.in(ho.any_y() ? y : nullptr, (size_t)S * my * nit * 8),
            s_u = cs.in(ho.any_u() ? u : nullptr, (size_t)S * nu * nit * 8),
            s_r = cs.in(ho.any_y() ? r : nullptr, (size_t)nref * my * nit * 8);
  const size_t dy = (size_t)S * my * 8, iy = (size_t)S * my * 4, du = (size_t)S * nu * 8;
  const int s_iae = cs.out(ho.iae, dy), s_ise = cs.out(ho.ise, dy), s_itae = cs.out(ho.itae, dy), s_emax = cs.out(ho.emax, dy),
            s_temax = cs.out(ho.t_emax, iy), s_over = cs.out(ho.over, dy), s_efinal = cs.out(ho.e_final, dy),
            s_settle = cs.out(ho.settle, iy), s_tv = cs.out(ho.tv, du), s_du2 = cs.out(ho.du2, du),
            s_dumax = cs.out(ho.dumax, du), s_ulo = cs.out(ho.u_lo, du), s_uhi = cs.out(ho.u_hi, du);
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    IndexOut dv{};
    dv.iae = cs.at<double>(s_iae);
    dv.ise = cs.at<double>(s_ise);
    dv.itae = cs.at<double>(s_itae);
    dv.emax = cs.at<double>(s_emax);
    dv.t_emax = cs.at<int>(s_temax);
    dv.over = cs.at<double>(s_over);
    dv.e_final = cs.at<double>(s_efinal);
    dv.settle = cs.at<int>(s_settle);
    dv.tv = cs.at<double>(s_tv);
    dv.du2 = cs.at<double>(s_du2);
    dv.dumax = cs.at<double>(s_dumax);
    dv.u_lo = cs.at<double>(s_ulo);
    dv.u_hi = cs.at<double>(s_uhi);
    rc = index_launch(cs.at<double>(s_y), cs.at<double>(s_u), cs.at<double>(s_r), S, nref, my, nu, nit, params, dv, cs.st);
  }
  return cs.close(rc);
}

// the chunk budget of mpct_eval_indices(_device) in bytes of trajectory scratch; 0: MPCT_INDEX_SCRATCH_BYTES.
// A test / bench hook, not part of include/mpct.h: the tests force ragged chunks at small sizes with it
static int64_t g_index_budget = 0;
extern "C" int32_t mpct_internal_index_budget(int64_t bytes) {
  if (bytes < 0) return fail(MPCT_EINVAL, "budget < 0");
  g_index_budget = bytes;
  return MPCT_OK;
}

// the trajectories y | u of one candidate in bytes, and the candidates a chunk of the index entries takes: what
// the budget holds, at least one
static size_t traj_bytes(int32_t nref, int my, int nu, int nit) { return (size_t)nref * (my + nu) * nit * 8; }
static int64_t index_chunk(int64_t C, int32_t nref, int my, int nu, int nit) {
  const size_t budget = g_index_budget > 0 ? (size_t)g_index_budget : (size_t)MPCT_INDEX_SCRATCH_BYTES;
  return std::min<int64_t>(C, std::max<int64_t>(1, (int64_t)(budget / traj_bytes(nref, my, nu, nit))));
}

// the caller's options for the closed loops of an index entry: closed loop, trajectories on
static mpct_opts traj_opts(const mpct_opts* opts) {
  mpct_opts o = opts ? *opts : mpct_opts{0, 0, 0, -1, 0.0};
  o.open_loop = 0;
  o.want_traj = 1;
  return o;
}

// width of index field id in a scenario's records, and whether it is an integer field
static int field_width(const mpct_scenario* s, int id) { return id < 8 ? s->my : s->nu; }
static bool field_is_int(int id) { return id == MPCT_IX_T_EMAX || id == MPCT_IX_SETTLE; }

// the argument checks of the two scoring entries, in the header's order; nothing here touches a device
static int check_eval_indices(mpct_scenario* s, const Batch& b, const mpct_opts* opts, const mpct_index_params* p,
                              const mpct_result* res, const mpct_index_result* out) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (res && (res->y || res->u || res->ys || res->uopt))
    return fail(MPCT_EINVAL, "the trajectory pointers of res must be NULL: the trajectories stay on the device");
  const mpct_result any{};
  const int rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  return index_check_tail(b.C * b.nref, s->my, s->nu, s->nit, p, out, true, true);
}

// enqueue one batch with device pointers on `stream` (ctx's device is current): chunks of whole
// candidates through launch_batch into the trajectory scratch, each followed by the reduction kernel
// records(y, u, n, s0): the chunk's trajectories, its n candidates, its first simulation
template <class Records>
static int walk_chunks(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const mpct_result* res,
                       hipStream_t stream, Records records) {
  if (b.C == 0) return MPCT_OK;
  const int my = s->my, nu = s->nu, nit = s->nit;
  const int32_t nref = b.nref;
  const int64_t cc = index_chunk(b.C, nref, my, nu, nit);
  char* scr = nullptr;
  int rc = cx->index.acquire((size_t)cc * traj_bytes(nref, my, nu, nit), stream, "trajectory scratch", &scr);
  if (rc) return rc;
  const mpct_opts o = traj_opts(opts);
  for (int64_t c0 = 0; c0 < b.C && rc == MPCT_OK; c0 += cc) {
    const int64_t n = std::min(cc, b.C - c0), s0 = c0 * nref;
    // the caller's cost fields from this chunk's first simulation on (its trajectory pointers are NULL)
    mpct_result per_chunk = res ? *res : mpct_result{};
    each_field(per_chunk, my, nu, nit, [&](auto*& f, int64_t w) { f = f ? f + s0 * w : nullptr; });
    per_chunk.y = reinterpret_cast<double*>(scr);
    per_chunk.u = per_chunk.y + (size_t)n * nref * my * nit;
    rc = launch_batch(s, cx, b.sub(c0, n, my, nu), &o, &per_chunk, stream);
    if (rc == MPCT_OK) rc = records(per_chunk.y, per_chunk.u, n, s0);
  }
  cx->index.mark(stream);
  return rc;
}

static int launch_indices(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const mpct_index_params* p,
                          const mpct_result* res, const mpct_index_result* out, hipStream_t stream) {
  const IndexOut io = index_out(out);
  return walk_chunks(s, cx, b, opts, res, stream, [&](const double* y, const double* u, int64_t n, int64_t s0) {
    return index_launch(y, u, b.r, n * b.nref, b.nref, s->my, s->nu, s->nit, p, io.from(s0, s->my, s->nu), stream);
  });
}

extern "C" int32_t mpct_eval_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                            const double* delta, const double* lambda, int32_t nref, const double* r,
                                            const double* v, const mpct_opts* opts, const mpct_index_params* params,
                                            mpct_result* res, const mpct_index_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_eval_indices(s, b, opts, params, res, out);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_indices(s, cx, b, opts, params, res, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu, const double* delta,
                                     const double* lambda, int32_t nref, const double* r, const double* v,
                                     const mpct_opts* opts, const mpct_index_params* params, mpct_result* res,
                                     const mpct_index_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_eval_indices(s, b, opts, params, res, out);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  // host buffers in, the records out on the context's own stream, staged as eval_host does
  const size_t S = (size_t)(C * nref);
  HostStage hs(s, cx, C);
  // slots 0..9: with a `res` its six cost fields live on the device, its trajectories never; 10..22: the index
  // fields that are asked for
  mpct_result hres = res ? *res : mpct_result{};
  int k = 0;
  each_field(hres, s->my, s->nu, s->nit, [&](auto* host, int64_t w) {
    hs.keep(host, S * w * sizeof(*host), res && k < 6);
    ++k;
  });
  void* const host[13] = {out->iae,    out->ise, out->itae, out->emax,  out->t_emax, out->over, out->e_final,
                          out->settle, out->tv,  out->du2,  out->dumax, out->u_lo,   out->u_hi};
  for (int id = 0; id < 13; ++id) hs.want(host[id], S * field_width(s, id) * (field_is_int(id) ? 4 : 8));
  rc = hs.upload(s, b);
  if (rc) return rc;
  mpct_result dres{};
  k = 0;
  each_field(dres, s->my, s->nu, s->nit, [&](auto*& dev, int64_t) { hs.bind(k++, dev); });
  auto dd = [&](int id) { return hs.at<double>(10 + id); };
  auto di = [&](int id) { return hs.at<int32_t>(10 + id); };
  const mpct_index_result dout{dd(0), dd(1), dd(2), dd(3), di(4), dd(5), dd(6), di(7), dd(8), dd(9), dd(10), dd(11), dd(12)};
  rc = launch_indices(s, cx, hs.dev, opts, params, res ? &dres : nullptr, &dout, hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

// ------------------------------------------------------------------------------------------
// statistics of a table over its draw axis, and of the performance indices over the plant draws
// (draw_stats.hip; include/mpct.h)

static DrawStatsOut stats_out(const mpct_draw_stats_result* o) {
  return DrawStatsOut{o->n, o->mean, o->lo, o->lo_draw, o->hi, o->hi_draw, o->quantile, o->cvar, o->q_draw};
}

// the level checks both entries share, in the header's order
static int stats_check_levels(int32_t nlev, const double* levels) {
  if (nlev < 0 || nlev > MPCT_TAIL_MAX_LEVELS) return fail(MPCT_EINVAL, "nlev must be 0 .. MPCT_TAIL_MAX_LEVELS (8)");
  if (nlev > 0 && !levels) return fail(MPCT_EINVAL, "null levels");
  for (int j = 0; j < nlev; ++j)
    if (!(levels[j] > 0.0 && levels[j] <= 1.0)) return fail(MPCT_EINVAL, "every level must lie in (0, 1], not NaN");
  return MPCT_OK;
}

// the argument checks of the primitive's two entries, in the header's order; nothing here touches a device
static int stats_check(const void* x, int32_t x_type, int64_t C, int32_t D, int32_t m, int32_t nlev, const double* levels,
                       const mpct_draw_stats_result* out) {
  if (C < 0 || D < 1 || m < 1) return fail(MPCT_EINVAL, "bad shape: C < 0, D < 1 or m < 1");
  if (x_type != MPCT_STAT_F64 && x_type != MPCT_STAT_I32) return fail(MPCT_EINVAL, "x_type must be MPCT_STAT_F64 or MPCT_STAT_I32");
  const int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  if (!out || !stats_out(out).any()) return fail(MPCT_EINVAL, "no output pointer in mpct_draw_stats_result");
  if (nlev == 0 && stats_out(out).any_level()) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  if (C > 0 && !x) return fail(MPCT_EINVAL, "x is NULL");
  if (D > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "D > MPCT_TAIL_MAX_DRAWS (4096): the kernel's LDS holds no more draws");
  if (C * (int64_t)m > MPCT_INDEX_MAX_ROWS) return fail(MPCT_ERANGE, "C*m exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

// the largest grid of draw_stats_kernel in workgroups; 0: kStatGridCap.  A test hook, not part of
// include/mpct.h: the tests force the workgroups to stride at small sizes with it
static int32_t g_stats_grid = 0;
extern "C" int32_t mpct_internal_draw_stats_grid(int32_t groups) {
  if (groups < 0) return fail(MPCT_EINVAL, "groups < 0");
  g_stats_grid = groups;
  return MPCT_OK;
}

static int32_t stats_launch(const void* x, int32_t x_type, const int32_t* alive, int64_t C, int32_t D, int32_t m,
                            int32_t nlev, const double* levels, const DrawStatsOut& out, int ldo, int off,
                            hipStream_t stream) {
  std::string err;
  const int rc = launch_draw_stats(x, x_type, alive, C, D, m, nlev, levels, out, ldo, off, g_stats_grid, stream, &err);
  return rc ? fail(MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_draw_stats_device(const void* x, int32_t x_type, const int32_t* alive, int64_t C, int32_t D,
                                          int32_t m, int32_t nlev, const double* levels,
                                          const mpct_draw_stats_result* out, void* stream) {
  const int rc = stats_check(x, x_type, C, D, m, nlev, levels, out);
  if (rc) return rc;
  return stats_launch(x, x_type, alive, C, D, m, nlev, levels, stats_out(out), m, 0, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_draw_stats(const void* x, int32_t x_type, const int32_t* alive, int64_t C, int32_t D, int32_t m,
                                   int32_t nlev, const double* levels, int32_t device, const mpct_draw_stats_result* out) {
  int rc = stats_check(x, x_type, C, D, m, nlev, levels, out);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage
  CallStage cs{"mpct_draw_stats", "draw statistics staging", "table", "draw statistics"};
  // the per-level fields are asked for with nlev >= 1 only (stats_check); levels stays on the host
  const size_t cols = (size_t)C * m, lev = cols * (size_t)nlev;
  const int s_x = cs.in(x, (size_t)C * D * m * (x_type == MPCT_STAT_I32 ? 4 : 8)), s_alive = cs.in(alive, (size_t)C * D * 4);
  const int s_n = cs.out(out->n, cols * 4), s_mean = cs.out(out->mean, cols * 8), s_lo = cs.out(out->lo, cols * 8),
            s_lodraw = cs.out(out->lo_draw, cols * 4), s_hi = cs.out(out->hi, cols * 8), s_hidraw = cs.out(out->hi_draw, cols * 4),
            s_quantile = cs.out(out->quantile, lev * 8), s_cvar = cs.out(out->cvar, lev * 8), s_qdraw = cs.out(out->q_draw, lev * 4);
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    DrawStatsOut dv{};
    dv.n = cs.at<int32_t>(s_n);
    dv.mean = cs.at<double>(s_mean);
    dv.lo = cs.at<double>(s_lo);
    dv.lo_draw = cs.at<int32_t>(s_lodraw);
    dv.hi = cs.at<double>(s_hi);
    dv.hi_draw = cs.at<int32_t>(s_hidraw);
    dv.quantile = cs.at<double>(s_quantile);
    dv.cvar = cs.at<double>(s_cvar);
    dv.q_draw = cs.at<int32_t>(s_qdraw);
    rc = stats_launch(cs.at<char>(s_x), x_type, cs.at<int32_t>(s_alive), C, D, m, nlev, levels, dv, m, 0, cs.st);
  }
  return cs.close(rc);
}

// the argument checks of the two robust index entries, in the header's order; nothing here touches a device
static int check_robust_indices(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                                const mpct_index_params* p, int32_t nsel, const int32_t* fields, int32_t nlev,
                                const double* levels, const mpct_robust_result* base, const mpct_draw_stats_result* out) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (nsel < 1 || nsel > 13 || !fields) return fail(MPCT_EINVAL, "nsel must be 1 .. 13 with a field list");
  unsigned seen = 0;
  for (int q = 0; q < nsel; ++q) {
    if (fields[q] < MPCT_IX_IAE || fields[q] > MPCT_IX_U_HI) return fail(MPCT_EINVAL, "field id out of range");
    if (seen & (1u << fields[q])) return fail(MPCT_EINVAL, "field id repeated");
    seen |= 1u << fields[q];
  }
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: the statistics need at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  const bool any_base = base && (base->mean || base->worst || base->n_failed || base->worst_draw || base->status);
  const bool any_out = out && stats_out(out).any();
  if (!any_base && !any_out) return fail(MPCT_EINVAL, "every output pointer of base and out is NULL");
  if (base && base->J1) return fail(MPCT_EINVAL, "base->J1 must be NULL: the sample lives per chunk");
  if (nlev == 0 && out && stats_out(out).any_level()) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  const mpct_result any{};
  rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = index_check_params(s->nit, p);
  if (rc) return rc;
  if (b.nref > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "nref > MPCT_TAIL_MAX_DRAWS (4096): the kernel's LDS holds no more draws");
  if (b.C * b.nref * (int64_t)s->my > kIndexMaxRows || b.C * b.nref * (int64_t)s->nu > kIndexMaxRows)
    return fail(MPCT_ERANGE, "C*nref*my or C*nref*nu exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

// enqueue one batch with device pointers on `stream` (ctx's device is current).  Per chunk of whole
// candidates: the closed loops with trajectories, J1 and status into the context's index scratch, the
// selected index records, alive[c][k], then the statistics of each selected field and the base record
// (shared by the performance, the limit and the segment indices: ny_fields of the up to kMaxRobustFields field
// ids are output-row fields, a row holds per_row values of a field (the segments; else 1), int_mask has the
// bits of the int32 ones, records(rec, y, u, S) enqueues the chunk's reduction kernel with rec[id] the
// selected fields' device records)
constexpr int kMaxRobustFields = 15;

// The walk itself, shared with the trajectory envelopes (envelope.hip), whose "record" is the trajectory:
// extra(Sc) is the scratch in bytes a chunk of Sc simulations needs behind alive; records(ex, y, u, S) enqueues
// what reduces the chunk's S simulations into that scratch `ex`; reduce(ex, y, u, alive, c0, n) enqueues the
// statistics of the chunk's n candidates, the batch's c0 onwards, once alive is written
template <class Extra, class Records, class Reduce>
static int walk_draw_chunks(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                            const RobustOut& base, hipStream_t stream, Extra extra, Records records, Reduce reduce) {
  if (b.C == 0) return MPCT_OK;
  const int my = s->my, nu = s->nu, nit = s->nit;
  const int64_t C = b.C;
  const int32_t nref = b.nref;
  const double bound = j_bound == 0.0 ? kRobustDefaultBound : j_bound;
  const int64_t cc = index_chunk(C, nref, my, nu, nit);  // launch_indices' chunking
  // the chunk's scratch: y | u | J1 | status | alive | the walk's own records, each 256-B aligned
  auto al = [](size_t n) { return (n + 255) & ~(size_t)255; };
  const size_t Sc = (size_t)cc * nref;
  const size_t o_j1 = al((size_t)cc * traj_bytes(nref, my, nu, nit)), o_st = o_j1 + al(Sc * my * 8), o_al = o_st + al(Sc * 4);
  const size_t o_ex = o_al + al(Sc * 4);
  char* scr = nullptr;
  int rc = cx->index.acquire(o_ex + extra(Sc), stream, "trajectory scratch", &scr);
  if (rc) return rc;
  const mpct_opts o = traj_opts(opts);
  const bool any_base = base.mean || base.worst || base.n_failed || base.worst_draw || base.status;
  std::string err;
  for (int64_t c0 = 0; c0 < C && rc == MPCT_OK; c0 += cc) {
    const int64_t n = std::min(cc, C - c0);
    mpct_result per_chunk{};
    per_chunk.J1 = reinterpret_cast<double*>(scr + o_j1);
    per_chunk.status = reinterpret_cast<int32_t*>(scr + o_st);
    per_chunk.y = reinterpret_cast<double*>(scr);
    per_chunk.u = per_chunk.y + (size_t)n * nref * my * nit;
    int32_t* alive = reinterpret_cast<int32_t*>(scr + o_al);
    rc = launch_batch(s, cx, b.sub(c0, n, my, nu), &o, &per_chunk, stream);
    if (rc == MPCT_OK) rc = records(scr + o_ex, per_chunk.y, per_chunk.u, n * nref);
    if (rc != MPCT_OK) break;
    int lrc = launch_draw_alive(n, nref, my, bound, per_chunk.J1, per_chunk.status, alive, stream, &err);
    if (lrc == 0 && any_base) {
      auto d = [](double* q, int64_t e) { return q ? q + e : nullptr; };
      auto i = [](int32_t* q, int64_t e) { return q ? q + e : nullptr; };
      const RobustOut ro{d(base.mean, c0 * my), d(base.worst, c0 * my), i(base.n_failed, c0), i(base.worst_draw, c0),
                         i(base.status, c0)};
      lrc = launch_robust_reduce(n, nref, my, bound, per_chunk.J1, per_chunk.status, ro, stream, &err);
    }
    if (lrc) {
      rc = fail(MPCT_EDEVICE, err);
      break;
    }
    rc = reduce(scr + o_ex, per_chunk.y, per_chunk.u, alive, c0, n);
  }
  cx->index.mark(stream);
  return rc;
}

template <class Records>
static int walk_robust_chunks(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                              int ny_fields, int per_row, unsigned int_mask, int32_t nsel, const int32_t* fields, int32_t nlev,
                              const double* levels, const RobustOut& base, const DrawStatsOut& out, hipStream_t stream,
                              Records records) {
  auto field_width = [&](const mpct_scenario* sc, int id) { return (id < ny_fields ? sc->my : sc->nu) * per_row; };
  auto field_is_int = [&](int id) { return (int_mask >> id & 1u) != 0; };
  // the selected fields' records, each 256-B aligned
  size_t o_f[kMaxRobustFields];
  int W = 0;
  for (int q = 0; q < nsel; ++q) W += field_width(s, fields[q]);
  void* rec[kMaxRobustFields] = {nullptr};
  return walk_draw_chunks(
      s, cx, b, j_bound, opts, base, stream,
      [&](size_t Sc) {
        size_t off = 0;
        for (int q = 0; q < nsel; ++q) {
          o_f[q] = off;
          off += (Sc * field_width(s, fields[q]) * (field_is_int(fields[q]) ? 4 : 8) + 255) & ~(size_t)255;
        }
        return off;
      },
      [&](char* ex, const double* y, const double* u, int64_t S) {
        for (int q = 0; q < nsel; ++q) rec[fields[q]] = ex + o_f[q];
        return records(rec, y, u, S);
      },
      [&](char*, const double*, const double*, const int32_t* alive, int64_t c0, int64_t n) {
        int rc = MPCT_OK, col = 0;
        if (!out.any()) return rc;
        for (int q = 0; q < nsel && rc == MPCT_OK; ++q) {
          const int w = field_width(s, fields[q]);
          rc = stats_launch(rec[fields[q]], field_is_int(fields[q]) ? MPCT_STAT_I32 : MPCT_STAT_F64, alive, n, b.nref, w,
                            nlev, levels, out.from(c0, W, nlev), W, col, stream);
          col += w;
        }
        return rc;
      });
}

static int launch_robust_indices(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                                 const mpct_index_params* p, int32_t nsel, const int32_t* fields, int32_t nlev,
                                 const double* levels, const RobustOut& base, const DrawStatsOut& out, hipStream_t stream) {
  const unsigned ints = 1u << MPCT_IX_T_EMAX | 1u << MPCT_IX_SETTLE;
  return walk_robust_chunks(
      s, cx, b, j_bound, opts, 8, 1, ints, nsel, fields, nlev, levels, base, out, stream,
      [&](void* const* rec, const double* y, const double* u, int64_t S) {
        const IndexOut io{(double*)rec[0], (double*)rec[1], (double*)rec[2], (double*)rec[3],  (int*)rec[4],
                          (double*)rec[5], (double*)rec[6], (int*)rec[7],    (double*)rec[8],  (double*)rec[9],
                          (double*)rec[10], (double*)rec[11], (double*)rec[12]};
        return index_launch(y, u, b.r, S, b.nref, s->my, s->nu, s->nit, p, io, stream);
      });
}

extern "C" int32_t mpct_eval_robust_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                   const double* delta, const double* lambda, int32_t nref,
                                                   const double* r, const double* v, double j_bound,
                                                   const mpct_opts* opts, const mpct_index_params* params, int32_t nsel,
                                                   const int32_t* fields, int32_t nlev, const double* levels,
                                                   mpct_robust_result* base, const mpct_draw_stats_result* out,
                                                   void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_robust_indices(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const RobustOut ro = base ? RobustOut{base->mean, base->worst, base->n_failed, base->worst_draw, base->status} : RobustOut{};
  return launch_robust_indices(s, cx, b, j_bound, opts, params, nsel, fields, nlev, levels, ro,
                               out ? stats_out(out) : DrawStatsOut{}, static_cast<hipStream_t>(stream));
}

// host buffers in, the statistics of W columns out on the context's own stream, staged as eval_host does:
// every field of base and out lives on the device only where it is asked for (the per-level ones only with
// nlev >= 1).  launch(hs, ro, dv) enqueues the walk on hs.st with the device-side batch hs.dev
template <class Launch>
static int robust_stats_host(mpct_scenario* s, DevCtx* cx, const Batch& b, size_t W, int32_t nlev,
                             const mpct_robust_result* base, const mpct_draw_stats_result* out, Launch launch) {
  const size_t C = (size_t)b.C, cm = C * s->my * 8, cols = C * W, lev = cols * (size_t)nlev;
  const mpct_robust_result hb = base ? *base : mpct_robust_result{};
  const mpct_draw_stats_result ho = out ? *out : mpct_draw_stats_result{};
  HostStage hs(s, cx, b.C);
  const int s_mean = hs.want(hb.mean, cm), s_worst = hs.want(hb.worst, cm), s_nf = hs.want(hb.n_failed, C * 4),
            s_wd = hs.want(hb.worst_draw, C * 4), s_st = hs.want(hb.status, C * 4);
  const int s_n = hs.want(ho.n, cols * 4), s_mn = hs.want(ho.mean, cols * 8), s_lo = hs.want(ho.lo, cols * 8),
            s_ld = hs.want(ho.lo_draw, cols * 4), s_hi = hs.want(ho.hi, cols * 8), s_hd = hs.want(ho.hi_draw, cols * 4),
            s_q = hs.want(ho.quantile, lev * 8), s_cv = hs.want(ho.cvar, lev * 8), s_qd = hs.want(ho.q_draw, lev * 4);
  int rc = hs.upload(s, b);
  if (rc) return rc;
  const RobustOut ro{hs.at<double>(s_mean), hs.at<double>(s_worst), hs.at<int32_t>(s_nf), hs.at<int32_t>(s_wd),
                     hs.at<int32_t>(s_st)};
  const DrawStatsOut dv{hs.at<int32_t>(s_n),  hs.at<double>(s_mn), hs.at<double>(s_lo), hs.at<int32_t>(s_ld), hs.at<double>(s_hi),
                        hs.at<int32_t>(s_hd), hs.at<double>(s_q),  hs.at<double>(s_cv), hs.at<int32_t>(s_qd)};
  rc = launch(hs, ro, dv);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

extern "C" int32_t mpct_eval_robust_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                            const double* delta, const double* lambda, int32_t nref, const double* r,
                                            const double* v, double j_bound, const mpct_opts* opts,
                                            const mpct_index_params* params, int32_t nsel, const int32_t* fields,
                                            int32_t nlev, const double* levels, mpct_robust_result* base,
                                            const mpct_draw_stats_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_robust_indices(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  size_t W = 0;
  for (int q = 0; q < nsel; ++q) W += field_width(s, fields[q]);
  return robust_stats_host(s, cx, b, W, nlev, base, out, [&](HostStage& hs, const RobustOut& ro, const DrawStatsOut& dv) {
    return launch_robust_indices(s, cx, hs.dev, j_bound, opts, params, nsel, fields, nlev, levels, ro, dv, hs.st);
  });
}

// ------------------------------------------------------------------------------------------
// limit indices per simulation and their statistics over the draws (limit_indices.hip; include/mpct.h,
// DESIGN.md §20)

static LimitOut limit_out(const mpct_limit_result* o) {
  return LimitOut{o->viol, o->viol2, o->vmax,   o->t_vmax,  o->n_out,    o->t_in,     o->y_margin,
                  o->n_lo, o->n_hi,  o->n_rate, o->sat_run, o->u_margin, o->du_margin};
}
// width of limit field id in a scenario's records, and the bits of the int32 fields
static int limit_width(const mpct_scenario* s, int id) { return id < MPCT_LX_N_LO ? s->my : s->nu; }
constexpr unsigned kLimitInts = 1u << MPCT_LX_T_VMAX | 1u << MPCT_LX_N_OUT | 1u << MPCT_LX_T_IN | 1u << MPCT_LX_N_LO |
                                1u << MPCT_LX_N_HI | 1u << MPCT_LX_N_RATE | 1u << MPCT_LX_SAT_RUN;

// the checks on the parameters from t0 on, in the header's order, and the kernel's by-value parameters: the
// caller's array where it gave one, else the scenario's own bound (s may be NULL), else no bound
static int limit_resolve(const mpct_scenario* s, int32_t my, int32_t nu, int32_t nit, const mpct_limit_params* p,
                         LimitParams* lp) {
  if (p->t0 < 0 || p->t0 >= nit) return fail(MPCT_EINVAL, "t0 must be 0 .. nit-1");
  if (my > MPCT_LIMIT_MAX_CH || nu > MPCT_LIMIT_MAX_CH)
    return fail(MPCT_ERANGE, "my or nu exceeds MPCT_LIMIT_MAX_CH (32): the bounds travel in the kernel argument");
  if (!(p->out_tol >= 0.0 && p->out_tol <= 1.7976931348623157e308 && p->sat_tol >= 0.0 &&
        p->sat_tol <= 1.7976931348623157e308))
    return fail(MPCT_EINVAL, "out_tol and sat_tol must be finite and >= 0, not NaN");
  const double *sy_lo = nullptr, *sy_hi = nullptr, *su_lo = nullptr, *su_hi = nullptr, *sd_lo = nullptr, *sd_hi = nullptr;
  if (s && s->nmpc) {  // nm: parameters | x0[3] | u0[nu] | u_min[nu] | u_max[nu] | ..
    su_lo = s->nm.data() + NM_NPAR + 3 + nu;
    su_hi = su_lo + nu;
  } else if (s) {
    sd_lo = s->bnd.data(), sd_hi = sd_lo + nu, su_lo = sd_lo + 2 * nu, su_hi = sd_lo + 3 * nu;
    if (s->mdband) sy_lo = s->obnd.data(), sy_hi = sy_lo + my;
  }
  *lp = LimitParams{};
  lp->t0 = p->t0, lp->out_tol = p->out_tol, lp->sat_tol = p->sat_tol;
  auto fill = [](double* dst, const double* own, const double* scen, int n, double none) {
    for (int c = 0; c < kLimitMaxCh; ++c) dst[c] = c >= n ? none : (own ? own[c] : (scen ? scen[c] : none));
  };
  fill(lp->y_lo, p->y_lo, sy_lo, my, -INFINITY), fill(lp->y_hi, p->y_hi, sy_hi, my, INFINITY);
  fill(lp->u_lo, p->u_lo, su_lo, nu, -INFINITY), fill(lp->u_hi, p->u_hi, su_hi, nu, INFINITY);
  fill(lp->du_lo, p->du_lo, sd_lo, nu, -INFINITY), fill(lp->du_hi, p->du_hi, sd_hi, nu, INFINITY);
  auto ok = [](const double* lo, const double* hi, int n) {
    for (int c = 0; c < n; ++c)
      if (!(lo[c] <= hi[c]) || lo[c] == INFINITY || hi[c] == -INFINITY) return false;  // !(<=) catches NaN
    return true;
  };
  if (!ok(lp->y_lo, lp->y_hi, my) || !ok(lp->u_lo, lp->u_hi, nu) || !ok(lp->du_lo, lp->du_hi, nu))
    return fail(MPCT_EINVAL, "bad bound: NaN, a lower bound above its upper bound, lower = +inf or upper = -inf");
  return MPCT_OK;
}

static int limit_check_out(int64_t S, int32_t my, int32_t nu, const mpct_limit_result* out, bool have_y, bool have_u) {
  if (!out) return fail(MPCT_EINVAL, "no output pointer in mpct_limit_result");
  const LimitOut lo = limit_out(out);
  if (!lo.any_y() && !lo.any_u()) return fail(MPCT_EINVAL, "no output pointer in mpct_limit_result");
  if (lo.any_y() && (my < 1 || (S > 0 && !have_y)))
    return fail(MPCT_EINVAL, "an output-row field needs my >= 1 and the trajectory y");
  if (lo.any_u() && (nu < 1 || (S > 0 && !have_u)))
    return fail(MPCT_EINVAL, "an input-row field needs nu >= 1 and the trajectory u");
  if (S * (int64_t)my > kIndexMaxRows || S * (int64_t)nu > kIndexMaxRows)
    return fail(MPCT_ERANGE, "S*my or S*nu exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int limit_check(const double* y, const double* u, int64_t S, int32_t my, int32_t nu, int32_t nit,
                       const mpct_limit_params* p, const mpct_limit_result* out, LimitParams* lp) {
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (S < 0 || my < 0 || nu < 0 || nit < 1) return fail(MPCT_EINVAL, "bad shape: S < 0, my < 0, nu < 0 or nit < 1");
  const int rc = limit_resolve(nullptr, my, nu, nit, p, lp);
  if (rc) return rc;
  return limit_check_out(S, my, nu, out, y != nullptr, u != nullptr);
}

static int32_t limit_launch(const double* y, const double* u, int64_t S, int32_t my, int32_t nu, int32_t nit,
                            const LimitParams& lp, const LimitOut& lo, hipStream_t stream) {
  if (S == 0) return MPCT_OK;
  std::string err;
  const int rc = launch_limit_indices(y, u, S, my, nu, nit, lp, lo, stream, &err);
  return rc ? fail(MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_limit_indices_device(const double* y, const double* u, int64_t S, int32_t my, int32_t nu,
                                             int32_t nit, const mpct_limit_params* params, const mpct_limit_result* out,
                                             void* stream) {
  LimitParams lp;
  const int rc = limit_check(y, u, S, my, nu, nit, params, out, &lp);
  if (rc) return rc;
  return limit_launch(y, u, S, my, nu, nit, lp, limit_out(out), static_cast<hipStream_t>(stream));
}

// the thirteen fields of an mpct_limit_result in the struct's order, each with its host pointer, its width
// per simulation and its element size
template <class F>
static void each_limit_field(const mpct_limit_result& o, int my, int nu, F f) {
  void* const host[13] = {o.viol, o.viol2, o.vmax,   o.t_vmax,  o.n_out,    o.t_in,     o.y_margin,
                          o.n_lo, o.n_hi,  o.n_rate, o.sat_run, o.u_margin, o.du_margin};
  for (int id = 0; id < 13; ++id) f(id, host[id], id < MPCT_LX_N_LO ? my : nu, (kLimitInts >> id & 1u) ? 4 : 8);
}
// the device-side record from the slots slot0 .. slot0 + 12 of a stage
template <class Stage>
static mpct_limit_result limit_slots(const Stage& st, int slot0) {
  auto dd = [&](int id) { return st.template at<double>(slot0 + id); };
  auto di = [&](int id) { return st.template at<int32_t>(slot0 + id); };
  return mpct_limit_result{dd(0), dd(1), dd(2), di(3), di(4), di(5), dd(6), di(7), di(8), di(9), di(10), dd(11), dd(12)};
}

extern "C" int32_t mpct_limit_indices(const double* y, const double* u, int64_t S, int32_t my, int32_t nu, int32_t nit,
                                      const mpct_limit_params* params, int32_t device, const mpct_limit_result* out) {
  LimitParams lp;
  int rc = limit_check(y, u, S, my, nu, nit, params, out, &lp);
  if (rc) return rc;
  if (S == 0) return MPCT_OK;  // nothing to stage
  const LimitOut ho = limit_out(out);
  CallStage cs{"mpct_limit_indices", "limit staging", "trajectories", "limit records"};
  // y travels only behind an output-row field, u only behind an input-row field
  const int s_y = cs.in(ho.any_y() ? y : nullptr, (size_t)S * my * nit * 8),
            s_u = cs.in(ho.any_u() ? u : nullptr, (size_t)S * nu * nit * 8);
  int slot0 = -1;
  each_limit_field(*out, my, nu, [&](int, void* host, int w, int esz) {
    const int k = cs.out(host, (size_t)S * w * esz);
    if (slot0 < 0) slot0 = k;
  });
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    const mpct_limit_result dv = limit_slots(cs, slot0);
    rc = limit_launch(cs.at<double>(s_y), cs.at<double>(s_u), S, my, nu, nit, lp, limit_out(&dv), cs.st);
  }
  return cs.close(rc);
}

// the argument checks of the two scoring entries, in the header's order; nothing here touches a device
static int check_eval_limits(mpct_scenario* s, const Batch& b, const mpct_opts* opts, const mpct_limit_params* p,
                             const mpct_result* res, const mpct_limit_result* out, LimitParams* lp) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (res && (res->y || res->u || res->ys || res->uopt))
    return fail(MPCT_EINVAL, "the trajectory pointers of res must be NULL: the trajectories stay on the device");
  const mpct_result any{};
  int rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = limit_resolve(s, s->my, s->nu, s->nit, p, lp);
  if (rc) return rc;
  return limit_check_out(b.C * b.nref, s->my, s->nu, out, true, true);
}

static int launch_limits(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const LimitParams& lp,
                         const mpct_result* res, const mpct_limit_result* out, hipStream_t stream) {
  const LimitOut lo = limit_out(out);
  return walk_chunks(s, cx, b, opts, res, stream, [&](const double* y, const double* u, int64_t n, int64_t s0) {
    return limit_launch(y, u, n * b.nref, s->my, s->nu, s->nit, lp, lo.from(s0, s->my, s->nu), stream);
  });
}

extern "C" int32_t mpct_eval_limit_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                  const double* delta, const double* lambda, int32_t nref,
                                                  const double* r, const double* v, const mpct_opts* opts,
                                                  const mpct_limit_params* params, mpct_result* res,
                                                  const mpct_limit_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  LimitParams lp;
  int rc = check_eval_limits(s, b, opts, params, res, out, &lp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_limits(s, cx, b, opts, lp, res, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_limit_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                           const double* delta, const double* lambda, int32_t nref, const double* r,
                                           const double* v, const mpct_opts* opts, const mpct_limit_params* params,
                                           mpct_result* res, const mpct_limit_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  LimitParams lp;
  int rc = check_eval_limits(s, b, opts, params, res, out, &lp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  // host buffers in, the records out on the context's own stream, staged as mpct_eval_indices does: slots
  // 0..9 the fields of `res` (its six cost fields on the device with a `res`, its trajectories never),
  // 10..22 the limit fields that are asked for
  const size_t S = (size_t)(C * nref);
  HostStage hs(s, cx, C);
  mpct_result hres = res ? *res : mpct_result{};
  int k = 0;
  each_field(hres, s->my, s->nu, s->nit, [&](auto* host, int64_t w) {
    hs.keep(host, S * w * sizeof(*host), res && k < 6);
    ++k;
  });
  each_limit_field(*out, s->my, s->nu, [&](int, void* host, int w, int esz) { hs.want(host, S * w * esz); });
  rc = hs.upload(s, b);
  if (rc) return rc;
  mpct_result dres{};
  k = 0;
  each_field(dres, s->my, s->nu, s->nit, [&](auto*& dev, int64_t) { hs.bind(k++, dev); });
  const mpct_limit_result dout = limit_slots(hs, 10);
  rc = launch_limits(s, cx, hs.dev, opts, lp, res ? &dres : nullptr, &dout, hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

// the argument checks of the two robust limit entries, in the header's order; nothing here touches a device
static int check_robust_limits(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                               const mpct_limit_params* p, int32_t nsel, const int32_t* fields, int32_t nlev,
                               const double* levels, const mpct_robust_result* base, const mpct_draw_stats_result* out,
                               LimitParams* lp) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (nsel < 1 || nsel > 13 || !fields) return fail(MPCT_EINVAL, "nsel must be 1 .. 13 with a field list");
  unsigned seen = 0;
  for (int q = 0; q < nsel; ++q) {
    if (fields[q] < MPCT_LX_VIOL || fields[q] > MPCT_LX_DU_MARGIN) return fail(MPCT_EINVAL, "field id out of range");
    if (seen & (1u << fields[q])) return fail(MPCT_EINVAL, "field id repeated");
    seen |= 1u << fields[q];
  }
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: the statistics need at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  const bool any_base = base && (base->mean || base->worst || base->n_failed || base->worst_draw || base->status);
  const bool any_out = out && stats_out(out).any();
  if (!any_base && !any_out) return fail(MPCT_EINVAL, "every output pointer of base and out is NULL");
  if (base && base->J1) return fail(MPCT_EINVAL, "base->J1 must be NULL: the sample lives per chunk");
  if (nlev == 0 && out && stats_out(out).any_level()) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  const mpct_result any{};
  rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = limit_resolve(s, s->my, s->nu, s->nit, p, lp);
  if (rc) return rc;
  if (b.nref > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "nref > MPCT_TAIL_MAX_DRAWS (4096): the kernel's LDS holds no more draws");
  if (b.C * b.nref * (int64_t)s->my > kIndexMaxRows || b.C * b.nref * (int64_t)s->nu > kIndexMaxRows)
    return fail(MPCT_ERANGE, "C*nref*my or C*nref*nu exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int launch_robust_limits(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                                const LimitParams& lp, int32_t nsel, const int32_t* fields, int32_t nlev,
                                const double* levels, const RobustOut& base, const DrawStatsOut& out, hipStream_t stream) {
  return walk_robust_chunks(
      s, cx, b, j_bound, opts, MPCT_LX_N_LO, 1, kLimitInts, nsel, fields, nlev, levels, base, out, stream,
      [&](void* const* rec, const double* y, const double* u, int64_t S) {
        const LimitOut lo{(double*)rec[0], (double*)rec[1], (double*)rec[2],  (int*)rec[3],     (int*)rec[4],
                          (int*)rec[5],    (double*)rec[6], (int*)rec[7],     (int*)rec[8],     (int*)rec[9],
                          (int*)rec[10],   (double*)rec[11], (double*)rec[12]};
        return limit_launch(y, u, S, s->my, s->nu, s->nit, lp, lo, stream);
      });
}

extern "C" int32_t mpct_eval_robust_limit_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                         const double* delta, const double* lambda, int32_t nref,
                                                         const double* r, const double* v, double j_bound,
                                                         const mpct_opts* opts, const mpct_limit_params* params,
                                                         int32_t nsel, const int32_t* fields, int32_t nlev,
                                                         const double* levels, mpct_robust_result* base,
                                                         const mpct_draw_stats_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  LimitParams lp;
  int rc = check_robust_limits(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &lp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const RobustOut ro = base ? RobustOut{base->mean, base->worst, base->n_failed, base->worst_draw, base->status} : RobustOut{};
  return launch_robust_limits(s, cx, b, j_bound, opts, lp, nsel, fields, nlev, levels, ro,
                              out ? stats_out(out) : DrawStatsOut{}, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_robust_limit_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                  const double* delta, const double* lambda, int32_t nref,
                                                  const double* r, const double* v, double j_bound,
                                                  const mpct_opts* opts, const mpct_limit_params* params, int32_t nsel,
                                                  const int32_t* fields, int32_t nlev, const double* levels,
                                                  mpct_robust_result* base, const mpct_draw_stats_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  LimitParams lp;
  int rc = check_robust_limits(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &lp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  size_t W = 0;
  for (int q = 0; q < nsel; ++q) W += limit_width(s, fields[q]);
  return robust_stats_host(s, cx, b, W, nlev, base, out, [&](HostStage& hs, const RobustOut& ro, const DrawStatsOut& dv) {
    return launch_robust_limits(s, cx, hs.dev, j_bound, opts, lp, nsel, fields, nlev, levels, ro, dv, hs.st);
  });
}

// ------------------------------------------------------------------------------------------
// step-response indices per setpoint segment and their statistics over the draws (segment_indices.hip;
// include/mpct.h)

static SegOut seg_out(const mpct_segment_result* o) {
  return SegOut{o->iae,    o->ise,  o->itae, o->emax, o->t_emax, o->over, o->under, o->e_final,
                o->settle, o->rise, o->tv,   o->du2,  o->dumax,  o->u_lo, o->u_hi};
}
// the bits of the int32 fields, and the fields of an mpct_segment_result in the struct's order, each with its
// host pointer, its width per simulation and segment and its element size
constexpr unsigned kSegInts = 1u << MPCT_SX_T_EMAX | 1u << MPCT_SX_SETTLE | 1u << MPCT_SX_RISE;
template <class F>
static void each_seg_field(const mpct_segment_result& o, int my, int nu, F f) {
  void* const host[15] = {o.iae,    o.ise,  o.itae, o.emax, o.t_emax, o.over, o.under, o.e_final,
                          o.settle, o.rise, o.tv,   o.du2,  o.dumax,  o.u_lo, o.u_hi};
  for (int id = 0; id < 15; ++id) f(id, host[id], id < MPCT_SX_TV ? my : nu, (kSegInts >> id & 1u) ? 4 : 8);
}
// the device-side record from the slots slot0 .. slot0 + 14 of a stage
template <class Stage>
static mpct_segment_result seg_slots(const Stage& st, int slot0) {
  auto dd = [&](int id) { return st.template at<double>(slot0 + id); };
  auto di = [&](int id) { return st.template at<int32_t>(slot0 + id); };
  return mpct_segment_result{dd(0), dd(1), dd(2), dd(3), di(4), dd(5), dd(6), dd(7), di(8), di(9), dd(10), dd(11), dd(12),
                             dd(13), dd(14)};
}

// the checks on the parameters from nseg to rise_hi, in the header's order, and the kernel's by-value parameters
static int seg_resolve(int32_t nit, const mpct_segment_params* p, SegParams* sp) {
  if (p->nseg < 1 || !p->tseg) return fail(MPCT_EINVAL, "nseg must be >= 1 with a boundary list tseg");
  if (p->nseg > MPCT_SEG_MAX)
    return fail(MPCT_ERANGE, "nseg exceeds MPCT_SEG_MAX (16): the boundaries travel in the kernel argument");
  bool ok = p->tseg[0] >= 0 && p->tseg[p->nseg] <= nit;
  for (int g = 0; g < p->nseg; ++g) ok = ok && p->tseg[g] < p->tseg[g + 1];
  if (!ok) return fail(MPCT_EINVAL, "tseg must be strictly ascending with 0 <= tseg[0] and tseg[nseg] <= nit");
  if (p->base != 0 && p->base != 1) return fail(MPCT_EINVAL, "base must be 0 or 1");
  if (!(p->band_rel >= 0.0 && p->band_rel <= 1.7976931348623157e308 && p->band_abs >= 0.0 &&
        p->band_abs <= 1.7976931348623157e308))
    return fail(MPCT_EINVAL, "band_rel and band_abs must be finite and >= 0, not NaN");
  if (!(p->rise_lo >= 0.0 && p->rise_lo <= p->rise_hi && p->rise_hi <= 1.0))  // a NaN fails a comparison
    return fail(MPCT_EINVAL, "rise_lo and rise_hi must satisfy 0 <= rise_lo <= rise_hi <= 1");
  *sp = SegParams{};
  sp->nseg = p->nseg, sp->base = p->base;
  // the unused boundaries repeat the last one: no segment of theirs exists
  for (int g = 0; g <= kSegMax; ++g) sp->tseg[g] = p->tseg[std::min<int>(g, p->nseg)];
  sp->band_rel = p->band_rel, sp->band_abs = p->band_abs, sp->rise_lo = p->rise_lo, sp->rise_hi = p->rise_hi;
  return MPCT_OK;
}

static int seg_check_out(int64_t S, int32_t my, int32_t nu, int32_t nseg, const mpct_segment_result* out, bool have_y,
                         bool have_u) {
  if (!out) return fail(MPCT_EINVAL, "no output pointer in mpct_segment_result");
  const SegOut so = seg_out(out);
  if (!so.any_y() && !so.any_u()) return fail(MPCT_EINVAL, "no output pointer in mpct_segment_result");
  if (so.any_y() && (my < 1 || (S > 0 && !have_y)))
    return fail(MPCT_EINVAL, "an output-row field needs my >= 1 and the trajectories y and r");
  if (so.any_u() && (nu < 1 || (S > 0 && !have_u)))
    return fail(MPCT_EINVAL, "an input-row field needs nu >= 1 and the trajectory u");
  // S * my <= 2^31 * 2^31 holds in int64 only below these guards: compare by division
  if ((my > 0 && S > kIndexMaxRows / ((int64_t)my * nseg)) || (nu > 0 && S > kIndexMaxRows / ((int64_t)nu * nseg)))
    return fail(MPCT_ERANGE, "S*my*nseg or S*nu*nseg exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int seg_check(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my, int32_t nu,
                     int32_t nit, const mpct_segment_params* p, const mpct_segment_result* out, SegParams* sp) {
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (S < 0 || my < 0 || nu < 0 || nit < 1) return fail(MPCT_EINVAL, "bad shape: S < 0, my < 0, nu < 0 or nit < 1");
  if (nref < 1) return fail(MPCT_EINVAL, "nref < 1");
  if (S % nref != 0) return fail(MPCT_EINVAL, "S must be a multiple of nref");
  const int rc = seg_resolve(nit, p, sp);
  if (rc) return rc;
  return seg_check_out(S, my, nu, p->nseg, out, y && r, u != nullptr);
}

static int32_t seg_launch(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                          int32_t nu, int32_t nit, const SegParams& sp, const SegOut& so, hipStream_t stream) {
  if (S == 0) return MPCT_OK;
  std::string err;
  const int rc = launch_segment_indices(y, u, r, S, nref, my, nu, nit, sp, so, stream, &err);
  return rc ? fail(MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_reference_segments(const double* r, int32_t nref, int32_t my, int32_t nit, const int32_t* extra,
                                           int32_t nextra, int32_t max_seg, int32_t* tseg_out, int32_t* nseg) {
  if (!r || !tseg_out || !nseg) return fail(MPCT_EINVAL, "null pointer: r, tseg_out and nseg are needed");
  if (nref < 1 || my < 1 || nit < 1) return fail(MPCT_EINVAL, "bad shape: nref < 1, my < 1 or nit < 1");
  if (max_seg < 1) return fail(MPCT_EINVAL, "max_seg < 1");
  if (nextra < 0 || (nextra > 0 && !extra)) return fail(MPCT_EINVAL, "nextra < 0, or extra samples without a list");
  for (int k = 0; k < nextra; ++k)
    if (extra[k] < 0 || extra[k] > nit) return fail(MPCT_EINVAL, "an extra sample lies outside [0, nit]");
  std::vector<char> cut((size_t)nit + 1, 0);
  cut[0] = cut[nit] = 1;
  for (int k = 0; k < nextra; ++k) cut[extra[k]] = 1;
  for (int64_t row = 0; row < (int64_t)nref * my; ++row) {
    const double* rr = r + row * nit;
    if (!std::isfinite(rr[0])) return fail(MPCT_EINVAL, "the reference holds a non-finite sample");
    for (int t = 1; t < nit; ++t) {
      if (!std::isfinite(rr[t])) return fail(MPCT_EINVAL, "the reference holds a non-finite sample");
      if (rr[t] != rr[t - 1]) cut[t] = 1;
    }
  }
  int64_t n = 0;
  for (int t = 0; t <= nit; ++t) n += cut[t];
  if (n - 1 > max_seg) return fail(MPCT_ERANGE, "the reference has more than max_seg segments");
  int k = 0;
  for (int t = 0; t <= nit; ++t)
    if (cut[t]) tseg_out[k++] = t;
  *nseg = k - 1;
  return MPCT_OK;
}

extern "C" int32_t mpct_segment_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                               int32_t my, int32_t nu, int32_t nit, const mpct_segment_params* params,
                                               const mpct_segment_result* out, void* stream) {
  SegParams sp;
  const int rc = seg_check(y, u, r, S, nref, my, nu, nit, params, out, &sp);
  if (rc) return rc;
  return seg_launch(y, u, r, S, nref, my, nu, nit, sp, seg_out(out), static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_segment_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                        int32_t my, int32_t nu, int32_t nit, const mpct_segment_params* params,
                                        int32_t device, const mpct_segment_result* out) {
  SegParams sp;
  int rc = seg_check(y, u, r, S, nref, my, nu, nit, params, out, &sp);
  if (rc) return rc;
  if (S == 0) return MPCT_OK;  // nothing to stage
  const SegOut ho = seg_out(out);
  CallStage cs{"mpct_segment_indices", "segment staging", "trajectories", "segment records"};
  // y and r travel only behind an output-row field, u only behind an input-row field
  const int s_y = cs.in(ho.any_y() ? y : nullptr, (size_t)S * my * nit * 8),
            s_u = cs.in(ho.any_u() ? u : nullptr, (size_t)S * nu * nit * 8),
            s_r = cs.in(ho.any_y() ? r : nullptr, (size_t)nref * my * nit * 8);
  int slot0 = -1;
  each_seg_field(*out, my, nu, [&](int, void* host, int w, int esz) {
    const int k = cs.out(host, (size_t)S * w * sp.nseg * esz);
    if (slot0 < 0) slot0 = k;
  });
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    const mpct_segment_result dv = seg_slots(cs, slot0);
    rc = seg_launch(cs.at<double>(s_y), cs.at<double>(s_u), cs.at<double>(s_r), S, nref, my, nu, nit, sp, seg_out(&dv), cs.st);
  }
  return cs.close(rc);
}

// the argument checks of the two scoring entries, in the header's order; nothing here touches a device
static int check_eval_segments(mpct_scenario* s, const Batch& b, const mpct_opts* opts, const mpct_segment_params* p,
                               const mpct_result* res, const mpct_segment_result* out, SegParams* sp) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (res && (res->y || res->u || res->ys || res->uopt))
    return fail(MPCT_EINVAL, "the trajectory pointers of res must be NULL: the trajectories stay on the device");
  const mpct_result any{};
  int rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = seg_resolve(s->nit, p, sp);
  if (rc) return rc;
  return seg_check_out(b.C * b.nref, s->my, s->nu, p->nseg, out, true, true);
}

static int launch_segments(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const SegParams& sp,
                           const mpct_result* res, const mpct_segment_result* out, hipStream_t stream) {
  const SegOut so = seg_out(out);
  return walk_chunks(s, cx, b, opts, res, stream, [&](const double* y, const double* u, int64_t n, int64_t s0) {
    return seg_launch(y, u, b.r, n * b.nref, b.nref, s->my, s->nu, s->nit, sp, so.from(s0, s->my, s->nu, sp.nseg), stream);
  });
}

extern "C" int32_t mpct_eval_segment_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                    const double* delta, const double* lambda, int32_t nref,
                                                    const double* r, const double* v, const mpct_opts* opts,
                                                    const mpct_segment_params* params, mpct_result* res,
                                                    const mpct_segment_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  SegParams sp;
  int rc = check_eval_segments(s, b, opts, params, res, out, &sp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_segments(s, cx, b, opts, sp, res, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_segment_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                             const double* delta, const double* lambda, int32_t nref, const double* r,
                                             const double* v, const mpct_opts* opts, const mpct_segment_params* params,
                                             mpct_result* res, const mpct_segment_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  SegParams sp;
  int rc = check_eval_segments(s, b, opts, params, res, out, &sp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  // host buffers in, the records out on the context's own stream, staged as mpct_eval_indices does: slots
  // 0..9 the fields of `res` (its six cost fields on the device with a `res`, its trajectories never),
  // 10..24 the segment fields that are asked for
  const size_t S = (size_t)(C * nref);
  HostStage hs(s, cx, C);
  mpct_result hres = res ? *res : mpct_result{};
  int k = 0;
  each_field(hres, s->my, s->nu, s->nit, [&](auto* host, int64_t w) {
    hs.keep(host, S * w * sizeof(*host), res && k < 6);
    ++k;
  });
  each_seg_field(*out, s->my, s->nu, [&](int, void* host, int w, int esz) { hs.want(host, S * w * sp.nseg * esz); });
  rc = hs.upload(s, b);
  if (rc) return rc;
  mpct_result dres{};
  k = 0;
  each_field(dres, s->my, s->nu, s->nit, [&](auto*& dev, int64_t) { hs.bind(k++, dev); });
  const mpct_segment_result dout = seg_slots(hs, 10);
  rc = launch_segments(s, cx, hs.dev, opts, sp, res ? &dres : nullptr, &dout, hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

// the argument checks of the two robust segment entries, in the header's order; nothing here touches a device
static int check_robust_segments(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                                 const mpct_segment_params* p, int32_t nsel, const int32_t* fields, int32_t nlev,
                                 const double* levels, const mpct_robust_result* base, const mpct_draw_stats_result* out,
                                 SegParams* sp) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (nsel < 1 || nsel > 15 || !fields) return fail(MPCT_EINVAL, "nsel must be 1 .. 15 with a field list");
  unsigned seen = 0;
  for (int q = 0; q < nsel; ++q) {
    if (fields[q] < MPCT_SX_IAE || fields[q] > MPCT_SX_U_HI) return fail(MPCT_EINVAL, "field id out of range");
    if (seen & (1u << fields[q])) return fail(MPCT_EINVAL, "field id repeated");
    seen |= 1u << fields[q];
  }
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: the statistics need at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  const bool any_base = base && (base->mean || base->worst || base->n_failed || base->worst_draw || base->status);
  const bool any_out = out && stats_out(out).any();
  if (!any_base && !any_out) return fail(MPCT_EINVAL, "every output pointer of base and out is NULL");
  if (base && base->J1) return fail(MPCT_EINVAL, "base->J1 must be NULL: the sample lives per chunk");
  if (nlev == 0 && out && stats_out(out).any_level()) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  const mpct_result any{};
  rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = seg_resolve(s->nit, p, sp);
  if (rc) return rc;
  if (b.nref > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "nref > MPCT_TAIL_MAX_DRAWS (4096): the kernel's LDS holds no more draws");
  const int64_t S = b.C * b.nref;
  if (S > kIndexMaxRows / ((int64_t)s->my * p->nseg) || S > kIndexMaxRows / ((int64_t)s->nu * p->nseg))
    return fail(MPCT_ERANGE, "C*nref*my*nseg or C*nref*nu*nseg exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int launch_robust_segments(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                                  const SegParams& sp, int32_t nsel, const int32_t* fields, int32_t nlev,
                                  const double* levels, const RobustOut& base, const DrawStatsOut& out, hipStream_t stream) {
  return walk_robust_chunks(
      s, cx, b, j_bound, opts, MPCT_SX_TV, sp.nseg, kSegInts, nsel, fields, nlev, levels, base, out, stream,
      [&](void* const* rec, const double* y, const double* u, int64_t S) {
        const SegOut so{(double*)rec[0], (double*)rec[1], (double*)rec[2],  (double*)rec[3],  (int*)rec[4],
                        (double*)rec[5], (double*)rec[6], (double*)rec[7],  (int*)rec[8],     (int*)rec[9],
                        (double*)rec[10], (double*)rec[11], (double*)rec[12], (double*)rec[13], (double*)rec[14]};
        return seg_launch(y, u, b.r, S, b.nref, s->my, s->nu, s->nit, sp, so, stream);
      });
}

extern "C" int32_t mpct_eval_robust_segment_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2,
                                                           const int32_t* Nu, const double* delta, const double* lambda,
                                                           int32_t nref, const double* r, const double* v, double j_bound,
                                                           const mpct_opts* opts, const mpct_segment_params* params,
                                                           int32_t nsel, const int32_t* fields, int32_t nlev,
                                                           const double* levels, mpct_robust_result* base,
                                                           const mpct_draw_stats_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  SegParams sp;
  int rc = check_robust_segments(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &sp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const RobustOut ro = base ? RobustOut{base->mean, base->worst, base->n_failed, base->worst_draw, base->status} : RobustOut{};
  return launch_robust_segments(s, cx, b, j_bound, opts, sp, nsel, fields, nlev, levels, ro,
                                out ? stats_out(out) : DrawStatsOut{}, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_robust_segment_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                    const double* delta, const double* lambda, int32_t nref,
                                                    const double* r, const double* v, double j_bound,
                                                    const mpct_opts* opts, const mpct_segment_params* params,
                                                    int32_t nsel, const int32_t* fields, int32_t nlev,
                                                    const double* levels, mpct_robust_result* base,
                                                    const mpct_draw_stats_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  SegParams sp;
  int rc = check_robust_segments(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &sp);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  size_t W = 0;
  for (int q = 0; q < nsel; ++q) W += (size_t)(fields[q] < MPCT_SX_TV ? s->my : s->nu) * sp.nseg;
  return robust_stats_host(s, cx, b, W, nlev, base, out, [&](HostStage& hs, const RobustOut& ro, const DrawStatsOut& dv) {
    return launch_robust_segments(s, cx, hs.dev, j_bound, opts, sp, nsel, fields, nlev, levels, ro, dv, hs.st);
  });
}

// ------------------------------------------------------------------------------------------
// oscillation indices per setpoint segment and their statistics over the draws (osc_indices.hip;
// include/mpct.h): the segment family's entries with mpct_osc_params and seven fields

static OscOut osc_out(const mpct_osc_result* o) {
  return OscOut{o->ncross, o->decay, o->period, o->a_last, o->nmove, o->nrev, o->t_rev};
}
// the bits of the int32 fields, and the fields of an mpct_osc_result in the struct's order, each with its host
// pointer, its width per simulation and segment and its element size
constexpr int kOscFields = 7;
constexpr unsigned kOscInts =
    1u << MPCT_OX_NCROSS | 1u << MPCT_OX_PERIOD | 1u << MPCT_OX_NMOVE | 1u << MPCT_OX_NREV | 1u << MPCT_OX_T_REV;
template <class F>
static void each_osc_field(const mpct_osc_result& o, int my, int nu, F f) {
  void* const host[kOscFields] = {o.ncross, o.decay, o.period, o.a_last, o.nmove, o.nrev, o.t_rev};
  for (int id = 0; id < kOscFields; ++id) f(id, host[id], id < MPCT_OX_NMOVE ? my : nu, (kOscInts >> id & 1u) ? 4 : 8);
}
// the device-side record from the slots slot0 .. slot0 + 6 of a stage
template <class Stage>
static mpct_osc_result osc_slots(const Stage& st, int slot0) {
  auto dd = [&](int id) { return st.template at<double>(slot0 + id); };
  auto di = [&](int id) { return st.template at<int32_t>(slot0 + id); };
  return mpct_osc_result{di(0), dd(1), di(2), dd(3), di(4), di(5), di(6)};
}

// the checks on the parameters from nseg to rev_tol, in the header's order, and the kernel's by-value
// parameters.  The boundaries, the base rule and the band are the segment family's: seg_resolve checks them, with
// rise levels that always pass
static int osc_resolve(int32_t nit, const mpct_osc_params* p, OscParams* op) {
  const mpct_segment_params as_seg{p->nseg, p->tseg, p->base, p->band_rel, p->band_abs, 0.0, 1.0};
  SegParams sp;
  const int rc = seg_resolve(nit, &as_seg, &sp);
  if (rc) return rc;
  if (!(p->rev_tol >= 0.0 && p->rev_tol <= 1.7976931348623157e308))
    return fail(MPCT_EINVAL, "rev_tol must be finite and >= 0, not NaN");
  *op = OscParams{};
  op->nseg = sp.nseg, op->base = sp.base;
  for (int g = 0; g <= kSegMax; ++g) op->tseg[g] = sp.tseg[g];
  op->band_rel = sp.band_rel, op->band_abs = sp.band_abs, op->rev_tol = p->rev_tol;
  return MPCT_OK;
}

static int osc_check_out(int64_t S, int32_t my, int32_t nu, int32_t nseg, const mpct_osc_result* out, bool have_y,
                         bool have_u) {
  if (!out) return fail(MPCT_EINVAL, "no output pointer in mpct_osc_result");
  const OscOut oo = osc_out(out);
  if (!oo.any_y() && !oo.any_u()) return fail(MPCT_EINVAL, "no output pointer in mpct_osc_result");
  if (oo.any_y() && (my < 1 || (S > 0 && !have_y)))
    return fail(MPCT_EINVAL, "an output-row field needs my >= 1 and the trajectories y and r");
  if (oo.any_u() && (nu < 1 || (S > 0 && !have_u)))
    return fail(MPCT_EINVAL, "an input-row field needs nu >= 1 and the trajectory u");
  // S * my <= 2^31 * 2^31 holds in int64 only below these guards: compare by division
  if ((my > 0 && S > kIndexMaxRows / ((int64_t)my * nseg)) || (nu > 0 && S > kIndexMaxRows / ((int64_t)nu * nseg)))
    return fail(MPCT_ERANGE, "S*my*nseg or S*nu*nseg exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int osc_check(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my, int32_t nu,
                     int32_t nit, const mpct_osc_params* p, const mpct_osc_result* out, OscParams* op) {
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (S < 0 || my < 0 || nu < 0 || nit < 1) return fail(MPCT_EINVAL, "bad shape: S < 0, my < 0, nu < 0 or nit < 1");
  if (nref < 1) return fail(MPCT_EINVAL, "nref < 1");
  if (S % nref != 0) return fail(MPCT_EINVAL, "S must be a multiple of nref");
  const int rc = osc_resolve(nit, p, op);
  if (rc) return rc;
  return osc_check_out(S, my, nu, p->nseg, out, y && r, u != nullptr);
}

static int32_t osc_launch(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                          int32_t nu, int32_t nit, const OscParams& op, const OscOut& oo, hipStream_t stream) {
  if (S == 0) return MPCT_OK;
  std::string err;
  const int rc = launch_osc_indices(y, u, r, S, nref, my, nu, nit, op, oo, stream, &err);
  return rc ? fail(MPCT_EDEVICE, err) : MPCT_OK;
}

extern "C" int32_t mpct_osc_indices_device(const double* y, const double* u, const double* r, int64_t S, int32_t nref,
                                           int32_t my, int32_t nu, int32_t nit, const mpct_osc_params* params,
                                           const mpct_osc_result* out, void* stream) {
  OscParams op;
  const int rc = osc_check(y, u, r, S, nref, my, nu, nit, params, out, &op);
  if (rc) return rc;
  return osc_launch(y, u, r, S, nref, my, nu, nit, op, osc_out(out), static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_osc_indices(const double* y, const double* u, const double* r, int64_t S, int32_t nref, int32_t my,
                                    int32_t nu, int32_t nit, const mpct_osc_params* params, int32_t device,
                                    const mpct_osc_result* out) {
  OscParams op;
  int rc = osc_check(y, u, r, S, nref, my, nu, nit, params, out, &op);
  if (rc) return rc;
  if (S == 0) return MPCT_OK;  // nothing to stage
  const OscOut ho = osc_out(out);
  CallStage cs{"mpct_osc_indices", "oscillation staging", "trajectories", "oscillation records"};
  // y and r travel only behind an output-row field, u only behind an input-row field
  const int s_y = cs.in(ho.any_y() ? y : nullptr, (size_t)S * my * nit * 8),
            s_u = cs.in(ho.any_u() ? u : nullptr, (size_t)S * nu * nit * 8),
            s_r = cs.in(ho.any_y() ? r : nullptr, (size_t)nref * my * nit * 8);
  int slot0 = -1;
  each_osc_field(*out, my, nu, [&](int, void* host, int w, int esz) {
    const int k = cs.out(host, (size_t)S * w * op.nseg * esz);
    if (slot0 < 0) slot0 = k;
  });
  rc = cs.open(device);
  if (rc == MPCT_OK) {
    const mpct_osc_result dv = osc_slots(cs, slot0);
    rc = osc_launch(cs.at<double>(s_y), cs.at<double>(s_u), cs.at<double>(s_r), S, nref, my, nu, nit, op, osc_out(&dv), cs.st);
  }
  return cs.close(rc);
}

// the argument checks of the two scoring entries, in the header's order; nothing here touches a device
static int check_eval_osc(mpct_scenario* s, const Batch& b, const mpct_opts* opts, const mpct_osc_params* p,
                          const mpct_result* res, const mpct_osc_result* out, OscParams* op) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (res && (res->y || res->u || res->ys || res->uopt))
    return fail(MPCT_EINVAL, "the trajectory pointers of res must be NULL: the trajectories stay on the device");
  const mpct_result any{};
  int rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = osc_resolve(s->nit, p, op);
  if (rc) return rc;
  return osc_check_out(b.C * b.nref, s->my, s->nu, p->nseg, out, true, true);
}

static int launch_osc(mpct_scenario* s, DevCtx* cx, const Batch& b, const mpct_opts* opts, const OscParams& op,
                      const mpct_result* res, const mpct_osc_result* out, hipStream_t stream) {
  const OscOut oo = osc_out(out);
  return walk_chunks(s, cx, b, opts, res, stream, [&](const double* y, const double* u, int64_t n, int64_t s0) {
    return osc_launch(y, u, b.r, n * b.nref, b.nref, s->my, s->nu, s->nit, op, oo.from(s0, s->my, s->nu, op.nseg), stream);
  });
}

extern "C" int32_t mpct_eval_osc_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                const double* delta, const double* lambda, int32_t nref, const double* r,
                                                const double* v, const mpct_opts* opts, const mpct_osc_params* params,
                                                mpct_result* res, const mpct_osc_result* out, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  OscParams op;
  int rc = check_eval_osc(s, b, opts, params, res, out, &op);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  return launch_osc(s, cx, b, opts, op, res, out, static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_osc_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                         const double* delta, const double* lambda, int32_t nref, const double* r,
                                         const double* v, const mpct_opts* opts, const mpct_osc_params* params,
                                         mpct_result* res, const mpct_osc_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  OscParams op;
  int rc = check_eval_osc(s, b, opts, params, res, out, &op);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  // staged as mpct_eval_segment_indices does: slots 0..9 the fields of `res`, 10..16 the oscillation fields
  // that are asked for
  const size_t S = (size_t)(C * nref);
  HostStage hs(s, cx, C);
  mpct_result hres = res ? *res : mpct_result{};
  int k = 0;
  each_field(hres, s->my, s->nu, s->nit, [&](auto* host, int64_t w) {
    hs.keep(host, S * w * sizeof(*host), res && k < 6);
    ++k;
  });
  each_osc_field(*out, s->my, s->nu, [&](int, void* host, int w, int esz) { hs.want(host, S * w * op.nseg * esz); });
  rc = hs.upload(s, b);
  if (rc) return rc;
  mpct_result dres{};
  k = 0;
  each_field(dres, s->my, s->nu, s->nit, [&](auto*& dev, int64_t) { hs.bind(k++, dev); });
  const mpct_osc_result dout = osc_slots(hs, 10);
  rc = launch_osc(s, cx, hs.dev, opts, op, res ? &dres : nullptr, &dout, hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

// the argument checks of the two robust oscillation entries, in the header's order; nothing here touches a device
static int check_robust_osc(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts,
                            const mpct_osc_params* p, int32_t nsel, const int32_t* fields, int32_t nlev,
                            const double* levels, const mpct_robust_result* base, const mpct_draw_stats_result* out,
                            OscParams* op) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (!p) return fail(MPCT_EINVAL, "null params");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the index entries are closed-loop only: open_loop must be 0");
  if (nsel < 1 || nsel > kOscFields || !fields) return fail(MPCT_EINVAL, "nsel must be 1 .. 7 with a field list");
  unsigned seen = 0;
  for (int q = 0; q < nsel; ++q) {
    if (fields[q] < MPCT_OX_NCROSS || fields[q] > MPCT_OX_T_REV) return fail(MPCT_EINVAL, "field id out of range");
    if (seen & (1u << fields[q])) return fail(MPCT_EINVAL, "field id repeated");
    seen |= 1u << fields[q];
  }
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: the statistics need at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  const bool any_base = base && (base->mean || base->worst || base->n_failed || base->worst_draw || base->status);
  const bool any_out = out && stats_out(out).any();
  if (!any_base && !any_out) return fail(MPCT_EINVAL, "every output pointer of base and out is NULL");
  if (base && base->J1) return fail(MPCT_EINVAL, "base->J1 must be NULL: the sample lives per chunk");
  if (nlev == 0 && out && stats_out(out).any_level()) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  const mpct_result any{};
  rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  rc = osc_resolve(s->nit, p, op);
  if (rc) return rc;
  if (b.nref > MPCT_TAIL_MAX_DRAWS) return fail(MPCT_ERANGE, "nref > MPCT_TAIL_MAX_DRAWS (4096): the kernel's LDS holds no more draws");
  const int64_t S = b.C * b.nref;
  if (S > kIndexMaxRows / ((int64_t)s->my * p->nseg) || S > kIndexMaxRows / ((int64_t)s->nu * p->nseg))
    return fail(MPCT_ERANGE, "C*nref*my*nseg or C*nref*nu*nseg exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

static int launch_robust_osc(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                             const OscParams& op, int32_t nsel, const int32_t* fields, int32_t nlev, const double* levels,
                             const RobustOut& base, const DrawStatsOut& out, hipStream_t stream) {
  return walk_robust_chunks(s, cx, b, j_bound, opts, MPCT_OX_NMOVE, op.nseg, kOscInts, nsel, fields, nlev, levels, base, out,
                            stream, [&](void* const* rec, const double* y, const double* u, int64_t S) {
                              const OscOut oo{(int*)rec[0], (double*)rec[1], (int*)rec[2], (double*)rec[3],
                                              (int*)rec[4], (int*)rec[5],    (int*)rec[6]};
                              return osc_launch(y, u, b.r, S, b.nref, s->my, s->nu, s->nit, op, oo, stream);
                            });
}

extern "C" int32_t mpct_eval_robust_osc_indices_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                       const double* delta, const double* lambda, int32_t nref,
                                                       const double* r, const double* v, double j_bound,
                                                       const mpct_opts* opts, const mpct_osc_params* params, int32_t nsel,
                                                       const int32_t* fields, int32_t nlev, const double* levels,
                                                       mpct_robust_result* base, const mpct_draw_stats_result* out,
                                                       void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  OscParams op;
  int rc = check_robust_osc(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &op);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const RobustOut ro = base ? RobustOut{base->mean, base->worst, base->n_failed, base->worst_draw, base->status} : RobustOut{};
  return launch_robust_osc(s, cx, b, j_bound, opts, op, nsel, fields, nlev, levels, ro, out ? stats_out(out) : DrawStatsOut{},
                           static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_robust_osc_indices(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                const double* delta, const double* lambda, int32_t nref, const double* r,
                                                const double* v, double j_bound, const mpct_opts* opts,
                                                const mpct_osc_params* params, int32_t nsel, const int32_t* fields,
                                                int32_t nlev, const double* levels, mpct_robust_result* base,
                                                const mpct_draw_stats_result* out) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  OscParams op;
  int rc = check_robust_osc(s, b, j_bound, opts, params, nsel, fields, nlev, levels, base, out, &op);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  size_t W = 0;
  for (int q = 0; q < nsel; ++q) W += (size_t)(fields[q] < MPCT_OX_NMOVE ? s->my : s->nu) * op.nseg;
  return robust_stats_host(s, cx, b, W, nlev, base, out, [&](HostStage& hs, const RobustOut& ro, const DrawStatsOut& dv) {
    return launch_robust_osc(s, cx, hs.dev, j_bound, opts, op, nsel, fields, nlev, levels, ro, dv, hs.st);
  });
}

// ------------------------------------------------------------------------------------------
// trajectory envelopes over the plant draws (envelope.hip; include/mpct.h)

static EnvSpreadOut spread_out(const mpct_envelope_spread* o) {
  return o ? EnvSpreadOut{o->spread, o->spread_max, o->t_spread_max} : EnvSpreadOut{};
}

// the checks both kinds of entry share from t0 on, in the header's order; base: the robust entries' optional record
static int envelope_check_out(int32_t nit, int32_t t0, int32_t nlev, const double* levels, const mpct_robust_result* base,
                              const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                              const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u) {
  if (t0 < 0 || t0 >= nit) return fail(MPCT_EINVAL, "t0 must lie in [0, nit)");
  const int rc = stats_check_levels(nlev, levels);
  if (rc) return rc;
  const DrawStatsOut oy = out_y ? stats_out(out_y) : DrawStatsOut{}, ou = out_u ? stats_out(out_u) : DrawStatsOut{};
  if ((spread_out(spread_y).any() && !(oy.lo && oy.hi)) || (spread_out(spread_u).any() && !(ou.lo && ou.hi)))
    return fail(MPCT_EINVAL, "a spread pointer needs the lo and hi of its side: the spread reads them");
  const bool any_base = base && (base->mean || base->worst || base->n_failed || base->worst_draw || base->status);
  if (!any_base && !oy.any() && !ou.any()) return fail(MPCT_EINVAL, "every output pointer is NULL");
  if (base && base->J1) return fail(MPCT_EINVAL, "base->J1 must be NULL: the sample lives per chunk");
  if (nlev == 0 && (oy.any_level() || ou.any_level())) return fail(MPCT_EINVAL, "quantile, cvar and q_draw need nlev >= 1");
  return MPCT_OK;
}

static int envelope_check_range(int64_t C, int32_t D, int32_t my, int32_t nu, int32_t nit, int32_t nlev) {
  if (nlev > 0 && D > MPCT_TAIL_MAX_DRAWS)
    return fail(MPCT_ERANGE, "D > MPCT_TAIL_MAX_DRAWS (4096) with levels: the kernel's LDS holds no more draws");
  if (C * (int64_t)my * nit > kIndexMaxRows || C * (int64_t)nu * nit > kIndexMaxRows)
    return fail(MPCT_ERANGE, "C*my*nit or C*nu*nit exceeds MPCT_INDEX_MAX_ROWS");
  return MPCT_OK;
}

// the argument checks of the two stored-trajectory entries, in the header's order; nothing here touches a device
static int envelope_check(const double* y, const double* u, int64_t C, int32_t D, int32_t my, int32_t nu, int32_t nit,
                          int32_t t0, int32_t nlev, const double* levels, const mpct_draw_stats_result* out_y,
                          const mpct_draw_stats_result* out_u, const mpct_envelope_spread* spread_y,
                          const mpct_envelope_spread* spread_u) {
  if (C < 0 || D < 1 || my < 0 || nu < 0 || nit < 1) return fail(MPCT_EINVAL, "bad shape: C < 0, D < 1, my < 0, nu < 0 or nit < 1");
  int rc = envelope_check_out(nit, t0, nlev, levels, nullptr, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  if (out_y && stats_out(out_y).any() && (my < 1 || (C > 0 && !y))) return fail(MPCT_EINVAL, "out_y needs my >= 1 and y");
  if (out_u && stats_out(out_u).any() && (nu < 1 || (C > 0 && !u))) return fail(MPCT_EINVAL, "out_u needs nu >= 1 and u");
  return envelope_check_range(C, D, my, nu, nit, nlev);
}

// test / bench hooks, not part of include/mpct.h.  The largest grid of draw_envelope_kernel in workgroups
// (0: kEnvGridCap): the tests force the workgroups to stride at small sizes with it.  And the draws up to which
// the levels run on the lane kernel (0: kEnvDefaultDlane; at most kEnvLaneMaxDraws): the tests and the bench run
// both kernels on one shape with it
static int32_t g_env_grid = 0, g_env_dlane = 0;
extern "C" int32_t mpct_internal_envelope_grid(int32_t groups) {
  if (groups < 0) return fail(MPCT_EINVAL, "groups < 0");
  g_env_grid = groups;
  return MPCT_OK;
}
extern "C" int32_t mpct_internal_envelope_dlane(int32_t draws) {
  if (draws < 0 || draws > kEnvLaneMaxDraws) return fail(MPCT_EINVAL, "draws must be 0 .. 227");
  g_env_dlane = draws;
  return MPCT_OK;
}

// one side: the table x [C][D][rows * nit], its records and its spread
static int32_t envelope_side(const double* x, const int32_t* alive, int64_t C, int32_t D, int32_t rows, int32_t nit,
                             int32_t t0, int32_t nlev, const double* levels, const DrawStatsOut& out,
                             const EnvSpreadOut& sp, hipStream_t stream) {
  if (!out.any() || C == 0) return MPCT_OK;
  const int m = rows * nit;
  const int dlane = g_env_dlane > 0 ? g_env_dlane : kEnvDefaultDlane;
  if (nlev > 0 && out.any_level() && D > dlane) {
    const int rc = stats_launch(x, MPCT_STAT_F64, alive, C, D, m, nlev, levels, out, m, 0, stream);
    if (rc) return rc;
  } else {
    std::string err;
    if (launch_draw_envelope(x, alive, C, D, m, nlev, levels, out, g_env_grid, stream, &err)) return fail(MPCT_EDEVICE, err);
  }
  std::string err;
  if (launch_envelope_spread(out.lo, out.hi, C * rows, nit, t0, sp, stream, &err)) return fail(MPCT_EDEVICE, err);
  return MPCT_OK;
}

static int32_t envelope_launch(const double* y, const double* u, const int32_t* alive, int64_t C, int32_t D, int32_t my,
                               int32_t nu, int32_t nit, int32_t t0, int32_t nlev, const double* levels,
                               const DrawStatsOut& oy, const DrawStatsOut& ou, const EnvSpreadOut& sy, const EnvSpreadOut& su,
                               hipStream_t stream) {
  const int rc = envelope_side(y, alive, C, D, my, nit, t0, nlev, levels, oy, sy, stream);
  return rc ? rc : envelope_side(u, alive, C, D, nu, nit, t0, nlev, levels, ou, su, stream);
}

extern "C" int32_t mpct_envelope_device(const double* y, const double* u, const int32_t* alive, int64_t C, int32_t D,
                                        int32_t my, int32_t nu, int32_t nit, int32_t t0, int32_t nlev, const double* levels,
                                        const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                        const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u,
                                        void* stream) {
  const int rc = envelope_check(y, u, C, D, my, nu, nit, t0, nlev, levels, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  return envelope_launch(y, u, alive, C, D, my, nu, nit, t0, nlev, levels, out_y ? stats_out(out_y) : DrawStatsOut{},
                         out_u ? stats_out(out_u) : DrawStatsOut{}, spread_out(spread_y), spread_out(spread_u),
                         static_cast<hipStream_t>(stream));
}

// the slots of one side's records and spread in a staging blob: want(host, bytes) reserves one and returns it
template <class Want>
static void envelope_slots(Want want, const mpct_draw_stats_result& o, const mpct_envelope_spread& sp, size_t C, size_t rows,
                           size_t nit, size_t nlev, int* slot) {
  const size_t cols = C * rows * nit, lev = cols * nlev, cr = C * rows;
  slot[0] = want(o.n, cols * 4), slot[1] = want(o.mean, cols * 8), slot[2] = want(o.lo, cols * 8);
  slot[3] = want(o.lo_draw, cols * 4), slot[4] = want(o.hi, cols * 8), slot[5] = want(o.hi_draw, cols * 4);
  slot[6] = want(o.quantile, lev * 8), slot[7] = want(o.cvar, lev * 8), slot[8] = want(o.q_draw, lev * 4);
  slot[9] = want(sp.spread, cr * 8), slot[10] = want(sp.spread_max, cr * 8), slot[11] = want(sp.t_spread_max, cr * 4);
}
template <class Stage>
static DrawStatsOut envelope_dev_out(const Stage& st, const int* slot) {
  return DrawStatsOut{st.template at<int32_t>(slot[0]), st.template at<double>(slot[1]), st.template at<double>(slot[2]),
                      st.template at<int32_t>(slot[3]), st.template at<double>(slot[4]), st.template at<int32_t>(slot[5]),
                      st.template at<double>(slot[6]),  st.template at<double>(slot[7]), st.template at<int32_t>(slot[8])};
}
template <class Stage>
static EnvSpreadOut envelope_dev_spread(const Stage& st, const int* slot) {
  return EnvSpreadOut{st.template at<double>(slot[9]), st.template at<double>(slot[10]), st.template at<int32_t>(slot[11])};
}

extern "C" int32_t mpct_envelope(const double* y, const double* u, const int32_t* alive, int64_t C, int32_t D, int32_t my,
                                 int32_t nu, int32_t nit, int32_t t0, int32_t nlev, const double* levels, int32_t device,
                                 const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                 const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u) {
  int rc = envelope_check(y, u, C, D, my, nu, nit, t0, nlev, levels, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage
  CallStage cs{"mpct_envelope", "envelope staging", "trajectories", "envelopes"};
  const mpct_draw_stats_result hy = out_y ? *out_y : mpct_draw_stats_result{}, hu = out_u ? *out_u : mpct_draw_stats_result{};
  const mpct_envelope_spread py = spread_y ? *spread_y : mpct_envelope_spread{}, pu = spread_u ? *spread_u : mpct_envelope_spread{};
  // a side without a result pointer is not uploaded
  const size_t S = (size_t)C * D;
  const int s_y = cs.in(stats_out(&hy).any() ? y : nullptr, S * my * nit * 8);
  const int s_u = cs.in(stats_out(&hu).any() ? u : nullptr, S * nu * nit * 8), s_alive = cs.in(alive, S * 4);
  int sy[12], su[12];
  auto want = [&](void* host, size_t bytes) { return cs.out(host, bytes); };
  envelope_slots(want, hy, py, (size_t)C, (size_t)my, (size_t)nit, (size_t)nlev, sy);
  envelope_slots(want, hu, pu, (size_t)C, (size_t)nu, (size_t)nit, (size_t)nlev, su);
  rc = cs.open(device);
  if (rc == MPCT_OK)
    rc = envelope_launch(cs.at<double>(s_y), cs.at<double>(s_u), cs.at<int32_t>(s_alive), C, D, my, nu, nit, t0, nlev, levels,
                         envelope_dev_out(cs, sy), envelope_dev_out(cs, su), envelope_dev_spread(cs, sy),
                         envelope_dev_spread(cs, su), cs.st);
  return cs.close(rc);
}

// the argument checks of the two scoring entries, in the header's order; nothing here touches a device
static int check_robust_envelope(mpct_scenario* s, const Batch& b, double j_bound, const mpct_opts* opts, int32_t t0,
                                 int32_t nlev, const double* levels, const mpct_robust_result* base,
                                 const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                 const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (opts && opts->open_loop) return fail(MPCT_EINVAL, "the envelope entries are closed-loop only: open_loop must be 0");
  if (b.nref < 1) return fail(MPCT_EINVAL, "nref < 1: the statistics need at least one draw");
  if (!(j_bound >= 0.0)) return fail(MPCT_EINVAL, "j_bound must be >= 0 (0 = 1e100, +inf allowed), not negative or NaN");
  int rc = envelope_check_out(s->nit, t0, nlev, levels, base, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  const mpct_result any{};
  rc = check_args(s, b, opts, &any);
  if (rc) return rc;
  return envelope_check_range(b.C, b.nref, s->my, s->nu, s->nit, nlev);
}

// enqueue one batch with device pointers on `stream`: the walk of the robust index entries, whose record is the
// chunk's trajectories themselves
static int launch_robust_envelope(mpct_scenario* s, DevCtx* cx, const Batch& b, double j_bound, const mpct_opts* opts,
                                  int32_t t0, int32_t nlev, const double* levels, const RobustOut& base,
                                  const DrawStatsOut& oy, const DrawStatsOut& ou, const EnvSpreadOut& sy, const EnvSpreadOut& su,
                                  hipStream_t stream) {
  const int my = s->my, nu = s->nu, nit = s->nit;
  return walk_draw_chunks(
      s, cx, b, j_bound, opts, base, stream, [](size_t) { return (size_t)0; },
      [](char*, const double*, const double*, int64_t) { return (int)MPCT_OK; },
      [&](char*, const double* y, const double* u, const int32_t* alive, int64_t c0, int64_t n) {
        return (int)envelope_launch(y, u, alive, n, b.nref, my, nu, nit, t0, nlev, levels, oy.from(c0, my * nit, nlev),
                                    ou.from(c0, nu * nit, nlev), sy.from(c0 * my), su.from(c0 * nu), stream);
      });
}

extern "C" int32_t mpct_eval_robust_envelope_device(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                                    const double* delta, const double* lambda, int32_t nref,
                                                    const double* r, const double* v, double j_bound, const mpct_opts* opts,
                                                    int32_t t0, int32_t nlev, const double* levels, mpct_robust_result* base,
                                                    const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                                    const mpct_envelope_spread* spread_y,
                                                    const mpct_envelope_spread* spread_u, void* stream) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_robust_envelope(s, b, j_bound, opts, t0, nlev, levels, base, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to enqueue, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  const RobustOut ro = base ? RobustOut{base->mean, base->worst, base->n_failed, base->worst_draw, base->status} : RobustOut{};
  return launch_robust_envelope(s, cx, b, j_bound, opts, t0, nlev, levels, ro, out_y ? stats_out(out_y) : DrawStatsOut{},
                                out_u ? stats_out(out_u) : DrawStatsOut{}, spread_out(spread_y), spread_out(spread_u),
                                static_cast<hipStream_t>(stream));
}

extern "C" int32_t mpct_eval_robust_envelope(mpct_scenario* s, int64_t C, const int32_t* N2, const int32_t* Nu,
                                             const double* delta, const double* lambda, int32_t nref, const double* r,
                                             const double* v, double j_bound, const mpct_opts* opts, int32_t t0, int32_t nlev,
                                             const double* levels, mpct_robust_result* base,
                                             const mpct_draw_stats_result* out_y, const mpct_draw_stats_result* out_u,
                                             const mpct_envelope_spread* spread_y, const mpct_envelope_spread* spread_u) {
  const Batch b{C, N2, Nu, delta, lambda, nref, r, v};
  int rc = check_robust_envelope(s, b, j_bound, opts, t0, nlev, levels, base, out_y, out_u, spread_y, spread_u);
  if (rc) return rc;
  if (C == 0) return MPCT_OK;  // nothing to stage, no device needed
  DevCtx* cx = nullptr;
  rc = ctx_for(s, opts, &cx);
  if (rc) return rc;
  // host buffers in, the records out on the context's own stream, staged as robust_stats_host does: every
  // field lives on the device only where it is asked for
  const size_t Cn = (size_t)C, cm = Cn * s->my * 8;
  const mpct_robust_result hb = base ? *base : mpct_robust_result{};
  const mpct_draw_stats_result hy = out_y ? *out_y : mpct_draw_stats_result{}, hu = out_u ? *out_u : mpct_draw_stats_result{};
  const mpct_envelope_spread py = spread_y ? *spread_y : mpct_envelope_spread{}, pu = spread_u ? *spread_u : mpct_envelope_spread{};
  HostStage hs(s, cx, C);
  const int s_mean = hs.want(hb.mean, cm), s_worst = hs.want(hb.worst, cm), s_nf = hs.want(hb.n_failed, Cn * 4),
            s_wd = hs.want(hb.worst_draw, Cn * 4), s_st = hs.want(hb.status, Cn * 4);
  int sy[12], su[12];
  auto want = [&](void* host, size_t bytes) { return hs.want(host, bytes); };
  envelope_slots(want, hy, py, Cn, (size_t)s->my, (size_t)s->nit, (size_t)nlev, sy);
  envelope_slots(want, hu, pu, Cn, (size_t)s->nu, (size_t)s->nit, (size_t)nlev, su);
  rc = hs.upload(s, b);
  if (rc) return rc;
  const RobustOut ro{hs.at<double>(s_mean), hs.at<double>(s_worst), hs.at<int32_t>(s_nf), hs.at<int32_t>(s_wd),
                     hs.at<int32_t>(s_st)};
  rc = launch_robust_envelope(s, cx, hs.dev, j_bound, opts, t0, nlev, levels, ro, envelope_dev_out(hs, sy),
                              envelope_dev_out(hs, su), envelope_dev_spread(hs, sy), envelope_dev_spread(hs, su), hs.st);
  if (rc) return hs.abandon(rc);
  return hs.finish();
}

static int32_t copy_name(const std::string& nm, char* buf, int32_t cap) {
  if (buf && cap > 0) {
    const size_t n = std::min<size_t>(nm.size(), (size_t)cap - 1);
    std::memcpy(buf, nm.data(), n);
    buf[n] = '\0';
  }
  return (int32_t)nm.size();
}

static std::string per_simulation_instance(const mpct_scenario* s, bool ext) {
  if (s->nmpc && !s->nmv.empty())
    return "nmpc_closed_loop_kernel<..., plant variants> (QP-size x LDS-tier class launches)";
  if (s->nmpc) return "nmpc_closed_loop_kernel (QP-size x LDS-tier class launches)";
  if (s->mdband && s->est)
    return "mdband_closed_loop_kernel (QP-size x LDS-tier class launches) + output-bias estimator";
  if (s->mdband) return "mdband_closed_loop_kernel (QP-size x LDS-tier class launches)";
  return closed_loop_instance(dev_scenario(s), s->nu * s->numax, ext);
}

extern "C" int32_t mpct_robust_instance(const mpct_scenario* s, const mpct_opts* opts, char* buf, int32_t cap) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (opts && (opts->open_loop || opts->want_traj))
    return fail(MPCT_EINVAL, "robust scoring is cost-only: open_loop and want_traj must be 0");
  std::string nm;
  if (!s->nmpc && !s->mdband && dtc_robust_eligible(dev_scenario(s), 1)) {
    nm = "dtc_robust_kernel<16>";
    if (s->nu * s->numax > 16) nm += " + dtc_robust_kernel<32>";
  } else {
    nm = per_simulation_instance(s, false) + " + robust_reduce_kernel";
  }
  return copy_name(nm, buf, cap);
}

extern "C" int32_t mpct_kernel_instance(const mpct_scenario* s, const mpct_opts* opts, char* buf, int32_t cap) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  const bool ext = opts && (opts->open_loop || opts->want_traj);
  return copy_name(per_simulation_instance(s, ext), buf, cap);
}

static int64_t lds_bytes_ext(const mpct_scenario* s, int32_t N2, int32_t Nu, bool ext) {
  if (!s) return fail(MPCT_EINVAL, "null scenario");
  if (s->nmpc) return nmpc_lds_bytes(s->nu * Nu, N2);
  const DevScenario ds = dev_scenario(s);
  // an estimator scenario always carries the second (parallel model) copy
  return s->mdband ? mdband_lds_bytes(ds, N2, Nu, ext || s->est ? 2 : 1) : lds_bytes_for(ds, N2, Nu, ext);
}

extern "C" int64_t mpct_lds_bytes(const mpct_scenario* s, int32_t N2, int32_t Nu) {
  return lds_bytes_ext(s, N2, Nu, true);
}

extern "C" int64_t mpct_lds_bytes_opts(const mpct_scenario* s, const mpct_opts* opts, int32_t N2, int32_t Nu) {
  return lds_bytes_ext(s, N2, Nu, opts && (opts->open_loop || opts->want_traj));
}
