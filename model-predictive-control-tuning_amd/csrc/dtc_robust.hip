// dtc_robust.hip — robust scoring over plant draws (mpct_eval_robust, include/mpct.h):
// per-candidate statistics of the D closed loops of one candidate, computed on the device.
//
//   * robust_reduce_kernel: the generic path.  The scenario's per-simulation instance has written
//     J1 / status of all C x D simulations; one wave per candidate reduces its D records
//     (robust_reduce.h).
//   * dtc_robust_kernel<16 | 32>: the fused path of small_dtc scenarios (dtc_small.hip's
//     eligibility, cost-only).  One workgroup of kRobustW waves owns one CANDIDATE: wave 0 builds the
//     first-move gain Km and the filter coefficients once (DTC_GPC_WW.m:98-105 computes K before its
//     loop, not once per draw), every wave then runs draws w, w + kRobustW, .. through the step loop
//     of dtc_small_kernel (dtc_step.h) on its own copy of the loop state, and after a workgroup
//     barrier wave 0 reduces the D records left in LDS with the same robust_reduce.
//   * robust_classify_kernel: the per-class candidate lists of the fused path, in dispatch order.
//     The workgroups of a class launch stride over their class's list, so none is started for a
//     candidate of the other class; skipped / bad-horizon candidates get their records here.
//   * robust_tail_kernel: quantiles and tail means of the total cost over the draws
//     (mpct_eval_robust_tail, robust_tail.h), on the J1 sample either path has left in global memory;
//     one single-wave workgroup per candidate.
#include <hip/hip_runtime.h>
#include <math.h>

#include "mpct_dev.h"
#include "wave_ops.h"
#include "gpc_prologue.h"
#include "dtc_step.h"
#include "robust_reduce.h"
#include "robust_tail.h"
#include "dtc_robust.h"

namespace mpct {

// ------------------------------------------------------------------------------------------
// generic path: J1 [C*D][my], status [C*D] in mpct_eval_batch's layout -> the candidate records
constexpr int kReduceWaves = 4;
__global__ void __launch_bounds__(kWave* kReduceWaves)
    robust_reduce_kernel(long long C, int D, int my, double j_bound, const double* __restrict__ J1,
                         const int* __restrict__ status, const RobustOut out) {
  const int lane = threadIdx.x & (kWave - 1);
  const long long c = (long long)blockIdx.x * kReduceWaves + (threadIdx.x >> 6);
  if (c >= C) return;
  const double* j = J1 + c * D * my;
  const int* s = status + c * D;
  robust_reduce(
      lane, D, my, j_bound, [&](int k, int i) __attribute__((always_inline)) { return j[k * my + i]; },
      [&](int k) __attribute__((always_inline)) { return s[k]; }, out, c);
}

// ------------------------------------------------------------------------------------------
// tail statistics: J1 [C*D][my], status [C*D] or null (read as 0: the fused path keeps none, and its
// failed draws carry a non-finite J1) -> quantile, cvar, q_draw [C][nlev].  The workgroup is ONE wave
// and the whole dynamic LDS (12 B per draw) is its candidate's slice, so the hand-offs inside
// robust_tail need lds_sync() only; with more waves per workgroup each would need a slice of its own
// (the hazard dtc_robust_kernel's barrier comment states).  The workgroups stride over the candidates
__global__ void __launch_bounds__(kWave)
    robust_tail_kernel(long long C, int D, int my, double j_bound, const double* __restrict__ J1,
                       const int* __restrict__ status, int nlev, const TailLevels lv, const TailOut out) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x;
  double* Js = lds;
  int* idx = reinterpret_cast<int*>(lds + D);
  for (long long c = blockIdx.x; c < C; c += gridDim.x) {
    const double* j = J1 + c * D * my;
    const int* s = status ? status + c * D : nullptr;
    robust_tail(
        lane, D, my, j_bound, [&](int k, int i) __attribute__((always_inline)) { return j[k * my + i]; },
        [&](int k) __attribute__((always_inline)) { return s ? s[k] : 0; }, nlev, lv, out, c, Js, idx);
  }
}

// ------------------------------------------------------------------------------------------
// candidate lists of the fused path: lists[0..C) the candidates with nu Nu <= 16, lists[C..2C)
// those above, both in dispatch order (perm, or the caller's order); lists[2C], lists[2C + 1] the
// two counts.  One workgroup: a stable compaction, 1024 slots per pass
constexpr int kClassifyThreads = 1024;
__global__ void __launch_bounds__(kClassifyThreads)
    robust_classify_kernel(int my, int nu, int n2max, int numax, long long C, int D, const int* __restrict__ N2v,
                           const int* __restrict__ Nuv, const int* __restrict__ perm, int* __restrict__ lists,
                           const RobustOut out, double* __restrict__ J1) {
  __shared__ int wc[2][kClassifyThreads / kWave];
  __shared__ int base[2];
  const int tid = threadIdx.x, lane = tid & (kWave - 1), w = tid >> 6;
  if (tid < 2) base[tid] = 0;
  __syncthreads();
  for (long long start = 0; start < C; start += kClassifyThreads) {
    const long long slot = start + tid;
    int cls = -1;
    long long c = 0;
    if (slot < C) {
      c = perm ? (long long)perm[slot] : slot;
      const int N2 = N2v[c], Nu = Nuv[c];
      int bad = 0;
      if (N2 <= 0) bad = MPCT_ST_SKIPPED_;
      else if (N2 > n2max || Nu < 1 || Nu > numax || Nu > N2) bad = MPCT_ST_BADHORIZON_;
      if (bad) {  // never simulated: the record mpct_eval_batch's statuses reduce to
        for (int i = 0; i < my; ++i) {
          if (out.mean) out.mean[c * my + i] = NAN;
          if (out.worst) out.worst[c * my + i] = NAN;
        }
        if (out.n_failed) out.n_failed[c] = 0;
        if (out.worst_draw) out.worst_draw[c] = -1;
        if (out.status) out.status[c] = bad;
        if (J1)
          for (int e = 0; e < D * my; ++e) J1[c * D * my + e] = NAN;
      } else {
        cls = nu * Nu <= 16 ? 0 : 1;
      }
    }
    const unsigned long long b0 = __ballot(cls == 0), b1 = __ballot(cls == 1);
    if (lane == 0) {
      wc[0][w] = __popcll(b0);
      wc[1][w] = __popcll(b1);
    }
    __syncthreads();
    if (cls >= 0) {
      int off = base[cls];
      for (int v = 0; v < w; ++v) off += wc[cls][v];
      off += __popcll((cls ? b1 : b0) & ((1ull << lane) - 1ull));
      lists[(long long)cls * C + off] = (int)c;
    }
    __syncthreads();
    if (tid < 2) {
      int n = base[tid];
      for (int v = 0; v < kClassifyThreads / kWave; ++v) n += wc[tid][v];
      base[tid] = n;
    }
    __syncthreads();
  }
  if (tid < 2) lists[2 * C + tid] = base[tid];
}

// ------------------------------------------------------------------------------------------
// fused path.  LDS of one workgroup (doubles): shared by the waves R (the prologue's M x M), the gain
// rows A, the filter coefficients fr, the prologue's verdict, the draw records [D][kRecW] (J1_0,
// J1_1, status); then kRobustW copies of the loop state (dtc_step.h: xy | ring | hist | frh)
struct RobustLds {
  int R, A, fr, flag, rec, state, sstride, total;
};
__host__ __device__ inline RobustLds robust_lds(const DevScenario& sc, int M, int D) {
  RobustLds L;
  int o = 0;
  auto take = [&](int n) { int r = o; o += (n + 1) & ~1; return r; };
  L.R = take(M * M);
  L.A = take(2 * kSmA);
  L.fr = take(2 * 8);
  L.flag = take(2);
  L.rec = take(D * kRecW);
  L.state = o;
  L.sstride = dtc_state_layout(sc, 0).total;
  L.total = L.state + kRobustW * L.sstride;
  return L;
}

// waves per SIMD and the prologue's Householder block: the values dtc_small_kernel settled on
// (dtc_small.hip MPCT_DTC_W16 / W32 / HB); a 256-thread workgroup puts one wave on each SIMD, so k
// waves per SIMD are k resident workgroups per CU
template <int MAXM>
__global__ void __launch_bounds__(kWave* kRobustW, MAXM <= 16 ? 4 : 3)
    dtc_robust_kernel(const DevScenario sc, long long C, int D, const int* __restrict__ N2v,
                      const int* __restrict__ Nuv, const double* __restrict__ deltav,
                      const double* __restrict__ lambdav, const double* __restrict__ rv,
                      const double* __restrict__ vv, const int* __restrict__ list, const int* __restrict__ cnt,
                      double j_bound, const RobustOut out, double* __restrict__ J1, int mcls) {
  extern __shared__ __attribute__((aligned(16))) double lds[];
  const int lane = threadIdx.x & (kWave - 1);
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int my = sc.my, nu = sc.nu;
  const RobustLds RL = robust_lds(sc, mcls, D);
  DtcLayout L = dtc_state_layout(sc, RL.state + wave * RL.sstride);  // this wave's loop state
  L.R = RL.R;
  L.A = RL.A;
  L.fr = RL.fr;
  int* flag = reinterpret_cast<int*>(lds + RL.flag);
  const int n = *cnt;
  for (int it = blockIdx.x; it < n; it += gridDim.x) {
    const long long c = list[it];
    const int N2 = N2v[c], Nu = Nuv[c];
    const int M = nu * Nu;
    if (wave == 0) {
      // once per candidate: gain pads, filter coefficients (fb taps 0..3, then fa), the first-move
      // rows of A (gpc_prologue.h, no R^-1)
      for (int e = lane; e < 2 * kSmA; e += kWave) lds[RL.A + e] = 0.0;
      if (lane < 2 * 8) {
        const int i = lane >> 3, k = lane & 7;
        lds[RL.fr + lane] = i < my ? sc.sm_fr[i * 8 + k] : 0.0;
      }
      lds_sync();
      const bool ok = gpc_prologue<MAXM, false, false, true, 4>(sc, lane, M, Nu, N2, deltav + c * my, lambdav + c * nu,
                                                                lds + RL.R, nullptr, lds + RL.A, kSmA, sc.sm_acol);
      if (lane == 0) flag[0] = ok ? 1 : 0;
    }
    // The gain and the filters are published to the OTHER waves here: a real workgroup barrier.
    // lds_sync() waits on this wave's own lgkmcnt only and orders nothing between waves; it is
    // valid for the hand-offs inside one wave (the prologue above, the step loop below) and nowhere
    // else in this kernel.
    __syncthreads();
    const int ok = __builtin_amdgcn_readfirstlane(flag[0]);
    for (int k = wave; k < D; k += kRobustW) {
      double j1o = NAN;
      int st = MPCT_ST_NONFINITE_;  // a gain that does not exist: every draw fails, as in dtc_small_kernel
      if (ok) {
        for (int e = lane; e < RL.sstride; e += kWave) lds[L.xy + e] = 0.0;  // this wave's state, re-zeroed per draw
        lds_sync();
        double j1, j22;
        dtc_closed_loop<true>(sc, lds, L, lane, k, rv, vv, j1, j22);
        j1o = __shfl(j1, (lane & 3) * 4, kWave);  // lane i <- lane 4 i
        const unsigned long long nf = __ballot(lane < my && !isfinite(j1o));
        st = nf ? MPCT_ST_NONFINITE_ : 0;
      }
      if (lane < my) lds[RL.rec + k * kRecW + lane] = j1o;
      if (lane == 0) lds[RL.rec + k * kRecW + 2] = (double)st;
    }
    __syncthreads();  // every wave's draw records -> the reducing wave (workgroup barrier, as above)
    // wave 0 reduces while wave 1 copies the sample out; the records are next written after the
    // next candidate's first barrier, which both reach only when they are done here
    if (wave == 0) {
      robust_reduce(
          lane, D, my, j_bound,
          [&](int k, int i) __attribute__((always_inline)) { return lds[RL.rec + k * kRecW + i]; },
          [&](int k) __attribute__((always_inline)) { return (int)lds[RL.rec + k * kRecW + 2]; }, out, c);
    } else if (wave == 1 && J1) {
      for (int e = lane; e < D * my; e += kWave) J1[c * D * my + e] = lds[RL.rec + (e / my) * kRecW + e % my];
    }
  }
}

}  // namespace mpct

// ------------------------------------------------------------------------------------------
// host-side launches
#include <string>

#include "launch_fan.h"

namespace mpct {

static int launched(std::string* err) {
  const hipError_t e = hipGetLastError();
  if (e == hipSuccess) return 0;
  *err = std::string("kernel launch failed: ") + hipGetErrorString(e);
  return -3;
}

int launch_robust_reduce(long long C, int D, int my, double j_bound, const double* J1, const int* status,
                         const RobustOut& out, hipStream_t stream, std::string* err) {
  if (C == 0) return 0;
  const unsigned grid = (unsigned)((C + kReduceWaves - 1) / kReduceWaves);
  hipLaunchKernelGGL(robust_reduce_kernel, dim3(grid), dim3(kWave * kReduceWaves), 0, stream, C, D, my, j_bound, J1,
                     status, out);
  return launched(err);
}

// D <= kTailMaxDraws, 1 <= nlev <= kTailMaxLevels (the callers check); status may be null
int launch_robust_tail(long long C, int D, int my, double j_bound, const double* J1, const int* status, int nlev,
                       const double* levels, const TailOut& out, hipStream_t stream, std::string* err) {
  if (C == 0) return 0;
  TailLevels lv;
  for (int q = 0; q < kTailMaxLevels; ++q) lv.a[q] = q < nlev ? levels[q] : 1.0;
  const long long cap = 1 << 20;  // beyond it the workgroups stride
  const unsigned grid = (unsigned)(C < cap ? C : cap);
  hipLaunchKernelGGL(robust_tail_kernel, dim3(grid), dim3(kWave), robust_tail_lds_bytes(D), stream, C, D, my, j_bound,
                     J1, status, nlev, lv, out);
  return launched(err);
}

long long dtc_robust_lds_bytes(const DevScenario& sc, int M, int D) { return (long long)robust_lds(sc, M, D).total * 8; }

// C candidates x D draws of a small_dtc scenario with nu * numax <= 32 and D <= kRobustMaxD.
// lists: 2 C + 2 ints of device scratch; perm: dispatch order or nullptr; ncu: the device's CUs
int launch_dtc_robust(const DevScenario& sc, long long C, int D, const int* N2, const int* Nu, const double* delta,
                      const double* lambda, const double* r, const double* v, const int* perm, int* lists,
                      double j_bound, const RobustOut& out, double* J1, int ncu, LaunchFan* fan, hipStream_t stream,
                      std::string* err) {
  if (C == 0) return 0;
  hipLaunchKernelGGL(robust_classify_kernel, dim3(1), dim3(kClassifyThreads), 0, stream, sc.my, sc.nu, sc.n2max,
                     sc.numax, C, D, N2, Nu, perm, lists, out, J1);
  int rc = launched(err);
  const bool two = sc.nu * sc.numax > 16;
  FanScope fs(two ? fan : nullptr, stream);
  // the heavier class first; each launch holds at most the workgroups the device keeps resident
  // and strides over its list
  for (int k = 0; k < 2 && rc == 0; ++k) {
    const int cls = two ? (k == 0 ? 32 : 16) : 16;
    if (!two && k == 1) break;
    if (sc.nu > cls) continue;
    const int nu_cls = sc.numax < cls / sc.nu ? sc.numax : cls / sc.nu;
    const int mcls = sc.nu * nu_cls;
    const size_t lds = (size_t)dtc_robust_lds_bytes(sc, mcls, D);
    const long long res = (long long)ncu * (cls == 16 ? 4 : 3);
    const unsigned grid = (unsigned)(C < res ? C : res);
    const int* list = lists + (cls == 16 ? 0 : C);
    const int* cnt = lists + 2 * C + (cls == 16 ? 0 : 1);
    const hipStream_t st = fs.stream(k);
    if (cls == 16)
      hipLaunchKernelGGL(dtc_robust_kernel<16>, dim3(grid), dim3(kWave * kRobustW), lds, st, sc, C, D, N2, Nu, delta,
                         lambda, r, v, list, cnt, j_bound, out, J1, mcls);
    else
      hipLaunchKernelGGL(dtc_robust_kernel<32>, dim3(grid), dim3(kWave * kRobustW), lds, st, sc, C, D, N2, Nu, delta,
                         lambda, r, v, list, cnt, j_bound, out, J1, mcls);
    rc = launched(err);
  }
  fs.join();
  return rc;
}

}  // namespace mpct
