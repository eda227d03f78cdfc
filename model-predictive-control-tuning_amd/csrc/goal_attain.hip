// goal_attain.hip — goal-attainment selection over C cost vectors for G goal / weight vectors (see
// goal_attain.h, include/mpct.h).
//
// O(G C k) terms.  The roles of pareto_count_kernel turned: a lane owns one goal vector g with goal_j,
// iw_j = 1 / w_j and its hard / soft column masks in registers (padded to a compile-time K; a padded column
// has neither mask bit, so whatever it computes is selected away and no 0 * INFINITY can reach a result);
// the candidates c stream through LDS as [K][T] tiles that every lane reads at the same address (a
// broadcast: no bank conflict).  Per (g, c), in ascending j:
//   hard j:  feasible &= F_cj <= goal_j
//   soft j:  d = F_cj - goal_j;  term = d * iw_j;  if (term > gamma) gamma = term, active = j
// each rounded on its own (contraction is off for this unit: the pragma below and -ffp-contract=off).
// A candidate with a NaN cost is infeasible for every g, so that test is made once per tile (sOk) and not per
// lane.  With a valid g no other NaN can arise: a soft goal is finite and 0 < iw < INFINITY.
//
// A lane keeps its NB smallest keys (gamma, c) sorted in registers, `active` packed beside c; the insertion
// is unrolled, so the list is never indexed dynamically, and the worst kept key is tested first.  Candidates
// arrive in ascending c, and a key moves in only where it is strictly smaller (-0.0 == +0.0), so equal gammas
// stay in ascending c: the contract's total order.  The candidate range is split over blockIdx.y; each
// (g, chunk) writes its list and counts to scratch and goal_merge_kernel inserts the chunks' lists in
// ascending chunk order with the same routine.  The key is a total order and the counts are integers, so the
// result does not depend on the split.  Every loop bound is a function of C, G, k, n_best and the grid;
// nothing waits on another workgroup.
#include "goal_attain.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {

constexpr int kActBits = 4;  // active < MPCT_PARETO_MAX_OBJ = 16 rides in the low bits of the candidate index

__device__ __forceinline__ double goal_nan() { return __longlong_as_double(0x7ff8000000000000ll); }
__device__ __forceinline__ double goal_inf() { return __longlong_as_double(0x7ff0000000000000ll); }

// the NB smallest keys seen so far, ascending; ci = (c << kActBits) | active, -1 = empty (then g is NaN)
template <int NB>
struct GoalList {
  double g[NB];
  int ci[NB];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int i = 0; i < NB; ++i) {
      g[i] = goal_nan();
      ci[i] = -1;
    }
  }
  __device__ __forceinline__ bool takes(double gam) const { return ci[NB - 1] < 0 || gam < g[NB - 1]; }
  // slot i takes its left neighbour where the key goes before that one, the key where it goes before slot i
  __device__ __forceinline__ void insert(double gam, int c) {
#pragma unroll
    for (int i = NB - 1; i >= 0; --i) {
      const bool here = ci[i] < 0 || gam < g[i];
      if (i > 0) {
        const bool left = ci[i - 1] < 0 || gam < g[i - 1];
        g[i] = left ? g[i - 1] : (here ? gam : g[i]);
        ci[i] = left ? ci[i - 1] : (here ? c : ci[i]);
      } else {
        g[i] = here ? gam : g[i];
        ci[i] = here ? c : ci[i];
      }
    }
  }
};

// the rows and counts of goal vector g; an invalid g gets -1 / NaN / -1 and -1 counts and no win
template <int NB>
__device__ __forceinline__ void goal_write(int g, bool valid, const GoalList<NB>& L, int nf, int na, int n_best,
                                           const GoalOut& out) {
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    if (i < n_best) {
      const int ci = valid ? L.ci[i] : -1;
      const size_t o = (size_t)g * n_best + i;
      if (out.best) out.best[o] = ci < 0 ? -1 : ci >> kActBits;
      if (out.gamma) out.gamma[o] = ci < 0 ? goal_nan() : L.g[i];
      if (out.active) out.active[o] = ci < 0 ? -1 : ci & ((1 << kActBits) - 1);
    }
  }
  if (out.n_feasible) out.n_feasible[g] = valid ? nf : -1;
  if (out.n_attained) out.n_attained[g] = valid ? na : -1;
  if (out.wins && valid && L.ci[0] >= 0) atomicAdd(&out.wins[L.ci[0] >> kActBits], 1);
}

}  // namespace

// iw[g][j] = 1 / w_gj (one correctly rounded division; 0 for a hard column) and meta[g] = the soft-column mask
// of a valid g, 0 for an invalid one (a valid g has a soft column)
__global__ void __launch_bounds__(kGoalBlock)
    goal_prep_kernel(const double* __restrict__ goals, const double* __restrict__ weights, int G, int k,
                     double* __restrict__ iw, int* __restrict__ meta) {
  const int g = (int)blockIdx.x * kGoalBlock + threadIdx.x;
  if (g >= G) return;
  bool ok = true;
  int soft = 0;
  for (int j = 0; j < k; ++j) {
    const double w = weights[(size_t)g * k + j], gl = goals[(size_t)g * k + j];
    double r = 0.0;
    if (w == 0.0) {
      ok &= gl == gl;  // a hard goal: anything but NaN
    } else if (w > 0.0 && w < goal_inf()) {
      r = 1.0 / w;
      ok &= r < goal_inf();                              // a subnormal w whose reciprocal overflows
      ok &= gl - gl == 0.0;                              // a soft goal is finite
      soft |= 1 << j;
    } else {
      ok = false;  // negative, NaN or infinite
    }
    iw[(size_t)g * k + j] = r;
  }
  meta[g] = ok ? soft : 0;
}

template <int K, int NB, int T>
__global__ void __launch_bounds__(kGoalBlock)
    goal_pair_kernel(const double* __restrict__ costs, int C, int k, int chunk, const double* __restrict__ goals,
                     const double* __restrict__ iw, const int* __restrict__ meta, int G, int n_best, int final,
                     GoalOut out, double* __restrict__ pg, int* __restrict__ pci, int* __restrict__ pcnt) {
  __shared__ __attribute__((aligned(16))) double sA[K * T];
  __shared__ int sOk[T];
  const int tid = threadIdx.x;
  const int g = (int)blockIdx.x * kGoalBlock + tid;
  const int soft = g < G ? meta[g] : 0;
  const bool live = soft != 0;
  double gl[K], wi[K];
  bool sf[K], hd[K];
#pragma unroll
  for (int j = 0; j < K; ++j) {
    const bool in = live && j < k;
    gl[j] = in ? goals[(size_t)g * k + j] : 0.0;
    wi[j] = in ? iw[(size_t)g * k + j] : 0.0;
    sf[j] = in && ((soft >> j) & 1);
    hd[j] = in && !((soft >> j) & 1);
  }
  const int first = live ? __ffs(soft) - 1 : 0;
  GoalList<NB> L;
  L.clear();
  int nf = 0, na = 0;
  const int a0 = (int)blockIdx.y * chunk < C ? (int)blockIdx.y * chunk : C;  // an empty chunk of a forced split: a0 = a1
  const int a1 = a0 + chunk < C ? a0 + chunk : C;
  if (__syncthreads_or(live ? 1 : 0)) {  // else no goal vector of this workgroup is valid
    for (int e = k * T + tid; e < K * T; e += kGoalBlock) sA[e] = 0.0;  // the padded columns, once
    // element e = t * k + j of a tile: (t, j) of this lane's first element and the step of kGoalBlock elements,
    // so the staging loop divides nothing
    const int tq = tid / k, tr = tid - tq * k, dq = kGoalBlock / k, dr = kGoalBlock - dq * k;
    for (int t0 = a0; t0 < a1; t0 += T) {
      // tile [t0, t0 + T) transposed into [k][T]; the global reads are contiguous
      const double* src = costs + (size_t)t0 * k;
      int t = tq, j = tr;
      for (int e = tid; e < T * k; e += kGoalBlock) {
        sA[j * T + t] = t0 + t < a1 ? src[e] : goal_nan();
        t += dq;
        j += dr;
        if (j >= k) {
          j -= k;
          ++t;
        }
      }
      __syncthreads();
      for (int t = tid; t < T; t += kGoalBlock) {
        bool ok = t0 + t < a1;
        for (int j = 0; j < k; ++j) ok &= sA[j * T + t] == sA[j * T + t];
        sOk[t] = ok ? 1 : 0;
      }
      __syncthreads();
#pragma unroll 2
      for (int t = 0; t < T; ++t) {
        bool feas = sOk[t] != 0 && live;
        double gam = -goal_inf();
        int act = first;
#pragma unroll
        for (int j = 0; j < K; ++j) {
          const double a = sA[j * T + t];
          const double d = a - gl[j];
          const double term = d * wi[j];
          feas &= !hd[j] || a <= gl[j];
          const bool up = sf[j] && term > gam;
          gam = up ? term : gam;
          act = up ? j : act;
        }
        if (feas) {
          ++nf;
          na += gam <= 0.0 ? 1 : 0;
          if (L.takes(gam)) L.insert(gam, ((t0 + t) << kActBits) | act);
        }
      }
      __syncthreads();
    }
  }
  if (g >= G) return;
  if (final) {
    goal_write<NB>(g, live, L, nf, na, n_best, out);
    return;
  }
  const size_t s = blockIdx.y;
#pragma unroll
  for (int i = 0; i < NB; ++i) {
    pg[(s * NB + i) * G + g] = L.g[i];
    pci[(s * NB + i) * G + g] = L.ci[i];
  }
  pcnt[(s * 2 + 0) * G + g] = nf;
  pcnt[(s * 2 + 1) * G + g] = na;
}

// per g: the NB smallest keys over the chunks' lists, taken in ascending chunk (so ascending candidate) order
template <int NB>
__global__ void __launch_bounds__(kGoalBlock)
    goal_merge_kernel(int G, int split, int n_best, const int* __restrict__ meta, const double* __restrict__ pg,
                      const int* __restrict__ pci, const int* __restrict__ pcnt, GoalOut out) {
  const int g = (int)blockIdx.x * kGoalBlock + threadIdx.x;
  if (g >= G) return;
  GoalList<NB> L;
  L.clear();
  int nf = 0, na = 0;
  for (size_t s = 0; s < (size_t)split; ++s) {
    nf += pcnt[(s * 2 + 0) * G + g];
    na += pcnt[(s * 2 + 1) * G + g];
    for (int i = 0; i < NB; ++i) {
      const int ci = pci[(s * NB + i) * G + g];
      if (ci < 0) break;  // the rest of this chunk's list is empty
      const double gam = pg[(s * NB + i) * G + g];
      if (L.takes(gam)) L.insert(gam, ci);
    }
  }
  goal_write<NB>(g, meta[g] != 0, L, nf, na, n_best, out);
}

void goal_grid(long long G, long long C, int tile, int split_override, int* split, int* chunk) {
  const long long tiles = (C + tile - 1) / tile;
  const long long nbx = (G + kGoalBlock - 1) / kGoalBlock;
  long long s = split_override > 0 ? split_override : (kGoalTargetBlocks + nbx - 1) / (nbx > 0 ? nbx : 1);
  if (s < 1) s = 1;
  if (split_override <= 0 && s > tiles) s = tiles > 0 ? tiles : 1;
  if (s > kGoalMaxSplit) s = kGoalMaxSplit;
  const long long per = ((C + s - 1) / s + tile - 1) / tile;  // tiles per chunk
  *chunk = (int)((per > 0 ? per : 1) * tile);
  // without an override no chunk is empty: as many as the tiles-per-chunk leave
  *split = split_override > 0 ? (int)s : (int)((C + *chunk - 1) / *chunk > 0 ? (C + *chunk - 1) / *chunk : 1);
}

namespace {

struct PairArgs {
  const double* costs;
  int C, k, chunk;
  const double *goals, *iw;
  const int* meta;
  int G, n_best, final;
  GoalOut out;
  double* pg;
  int *pci, *pcnt;
};

template <int K, int NB, int T>
void launch_pair3(dim3 grid, hipStream_t stream, const PairArgs& a) {
  hipLaunchKernelGGL((goal_pair_kernel<K, NB, T>), grid, dim3(kGoalBlock), 0, stream, a.costs, a.C, a.k, a.chunk, a.goals,
                     a.iw, a.meta, a.G, a.n_best, a.final, a.out, a.pg, a.pci, a.pcnt);
}

template <int K, int NB>
void launch_pair2(int tile, dim3 grid, hipStream_t stream, const PairArgs& a) {
  if (tile == 128)
    launch_pair3<K, NB, 128>(grid, stream, a);
  else
    launch_pair3<K, NB, kGoalTile>(grid, stream, a);
}

template <int K>
void launch_pair1(int NB, int tile, dim3 grid, hipStream_t stream, const PairArgs& a) {
  switch (NB) {
    case 1: launch_pair2<K, 1>(tile, grid, stream, a); break;
    case 4: launch_pair2<K, 4>(tile, grid, stream, a); break;
    default: launch_pair2<K, 16>(tile, grid, stream, a); break;
  }
}

}  // namespace

int goal_attain_device(const double* costs, long long C64, int k, const double* goals, const double* weights,
                       long long G64, int n_best, const GoalOut& out, hipStream_t stream, std::string* err, int tile,
                       int split_override) {
  const int C = (int)C64, G = (int)G64;
  if (out.wins && C > 0 && hipMemsetAsync(out.wins, 0, (size_t)C * sizeof(int), stream) != hipSuccess) {
    *err = "hipMemsetAsync failed (wins)";
    return -3;
  }
  if (G == 0) return 0;
  if (tile != 128 && tile != kGoalTile) tile = kGoalTile;
  const int K = k <= 4 ? 4 : k <= 8 ? 8 : 16;
  const int NB = n_best <= 1 ? 1 : n_best <= 4 ? 4 : 16;
  int split = 1, chunk = tile;
  goal_grid(G, C, tile, split_override, &split, &chunk);
  const bool merge = split > 1;
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t b_iw = al((size_t)G * k * sizeof(double)), b_meta = al((size_t)G * sizeof(int));
  const size_t b_pg = merge ? al((size_t)split * NB * G * sizeof(double)) : 0;
  const size_t b_pci = merge ? al((size_t)split * NB * G * sizeof(int)) : 0;
  const size_t b_pcnt = merge ? al((size_t)split * 2 * G * sizeof(int)) : 0;
  void* buf = nullptr;
  if (hipMallocAsync(&buf, b_iw + b_meta + b_pg + b_pci + b_pcnt, stream) != hipSuccess) {
    *err = "hipMallocAsync failed (goal-attainment buffers)";
    return -2;
  }
  char* p = static_cast<char*>(buf);
  double* iw = reinterpret_cast<double*>(p);
  int* meta = reinterpret_cast<int*>(p + b_iw);
  double* pg = reinterpret_cast<double*>(p + b_iw + b_meta);
  int* pci = reinterpret_cast<int*>(p + b_iw + b_meta + b_pg);
  int* pcnt = reinterpret_cast<int*>(p + b_iw + b_meta + b_pg + b_pci);
  const unsigned nbx = (unsigned)((G + kGoalBlock - 1) / kGoalBlock);
  int rc = 0;
  auto launched = [&](const char* what) {
    if (hipGetLastError() == hipSuccess) return true;
    *err = std::string(what) + " launch failed";
    rc = -3;
    return false;
  };
  do {
    hipLaunchKernelGGL(goal_prep_kernel, dim3(nbx), dim3(kGoalBlock), 0, stream, goals, weights, G, k, iw, meta);
    if (!launched("goal_prep_kernel")) break;
    const PairArgs a{costs, C, k, chunk, goals, iw, meta, G, n_best, merge ? 0 : 1, out, pg, pci, pcnt};
    const dim3 grid(nbx, (unsigned)split);
    switch (K) {
      case 4: launch_pair1<4>(NB, tile, grid, stream, a); break;
      case 8: launch_pair1<8>(NB, tile, grid, stream, a); break;
      default: launch_pair1<16>(NB, tile, grid, stream, a); break;
    }
    if (!launched("goal_pair_kernel")) break;
    if (merge) {
      switch (NB) {
        case 1: hipLaunchKernelGGL(goal_merge_kernel<1>, dim3(nbx), dim3(kGoalBlock), 0, stream, G, split, n_best, (const int*)meta, (const double*)pg, (const int*)pci, (const int*)pcnt, out); break;
        case 4: hipLaunchKernelGGL(goal_merge_kernel<4>, dim3(nbx), dim3(kGoalBlock), 0, stream, G, split, n_best, (const int*)meta, (const double*)pg, (const int*)pci, (const int*)pcnt, out); break;
        default: hipLaunchKernelGGL(goal_merge_kernel<16>, dim3(nbx), dim3(kGoalBlock), 0, stream, G, split, n_best, (const int*)meta, (const double*)pg, (const int*)pci, (const int*)pcnt, out); break;
      }
      if (!launched("goal_merge_kernel")) break;
    }
  } while (false);
  (void)hipFreeAsync(buf, stream);
  return rc;
}

}  // namespace mpct
