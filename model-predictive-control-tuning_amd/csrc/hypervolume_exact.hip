// hypervolume_exact.hip — exact hypervolume of M cost vectors inside a box and every member's exclusive
// contribution, for k <= 3 (see hypervolume_exact.h, include/mpct.h).
//
// One algorithm serves k = 1, 2, 3: a missing axis is the degenerate axis lo = 0, ref = 1, coordinate 0, and
// a product with 1.0 is exact.  The active entries are ordered twice by counting ranks, by (x, y, z, m) and by
// (z, x, y, m); both orders are total, so the sorted sequences are a function of the clipped vectors alone and
// not of where an entry sits in `members`.  Slab s is [z_s, z_(s+1)) in z order (the last ends at ref_z) and
// holds the entries of z rank <= s.  Inside a slab the union is a staircase in (x, y): walking the entries in
// x order, column j = [x_j, x_(j+1)) (the last ends at ref_x) is covered from m1, the smallest y among the
// slab's entries seen so far, up to ref_y, and between m1 and m2, the second smallest, by the holder of m1
// alone.  (m1, holder, m2) is a prefix scan over the lanes of a wave with the carry handed from chunk to
// chunk.  Every term is a product of non-negative differences of clipped coordinates; no volume is ever
// subtracted.
//
// No floating-point atomics.  Workgroup g, one wave, walks the slabs s = g, g + G, .. in ascending order and
// adds into its own phv[g] and pe[g][M]; G is a compile-time constant, so the order of every sum is fixed by
// the sorted values: inside a chunk the fixed trees below, the chunks of a slab in ascending order, the slabs
// of a group in ascending order, the groups in ascending order (hvx_finish_kernel).  Within a slab the holder
// changes only to an entry with a smaller y and never changes back, so a holder owns one run of consecutive
// columns: a segmented scan gives the run's sum inside a chunk, the open run at the chunk's end is carried in
// registers, and pe[g][holder] gets one add per run and slab.  A slab of zero height (equal z values) adds
// only +0.0 and is skipped.
//
// Contraction is off for this unit (the pragma below and the unit's flags, __graft_entry__.UNIT_FLAGS).
#include "hypervolume_exact.h"

#include "wave_ops.h"

#pragma clang fp contract(off)

namespace mpct {

namespace {

constexpr double kHvxInf = __builtin_huge_val();

// the box padded to three axes; false for a box that is not finite with lo < ref
__device__ __forceinline__ bool hvx_box(int k, const double* __restrict__ lo, const double* __restrict__ ref, double (&L)[3],
                                        double (&R)[3]) {
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    L[j] = 0.0;
    R[j] = 1.0;
    if (j < k) {
      const double l = lo[j], r = ref[j];
      ok = ok && l - l == 0.0 && r - r == 0.0 && l < r;
      L[j] = l;
      R[j] = r;
    }
  }
  return ok;
}

// (m1, h, m2) <- combine(left = (a1, ha, a2), right = (m1, h, m2)): the two smallest y of both sides and the
// holder of the smallest, the left one on a tie (then m2 == m1 and the holder owns nothing)
__device__ __forceinline__ void hvx_comb(double a1, int ha, double a2, double& m1, int& h, double& m2) {
  const bool left = a1 <= m1;
  const double n2 = left ? fmin(a2, m1) : fmin(m2, a1);
  m1 = left ? a1 : m1;
  h = left ? ha : h;
  m2 = n2;
}

template <int CTRL, int D>
__device__ __forceinline__ void hvx_scan_row(double& m1, int& h, double& m2, int lane) {
  const double p1 = dppd<CTRL>(m1), p2 = dppd<CTRL>(m2);
  const int ph = dppi<CTRL>(h);
  if ((lane & 15) >= D) hvx_comb(p1, ph, p2, m1, h, m2);
}

// inclusive scan of (m1, h, m2) over the 64 lanes: DPP row_shr steps inside the 16-lane rows, then the last
// lane of the row before (rows 1 and 3) and lane 31 (rows 2 and 3)
__device__ __forceinline__ void hvx_scan(double& m1, int& h, double& m2, int lane) {
  hvx_scan_row<0x111, 1>(m1, h, m2, lane);
  hvx_scan_row<0x112, 2>(m1, h, m2, lane);
  hvx_scan_row<0x114, 4>(m1, h, m2, lane);
  hvx_scan_row<0x118, 8>(m1, h, m2, lane);
  {
    const int src = ((lane & ~15) - 1) & 63;
    const double p1 = __shfl(m1, src, 64), p2 = __shfl(m2, src, 64);
    const int ph = __shfl(h, src, 64);
    if (lane & 16) hvx_comb(p1, ph, p2, m1, h, m2);
  }
  {
    const double p1 = __shfl(m1, 31, 64), p2 = __shfl(m2, 31, 64);
    const int ph = __shfl(h, 31, 64);
    if (lane & 32) hvx_comb(p1, ph, p2, m1, h, m2);
  }
}

template <int CTRL, int D>
__device__ __forceinline__ void hvx_seg_row(double& v, int h, int lane) {
  const double pv = dppd<CTRL>(v);
  const int ph = dppi<CTRL>(h);
  if ((lane & 15) >= D && ph == h) v += pv;
}

// inclusive sum of v over the lanes before this one that have the same holder (a holder's lanes are
// consecutive), in the same fixed tree as hvx_scan
__device__ __forceinline__ double hvx_seg_sum(double v, int h, int lane) {
  hvx_seg_row<0x111, 1>(v, h, lane);
  hvx_seg_row<0x112, 2>(v, h, lane);
  hvx_seg_row<0x114, 4>(v, h, lane);
  hvx_seg_row<0x118, 8>(v, h, lane);
  {
    const int src = ((lane & ~15) - 1) & 63;
    const double pv = __shfl(v, src, 64);
    const int ph = __shfl(h, src, 64);
    if ((lane & 16) && ph == h) v += pv;
  }
  {
    const double pv = __shfl(v, 31, 64);
    const int ph = __shfl(h, 31, 64);
    if ((lane & 32) && ph == h) v += pv;
  }
  return v;
}

}  // namespace

__global__ void __launch_bounds__(kHvxBlock)
    hvx_stage_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                     const double* __restrict__ lo, const double* __restrict__ ref, double* __restrict__ b) {
  const int m = blockIdx.x * kHvxBlock + threadIdx.x;
  if (m >= M) return;
  double L[3], R[3];
  const bool box = hvx_box(k, lo, ref, L, R);
  const int c = members ? members[m] : m;
  bool act = box && c >= 0 && c < C;
  double v[3] = {0.0, 0.0, 0.0};
#pragma unroll
  for (int j = 0; j < 3; ++j) {
    if (j < k && act) {
      const double a = costs[(size_t)c * k + j];
      double bj = a > L[j] ? a : L[j];  // a NaN stays out: the comparison below is false for it
      bj = bj + 0.0;                    // -0.0 -> +0.0
      act = a == a && bj < R[j];
      v[j] = bj;
    }
  }
#pragma unroll
  for (int j = 0; j < 3; ++j) b[(size_t)j * M + m] = act ? v[j] : kHvxInf;
}

__global__ void __launch_bounds__(kHvxBlock)
    hvx_rank_kernel(const double* __restrict__ b, int M, double* __restrict__ xs, double* __restrict__ yx,
                    double* __restrict__ zs, int* __restrict__ idx, int* __restrict__ zrx, int* __restrict__ nact) {
  __shared__ double sx[kHvxBlock], sy[kHvxBlock], sz[kHvxBlock];
  const int tid = threadIdx.x;
  const int m = blockIdx.x * kHvxBlock + tid;
  const double x = m < M ? b[m] : kHvxInf;
  const double y = m < M ? b[(size_t)M + m] : kHvxInf;
  const double z = m < M ? b[2 * (size_t)M + m] : kHvxInf;
  int rx = 0, rz = 0, na = 0;
  for (int t0 = 0; t0 < M; t0 += kHvxBlock) {
    const int e = t0 + tid;
    sx[tid] = e < M ? b[e] : kHvxInf;
    sy[tid] = e < M ? b[(size_t)M + e] : kHvxInf;
    sz[tid] = e < M ? b[2 * (size_t)M + e] : kHvxInf;
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < kHvxBlock; ++t) {
      const double xx = sx[t], yy = sy[t], zz = sz[t];
      const bool tie = t0 + t < m;
      const bool ltx = xx < x || (xx == x && (yy < y || (yy == y && (zz < z || (zz == z && tie)))));
      const bool ltz = zz < z || (zz == z && (xx < x || (xx == x && (yy < y || (yy == y && tie)))));
      rx += ltx ? 1 : 0;
      rz += ltz ? 1 : 0;
      na += xx < kHvxInf ? 1 : 0;
    }
    __syncthreads();
  }
  if (m < M && x < kHvxInf) {  // an inactive entry is +INF and below no active one: rx, rz < n <= M
    xs[rx] = x;
    yx[rx] = y;
    idx[rx] = m;
    zrx[rx] = rz;
    zs[rz] = z;
  }
  if (m == 0) nact[0] = na;
}

__global__ void __launch_bounds__(64)
    hvx_sweep_kernel(const double* __restrict__ xs, const double* __restrict__ yx, const double* __restrict__ zs,
                     const int* __restrict__ idx, const int* __restrict__ zrx, const int* __restrict__ nact, int k,
                     const double* __restrict__ lo, const double* __restrict__ ref, int M, double* __restrict__ phv,
                     double* __restrict__ pe) {
  const int g = blockIdx.x, lane = threadIdx.x;
  int n = nact[0];
  n = n < M ? n : M;
  double L[3], R[3];
  (void)hvx_box(k, lo, ref, L, R);  // a bad box has n = 0 (hvx_stage_kernel)
  double* __restrict__ pg = pe ? pe + (size_t)g * M : nullptr;
  double hv_acc = 0.0;
  for (int s = g; s < n; s += kHvxGroups) {
    const double z0 = zs[s], z1 = s + 1 < n ? zs[s + 1] : R[2];
    const double dz = z1 - z0;
    if (!(dz > 0.0)) continue;  // equal z values: every term of this slab is +0.0
    double c1 = kHvxInf, c2 = kHvxInf;  // the scan's carry: (m1, holder, m2) of the columns before this chunk
    int ch = -1;
    int rh = -1;      // the open run's holder and its sum so far
    double rv = 0.0;
    double area = 0.0;
    for (int j0 = 0; j0 < n; j0 += 64) {
      const int j = j0 + lane;
      const bool in = j < n;
      double dx = 0.0, m1 = kHvxInf, m2 = kHvxInf;
      int h = -1;
      if (in) {
        const double x0 = xs[j], x1 = j + 1 < n ? xs[j + 1] : R[0];
        dx = x1 - x0;
        if (zrx[j] <= s) {
          m1 = yx[j];
          h = idx[j];
        }
      }
      hvx_scan(m1, h, m2, lane);
      hvx_comb(c1, ch, c2, m1, h, m2);
      c1 = bcast(m1, 63);
      c2 = bcast(m2, 63);
      ch = __builtin_amdgcn_readlane(h, 63);
      const bool any = m1 < kHvxInf;
      const double ta = any ? dx * (R[1] - m1) : 0.0;
      area += wave_sum64(ta);
      if (pg) {
        const double te = any ? dx * (fmin(m2, R[1]) - m1) : 0.0;
        const double v = hvx_seg_sum(te, h, lane);
        const int h0 = __builtin_amdgcn_readlane(h, 0);
        const int hn = __shfl_down(h, 1, 64);
        if (h0 != rh) {  // the carried run ended with the last chunk
          if (rh >= 0 && lane == 0) pg[rh] += dz * rv;
          rv = 0.0;
        }
        const double tot = h == h0 ? rv + v : v;
        if (lane != 63 && hn != h && h >= 0 && h < M) pg[h] += dz * tot;
        rh = __builtin_amdgcn_readlane(h, 63);
        rv = bcast(tot, 63);
      }
    }
    hv_acc += dz * area;
    if (pg) {
      if (rh >= 0 && rh < M && lane == 0) pg[rh] += dz * rv;
      // the next slab's adds to pe[g][.] come from other lanes of this wave: keep them in program order
      __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
      __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    }
  }
  if (lane == 0) phv[g] = hv_acc;
}

__global__ void __launch_bounds__(kHvxBlock)
    hvx_finish_kernel(const double* __restrict__ phv, const double* __restrict__ pe, const int* __restrict__ nact, int k,
                      const double* __restrict__ lo, const double* __restrict__ ref, int M, double* __restrict__ hv,
                      double* __restrict__ excl, long long* __restrict__ n_active) {
  const int m = blockIdx.x * kHvxBlock + threadIdx.x;
  double L[3], R[3];
  const bool box = hvx_box(k, lo, ref, L, R);
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  if (excl && m < M) {
    double e = 0.0;
    for (int g = 0; g < kHvxGroups; ++g) e += pe[(size_t)g * M + m];
    excl[m] = box ? e : nan;
  }
  if (m == 0) {
    if (hv) {
      double v = 0.0;
      for (int g = 0; g < kHvxGroups; ++g) v += phv[g];
      hv[0] = box ? v : nan;
    }
    if (n_active) n_active[0] = (long long)nact[0];
  }
}

// scratch: nact (256 B) | phv[G] | pe[G][M] (if excl is wanted) | b[3][M] | xs[M] yx[M] zs[M] | idx[M] zrx[M]
size_t hvx_scratch_bytes(long long M, bool want_excl) {
  const size_t m = (size_t)M;
  return 256 + (size_t)kHvxGroups * 8 + (want_excl ? (size_t)kHvxGroups * m * 8 : 0) + 6 * m * 8 + 2 * m * 4;
}

int hypervolume_exact_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                             const double* ref, const HvxOut& out, hipStream_t stream, std::string* err) {
  const size_t m = (size_t)M;
  const bool want_excl = out.excl != nullptr && M > 0;
  char* blob = nullptr;
  if (hipMallocAsync(reinterpret_cast<void**>(&blob), hvx_scratch_bytes(M, want_excl), stream) != hipSuccess) {
    *err = "hipMallocAsync failed (hypervolume_exact scratch)";
    return -2;
  }
  int* nact = reinterpret_cast<int*>(blob);
  double* phv = reinterpret_cast<double*>(blob + 256);
  double* pe = want_excl ? phv + kHvxGroups : nullptr;
  const size_t zeroed = 256 + (size_t)kHvxGroups * 8 + (want_excl ? (size_t)kHvxGroups * m * 8 : 0);
  double* b = reinterpret_cast<double*>(blob + zeroed);
  double* xs = b + 3 * m;
  double* yx = xs + m;
  double* zs = yx + m;
  int* idx = reinterpret_cast<int*>(zs + m);
  int* zrx = idx + m;
  int rc = 0;
  do {
    if (hipMemsetAsync(blob, 0, zeroed, stream) != hipSuccess) {
      *err = "hipMemsetAsync failed (hypervolume_exact scratch)";
      rc = -3;
      break;
    }
    const unsigned nb = (unsigned)((M + kHvxBlock - 1) / kHvxBlock);
    if (M > 0) {
      hipLaunchKernelGGL(hvx_stage_kernel, dim3(nb), dim3(kHvxBlock), 0, stream, costs, (int)C, k, members, (int)M, lo, ref, b);
      hipLaunchKernelGGL(hvx_rank_kernel, dim3(nb), dim3(kHvxBlock), 0, stream, (const double*)b, (int)M, xs, yx, zs, idx, zrx, nact);
      hipLaunchKernelGGL(hvx_sweep_kernel, dim3(kHvxGroups), dim3(64), 0, stream, (const double*)xs, (const double*)yx,
                         (const double*)zs, (const int*)idx, (const int*)zrx, (const int*)nact, k, lo, ref, (int)M, phv, pe);
    }
    hipLaunchKernelGGL(hvx_finish_kernel, dim3(nb ? nb : 1), dim3(kHvxBlock), 0, stream, (const double*)phv, (const double*)pe,
                       (const int*)nact, k, lo, ref, (int)M, out.hv, want_excl ? out.excl : nullptr, out.n_active);
    if (hipGetLastError() != hipSuccess) {
      *err = "hypervolume_exact kernel launch failed";
      rc = -3;
    }
  } while (false);
  (void)hipFreeAsync(blob, stream);
  return rc;
}

}  // namespace mpct
