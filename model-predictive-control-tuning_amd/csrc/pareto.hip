// pareto.hip — Pareto front, domination counts and layers of C cost vectors (see pareto.h, include/mpct.h).
//
// O(C^2 k) pair tests, all integer results.  A lane owns one candidate b with its costs in registers;
// the competitors a stream through LDS as [K][T] tiles that every lane reads at the same address (a
// broadcast: no bank conflict, the pattern of robust_tail_kernel).  Per a:
//   le = AND_j (a_j <= b_j),  lt = OR_j (a_j < b_j),  count += le & lt.
// A NaN in a makes le false, so invalid, dead (layer < pass) and out-of-range competitors are all
// staged with a NaN in column 0 and the inner loop has no branch; a lane without a live b holds NaN and
// counts nothing.  The a-range is split over blockIdx.y and the partial counts meet in integer atomic
// adds (order-independent, so a repeated call is bitwise identical).  Every loop bound is a function
// of C, k and the grid; nothing waits on another workgroup.
#include "pareto.h"

#include "work_order.h"

namespace mpct {

template <int K, int T>
__global__ void __launch_bounds__(kParetoBlock)
    pareto_count_kernel(const double* __restrict__ costs, int C, int k, int chunk, int pass,
                        const int* __restrict__ lay, const int* __restrict__ remaining, int* __restrict__ cnt) {
  __shared__ __attribute__((aligned(16))) double sA[K * T];
  if (*remaining == 0) return;  // every valid candidate has its layer: the pass costs one load
  const int a0 = (int)blockIdx.y * chunk;
  if (a0 >= C) return;          // an empty chunk of a forced split
  const int a1 = a0 + chunk < C ? a0 + chunk : C;
  const int tid = threadIdx.x;
  const int b = (int)blockIdx.x * kParetoBlock + tid;
  const bool mine = b < C && lay[b] == kParetoUnassigned;
  if (!__syncthreads_or(mine ? 1 : 0)) return;  // no candidate of this workgroup is still open
  const double nan = __longlong_as_double(0x7ff8000000000000ll);
  double bv[K];
#pragma unroll
  for (int j = 0; j < K; ++j) bv[j] = j < k ? (mine ? costs[(size_t)b * k + j] : nan) : 0.0;
  for (int e = k * T + tid; e < K * T; e += kParetoBlock) sA[e] = 0.0;  // the padded columns, once
  int count = 0;
  for (int t0 = a0; t0 < a1; t0 += T) {
    // tile [t0, t0 + T) transposed into [k][T]; the global reads are contiguous
    const double* src = costs + (size_t)t0 * k;
    for (int e = tid; e < T * k; e += kParetoBlock) {
      const int t = e / k, j = e - t * k, a = t0 + t;
      double v = nan;
      if (a < a1) {
        v = src[e];
        if (j == 0 && lay[a] < pass) v = nan;  // invalid (-1) or assigned to an earlier layer
      }
      sA[j * T + t] = v;
    }
    __syncthreads();
#pragma unroll 4
    for (int t = 0; t < T; ++t) {
      bool le = true, lt = false;
#pragma unroll
      for (int j = 0; j < K; ++j) {
        const double a = sA[j * T + t];
        le &= a <= bv[j];
        lt |= a < bv[j];
      }
      count += (le & lt) ? 1 : 0;
    }
    __syncthreads();
  }
  if (mine && count) atomicAdd(&cnt[b], count);
}

__global__ void __launch_bounds__(kParetoBlock)
    pareto_init_kernel(const double* __restrict__ costs, int C, int k, int* __restrict__ lay, int* __restrict__ cnt,
                       int* __restrict__ remaining) {
  const int c = (int)blockIdx.x * kParetoBlock + threadIdx.x;
  int valid = 0;
  if (c < C) {
    valid = 1;
    for (int j = 0; j < k; ++j) valid &= costs[(size_t)c * k + j] == costs[(size_t)c * k + j] ? 1 : 0;
    lay[c] = valid ? kParetoUnassigned : -1;
    cnt[c] = 0;
  }
  const int n = __syncthreads_count(valid);
  if (threadIdx.x == 0 && n) atomicAdd(remaining, n);
}

__global__ void __launch_bounds__(kParetoBlock)
    pareto_assign_kernel(int C, int pass, int* __restrict__ lay, int* __restrict__ cnt, int* __restrict__ domc,
                         int* __restrict__ remaining) {
  const int c = (int)blockIdx.x * kParetoBlock + threadIdx.x;
  int done = 0;
  if (c < C && lay[c] == kParetoUnassigned) {
    const int n = cnt[c];
    cnt[c] = 0;
    if (pass == 0) domc[c] = n;
    if (n == 0) {
      lay[c] = pass;
      done = 1;
    }
  }
  const int n = __syncthreads_count(done);
  if (threadIdx.x == 0 && n) atomicSub(remaining, n);
}

__global__ void __launch_bounds__(kParetoBlock)
    pareto_finish_kernel(int C, int max_layers, const int* __restrict__ lay, const int* __restrict__ domc,
                         int* __restrict__ dom_count, int* __restrict__ layer, int* __restrict__ flag) {
  const int c = (int)blockIdx.x * kParetoBlock + threadIdx.x;
  if (c > C) return;
  if (c == C) {
    flag[C] = 0;  // the scan's last entry: pos[C] = size of the front
    return;
  }
  const int l = lay[c];
  const bool valid = l != -1;
  if (dom_count) dom_count[c] = valid ? domc[c] : -1;
  if (layer) layer[c] = !valid ? -1 : (l == kParetoUnassigned ? max_layers : l);
  flag[c] = l == 0 ? 1 : 0;
}

__global__ void __launch_bounds__(kParetoBlock)
    pareto_front_kernel(int C, const int* __restrict__ flag, const int* __restrict__ pos, int* __restrict__ front,
                        int* __restrict__ n_front) {
  const int c = (int)blockIdx.x * kParetoBlock + threadIdx.x;
  if (c >= C) return;
  const int total = pos[C];
  if (c == 0 && n_front) n_front[0] = total;
  if (!front) return;
  if (flag[c]) front[pos[c]] = c;  // pos[c] < total: disjoint from the fill below
  if (c >= total) front[c] = -1;
}

void pareto_grid(long long C, int tile, int split_override, int* split, int* chunk) {
  const long long tiles = (C + tile - 1) / tile;
  const long long nbx = (C + kParetoBlock - 1) / kParetoBlock;
  long long s = split_override > 0 ? split_override : (kParetoTargetBlocks + nbx - 1) / (nbx > 0 ? nbx : 1);
  if (s < 1) s = 1;
  if (split_override <= 0 && s > tiles) s = tiles > 0 ? tiles : 1;
  if (s > 1024) s = 1024;
  const long long per = ((C + s - 1) / s + tile - 1) / tile;  // tiles per chunk
  *chunk = (int)((per > 0 ? per : 1) * tile);
  // without an override no chunk is empty: as many as the tiles-per-chunk leave
  *split = split_override > 0 ? (int)s : (int)((C + *chunk - 1) / *chunk > 0 ? (C + *chunk - 1) / *chunk : 1);
}

template <int T>
static void launch_count(int K, dim3 grid, hipStream_t stream, const double* costs, int C, int k, int chunk, int pass,
                         const int* lay, const int* remaining, int* cnt) {
  const dim3 blk(kParetoBlock);
  switch (K) {
    case 2: hipLaunchKernelGGL((pareto_count_kernel<2, T>), grid, blk, 0, stream, costs, C, k, chunk, pass, lay, remaining, cnt); break;
    case 4: hipLaunchKernelGGL((pareto_count_kernel<4, T>), grid, blk, 0, stream, costs, C, k, chunk, pass, lay, remaining, cnt); break;
    case 8: hipLaunchKernelGGL((pareto_count_kernel<8, T>), grid, blk, 0, stream, costs, C, k, chunk, pass, lay, remaining, cnt); break;
    default: hipLaunchKernelGGL((pareto_count_kernel<16, T>), grid, blk, 0, stream, costs, C, k, chunk, pass, lay, remaining, cnt); break;
  }
}

int pareto_device(const double* costs, long long C64, int k, int max_layers, const ParetoOut& out, hipStream_t stream,
                  std::string* err, int tile, int split_override) {
  if (C64 == 0) {
    if (out.n_front && hipMemsetAsync(out.n_front, 0, sizeof(int), stream) != hipSuccess) {
      *err = "hipMemsetAsync failed (n_front)";
      return -3;
    }
    return 0;
  }
  const int C = (int)C64;
  if (tile != 128 && tile != kParetoTile) tile = kParetoTile;
  const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
  int split = 1, chunk = tile;
  pareto_grid(C, tile, split_override, &split, &chunk);
  const bool want_front = out.front || out.n_front;
  size_t temp = 0;
  if (want_front && scan_exclusive_bytes(C + 1, &temp, err)) return -3;
  const size_t arr = (((size_t)C + 1) * sizeof(int) + 255) & ~(size_t)255;
  void* buf = nullptr;
  if (hipMallocAsync(&buf, 5 * arr + 256 + temp, stream) != hipSuccess) {
    *err = "hipMallocAsync failed (Pareto buffers)";
    return -2;
  }
  char* p = static_cast<char*>(buf);
  int* lay = reinterpret_cast<int*>(p);
  int* cnt = reinterpret_cast<int*>(p + arr);
  int* domc = reinterpret_cast<int*>(p + 2 * arr);
  int* flag = reinterpret_cast<int*>(p + 3 * arr);
  int* pos = reinterpret_cast<int*>(p + 4 * arr);
  int* remaining = reinterpret_cast<int*>(p + 5 * arr);
  void* tmp = p + 5 * arr + 256;
  const unsigned nbx = (unsigned)((C + kParetoBlock - 1) / kParetoBlock);
  const dim3 blk(kParetoBlock);
  int rc = 0;
  auto launched = [&](const char* what) {
    if (hipGetLastError() == hipSuccess) return true;
    *err = std::string(what) + " launch failed";
    rc = -3;
    return false;
  };
  do {
    if (hipMemsetAsync(remaining, 0, sizeof(int), stream) != hipSuccess) {
      *err = "hipMemsetAsync failed (Pareto buffers)";
      rc = -3;
      break;
    }
    hipLaunchKernelGGL(pareto_init_kernel, dim3(nbx), blk, 0, stream, costs, C, k, lay, cnt, remaining);
    if (!launched("pareto_init_kernel")) break;
    // pass 0 is the dom_count pass; exactly max_layers passes when layers are asked for, no host sync
    const int passes = out.layer ? max_layers : 1;
    for (int pass = 0; pass < passes && rc == 0; ++pass) {
      if (tile == 128)
        launch_count<128>(K, dim3(nbx, (unsigned)split), stream, costs, C, k, chunk, pass, lay, remaining, cnt);
      else
        launch_count<kParetoTile>(K, dim3(nbx, (unsigned)split), stream, costs, C, k, chunk, pass, lay, remaining, cnt);
      if (!launched("pareto_count_kernel")) break;
      hipLaunchKernelGGL(pareto_assign_kernel, dim3(nbx), blk, 0, stream, C, pass, lay, cnt, domc, remaining);
      if (!launched("pareto_assign_kernel")) break;
    }
    if (rc) break;
    hipLaunchKernelGGL(pareto_finish_kernel, dim3((unsigned)(C / kParetoBlock + 1)), blk, 0, stream, C, max_layers,
                       (const int*)lay, (const int*)domc, out.dom_count, out.layer, flag);
    if (!launched("pareto_finish_kernel")) break;
    if (want_front) {
      if (scan_exclusive(flag, pos, C + 1, tmp, temp, stream, err)) {
        rc = -3;
        break;
      }
      hipLaunchKernelGGL(pareto_front_kernel, dim3(nbx), blk, 0, stream, C, (const int*)flag, (const int*)pos,
                         out.front, out.n_front);
      if (!launched("pareto_front_kernel")) break;
    }
  } while (false);
  (void)hipFreeAsync(buf, stream);
  return rc;
}

}  // namespace mpct
