// hv_select.hip — greedy forward selection of the members that carry a front, on the coverage count of the
// hypervolume contract (see hv_select.h, include/mpct.h).
//
// n_pick rounds x N sample points x M members x k column tests, every result an integer.  Round r needs, per
// member, the number of points it covers that no earlier pick covers: a count per MEMBER, where
// hv_count_kernel counts per point.  A lane still owns one sample point, generated in registers by
// hv_points.h, and the members still stream through LDS as [K][T] tiles read at a wave-uniform address.  A
// persistent bitmask holds every point's "still uncovered" bit; a wave owns whole 64-bit words of it.  Per
// member the wave's gain is popcount(ballot(live && le)), a scalar; lane (t mod 64) keeps it, so a tile of
// T members costs T / 64 registers and a compare and a select per member.  The waves of
// a workgroup meet in LDS adds, the workgroups in one 64-bit atomic add per member with a non-zero gain, per
// tile and trip.  Integer adds commute: a repeated call is bitwise identical whatever the grid.
//
// The call is a fixed sequence of launches on the caller's stream -- per round the gain kernel, then the
// one-workgroup argmax -- that depends on n_pick, N and M only; the rounds hand on through HvselState in
// device memory, with a kernel boundary between writer and reader.  Once the largest gain is 0 the later
// rounds' kernels leave on their first read of st->done.  Every loop bound is a function of the arguments
// and the grid; no workgroup waits for another.
#include "hv_select.h"

#include <vector>

#pragma clang fp contract(off)

namespace mpct {

template <int K, int T>
__global__ void __launch_bounds__(kHvBlock)
    hvsel_gain_kernel(const double* __restrict__ costs, int C, int k, const int* __restrict__ members, int M,
                      const double* __restrict__ lo, const double* __restrict__ ref, long long N,
                      unsigned long long seed, int round, unsigned long long* __restrict__ alive,
                      unsigned long long* __restrict__ gains, HvselState* __restrict__ st) {
  static_assert(T % 64 == 0 && T <= kHvBlock, "a tile is whole waves of members and one flush per thread");
  __shared__ __attribute__((aligned(16))) double sA[K * T];
  __shared__ unsigned sG[T];  // this trip's gains of the tile's members, over the workgroup's waves
  if (round > 0 && st->done) return;  // the same for every wave of the grid
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6;
  hv_tile_pad<K, T>(sA, k, tid);
  if (tid < T) sG[tid] = 0;
  double row[K];  // the previous pick
#pragma unroll
  for (int j = 0; j < K; ++j) row[j] = round > 0 ? st->row[j] : 0.0;
  unsigned long long ncov = 0;  // round 0: this wave's points that any entry covers
  const long long nblocks = (N + kHvBlock - 1) / kHvBlock;
  for (long long blk = blockIdx.x; blk < nblocks; blk += gridDim.x) {
    const long long i = blk * kHvBlock + tid;
    const bool active = i < N;
    double p[K];
    hv_point<K>(p, k, lo, ref, seed, i, active);
    const long long widx = blk * (kHvBlock / 64) + w;  // alive has 4 words per point block
    unsigned long long word;
    if (round == 0) {
      word = __ballot(active);
    } else {
      const unsigned long long old = alive[widx];
      bool cov = true;
#pragma unroll
      for (int j = 0; j < K; ++j) cov &= row[j] <= p[j];
      word = old & ~__ballot(cov);
      if (lane == 0 && word != old) alive[widx] = word;
    }
    const bool live = (word >> lane) & 1ull;
    bool any = false;
    if (__syncthreads_or(word != 0ull)) {  // a workgroup with no live point stages nothing
      for (int t0 = 0; t0 < M; t0 += T) {
        hv_stage_tile<T>(sA, costs, C, k, members, M, t0, tid);
        __syncthreads();
        if (word != 0ull) {  // wave-uniform: a wave whose 64 bits are all clear skips the members
          int acc[T / 64];
#pragma unroll
          for (int h = 0; h < T / 64; ++h) {
            acc[h] = 0;
#pragma unroll 4
            for (int tt = 0; tt < 64; ++tt) {
              const int t = h * 64 + tt;
              bool le = true;
#pragma unroll
              for (int j = 0; j < K; ++j) le &= sA[j * T + t] <= p[j];
              any |= le;
              const int cnt = __popcll(__ballot(live && le));  // by every lane: not inside the select below
              acc[h] = lane == tt ? cnt : acc[h];
            }
            if (acc[h]) atomicAdd(&sG[h * 64 + lane], (unsigned)acc[h]);
          }
        }
        __syncthreads();
        if (tid < T) {
          const unsigned g = sG[tid];
          if (g && t0 + tid < M) atomicAdd(&gains[t0 + tid], (unsigned long long)g);
          sG[tid] = 0;
        }
      }
    }
    if (round == 0) {  // a point that no entry covers never contributes: clear it now
      const unsigned long long first = __ballot(live && any);
      ncov += (unsigned long long)__popcll(first);
      if (lane == 0) alive[widx] = first;
    }
  }
  if (round == 0 && lane == 0 && ncov) atomicAdd(&st->n_covered_all, ncov);
}

namespace {
struct HvselBest {
  unsigned long long g;
  int m, cnt;
};
__device__ __forceinline__ void hvsel_merge(HvselBest& a, unsigned long long g, int m, int cnt) {
  if (g > a.g) {
    a.g = g, a.m = m, a.cnt = cnt;
  } else if (g == a.g) {
    a.cnt += cnt;
    a.m = m < a.m ? m : a.m;
  }
}
__device__ __forceinline__ double hvsel_hv(unsigned long long covered, long long N, int k, const double* __restrict__ lo,
                                           const double* __restrict__ ref) {
  bool box = true;
  const double vol = hv_box_volume(k, lo, ref, &box);
  return box ? ((double)covered / (double)N) * vol : __longlong_as_double(0x7ff8000000000000ll);
}
}  // namespace

__global__ void __launch_bounds__(kHvBlock)
    hvsel_pick_kernel(const double* __restrict__ costs, int k, const int* __restrict__ members, int M,
                      const double* __restrict__ lo, const double* __restrict__ ref, long long N, int round,
                      unsigned long long* __restrict__ gains, HvselState* __restrict__ st, HvSelOut out) {
  __shared__ unsigned long long sg[kHvBlock / 64];
  __shared__ int sm[kHvBlock / 64], sc[kHvBlock / 64];
  if (blockIdx.x != 0 || st->done) return;
  const int tid = threadIdx.x;
  HvselBest b{0ull, 0x7fffffff, 0};
  for (int m = tid; m < M; m += kHvBlock) {
    hvsel_merge(b, gains[m], m, 1);
    gains[m] = 0;  // for the next round
  }
#pragma unroll
  for (int off = 32; off >= 1; off >>= 1) {
    const unsigned long long g = __shfl_xor(b.g, off);
    const int m = __shfl_xor(b.m, off), cnt = __shfl_xor(b.cnt, off);
    hvsel_merge(b, g, m, cnt);
  }
  if ((tid & 63) == 0) sg[tid >> 6] = b.g, sm[tid >> 6] = b.m, sc[tid >> 6] = b.cnt;
  __syncthreads();
  if (tid != 0) return;
  for (int v = 1; v < kHvBlock / 64; ++v) hvsel_merge(b, sg[v], sm[v], sc[v]);
  if (b.g == 0ull) {  // nothing left to cover: the slots from here on are the finish kernel's
    st->done = 1;
    return;
  }
  const int c = members ? members[b.m] : b.m;  // in [0, C): the entry covers a point
  const unsigned long long covered = st->covered + b.g;
  st->covered = covered;
  st->n_picked = round + 1;
  for (int j = 0; j < 16; ++j) st->row[j] = j < k ? costs[(size_t)c * k + j] : 0.0;
  if (out.pos) out.pos[round] = b.m;
  if (out.index) out.index[round] = c;
  if (out.gain) out.gain[round] = (long long)b.g;
  if (out.covered) out.covered[round] = (long long)covered;
  if (out.hv) out.hv[round] = hvsel_hv(covered, N, k, lo, ref);
  if (out.ties) out.ties[round] = b.cnt;
}

__global__ void __launch_bounds__(kHvBlock)
    hvsel_finish_kernel(int k, const double* __restrict__ lo, const double* __restrict__ ref, long long N, int n_pick,
                        const HvselState* __restrict__ st, HvSelOut out) {
  if (blockIdx.x != 0) return;
  const int tid = threadIdx.x, np = st->n_picked;
  const unsigned long long covered = st->covered;
  if (tid == 0) {
    if (out.n_picked) out.n_picked[0] = np;
    if (out.n_covered_all) out.n_covered_all[0] = (long long)st->n_covered_all;
  }
  for (int r = np + tid; r < n_pick; r += kHvBlock) {
    if (out.pos) out.pos[r] = -1;
    if (out.index) out.index[r] = -1;
    if (out.gain) out.gain[r] = 0;
    if (out.covered) out.covered[r] = (long long)covered;
    if (out.hv) out.hv[r] = hvsel_hv(covered, N, k, lo, ref);
    if (out.ties) out.ties[r] = 0;
  }
}

template <int T>
static void launch_gain(int K, unsigned grid, hipStream_t stream, const double* costs, int C, int k, const int* members,
                        int M, const double* lo, const double* ref, long long N, unsigned long long seed, int round,
                        unsigned long long* alive, unsigned long long* gains, HvselState* st) {
  const dim3 g(grid), blk(kHvBlock);
  switch (K) {
    case 2: hipLaunchKernelGGL((hvsel_gain_kernel<2, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, round, alive, gains, st); break;
    case 4: hipLaunchKernelGGL((hvsel_gain_kernel<4, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, round, alive, gains, st); break;
    case 8: hipLaunchKernelGGL((hvsel_gain_kernel<8, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, round, alive, gains, st); break;
    default: hipLaunchKernelGGL((hvsel_gain_kernel<16, T>), g, blk, 0, stream, costs, C, k, members, M, lo, ref, N, seed, round, alive, gains, st); break;
  }
}

int hv_select_device(const double* costs, long long C, int k, const int* members, long long M, const double* lo,
                     const double* ref, long long N, unsigned long long seed, int n_pick, const HvSelOut& out,
                     hipStream_t stream, std::string* err, int tile, int max_blocks, float* round_ms) {
  if (tile != 128 && tile != 256) tile = kHvselTile;
  const int K = k <= 2 ? 2 : k <= 4 ? 4 : k <= 8 ? 8 : 16;
  const long long nblocks = (N + kHvBlock - 1) / kHvBlock;
  const long long cap = max_blocks > 0 && max_blocks < kHvselGridCap ? max_blocks : kHvselGridCap;
  const unsigned grid = (unsigned)(nblocks < cap ? nblocks : cap);
  // one blob: the state | gains[M] | alive[4 nblocks], each 256-B aligned
  auto al = [](size_t b) { return (b + 255) & ~(size_t)255; };
  const size_t ns = al(sizeof(HvselState)), ng = al((size_t)(M > 0 ? M : 1) * sizeof(unsigned long long)),
               na = (size_t)nblocks * (kHvBlock / 64) * sizeof(unsigned long long);
  char* blob = nullptr;
  if (hipMallocAsync(reinterpret_cast<void**>(&blob), ns + ng + na, stream) != hipSuccess) {
    *err = "hipMallocAsync failed (hv_select state, gains and bitmask)";
    return -2;
  }
  HvselState* st = reinterpret_cast<HvselState*>(blob);
  unsigned long long* gains = reinterpret_cast<unsigned long long*>(blob + ns);
  unsigned long long* alive = reinterpret_cast<unsigned long long*>(blob + ns + ng);
  std::vector<hipEvent_t> ev;
  int rc = 0;
  do {
    if (hipMemsetAsync(blob, 0, ns + ng, stream) != hipSuccess) {  // alive is written whole by round 0
      *err = "hipMemsetAsync failed (hv_select state)";
      rc = -3;
      break;
    }
    const int rounds = M > 0 ? n_pick : 0;
    if (round_ms) {
      ev.resize((size_t)rounds + 1, nullptr);
      for (auto& e : ev)
        if (hipEventCreate(&e) != hipSuccess) rc = -3;
      if (rc) {
        *err = "hipEventCreate failed (hv_select round timing)";
        break;
      }
      (void)hipEventRecord(ev[0], stream);
    }
    for (int r = 0; r < rounds; ++r) {
      if (tile == 128)
        launch_gain<128>(K, grid, stream, costs, (int)C, k, members, (int)M, lo, ref, N, seed, r, alive, gains, st);
      else
        launch_gain<256>(K, grid, stream, costs, (int)C, k, members, (int)M, lo, ref, N, seed, r, alive, gains, st);
      hipLaunchKernelGGL(hvsel_pick_kernel, dim3(1), dim3(kHvBlock), 0, stream, costs, k, members, (int)M, lo, ref, N, r,
                         gains, st, out);
      if (round_ms) (void)hipEventRecord(ev[(size_t)r + 1], stream);
    }
    hipLaunchKernelGGL(hvsel_finish_kernel, dim3(1), dim3(kHvBlock), 0, stream, k, lo, ref, N, n_pick,
                       (const HvselState*)st, out);
    if (hipGetLastError() != hipSuccess) {
      *err = "hv_select kernel launch failed";
      rc = -3;
      break;
    }
    if (round_ms) {
      if (hipStreamSynchronize(stream) != hipSuccess) {
        *err = "hipStreamSynchronize failed (hv_select round timing)";
        rc = -3;
        break;
      }
      for (int r = 0; r < n_pick; ++r) {
        round_ms[r] = 0.0f;
        if (r < rounds) (void)hipEventElapsedTime(&round_ms[r], ev[(size_t)r], ev[(size_t)r + 1]);
      }
    }
  } while (false);
  for (auto e : ev)
    if (e) (void)hipEventDestroy(e);
  (void)hipFreeAsync(blob, stream);
  return rc;
}

}  // namespace mpct
