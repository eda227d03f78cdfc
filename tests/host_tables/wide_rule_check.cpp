// Stand-alone check of the wide split's slot count (csrc/mpct_dev.h wide_slot_rule, wide_slots), built
// with the address, leak and undefined-behaviour sanitizers by tests/test_wide_split.py.  No GPU is used.
//   wide_slots: 0 for a launch that is not eligible (no permutation), never more than S, the forced
//   count where one is given (0: the single launch);
//   wide_slot_rule on 256 compute units (one round of gpc_small_kernel: 4096): 0 below the smallest
//   ordered size, every slot up to half a round, a quarter of a round at a full one, 0 above it.
// Exit status 0 when every expectation held.
#include "check.h"

int main() {
  const int ncu = 256;
  CHECK(wide_slot_rule(255, ncu) == 0);
  CHECK(wide_slot_rule(256, ncu) == 256);
  CHECK(wide_slot_rule(2048, ncu) == 2048);
  CHECK(wide_slot_rule(2049, ncu) == 2047);
  CHECK(wide_slot_rule(4096, ncu) == 1024);
  CHECK(wide_slot_rule(4097, ncu) == 0);
  CHECK(wide_slot_rule(8192, ncu) == 0);
  CHECK(wide_slot_rule(4096, 0) == 0);
  std::printf("rule at S = 255, 256, 4096, 8192 on 256 CUs: %lld %lld %lld %lld\n", wide_slot_rule(255, ncu),
              wide_slot_rule(256, ncu), wide_slot_rule(4096, ncu), wide_slot_rule(8192, ncu));
  long long over = 0, unordered = 0, forced_bad = 0, above = 0;
  for (long long S = 1; S <= 9000; ++S) {
    for (int cu : {1, 64, 256, 304}) {
      const long long h = wide_slots(S, cu, true, -1);
      over += h < 0 || h > S;
      above += S > 16LL * cu && h != 0;
      unordered += wide_slots(S, cu, false, -1) != 0 || wide_slots(S, cu, false, 37) != 0;
      for (long long n : {0LL, 1LL, 37LL, 256LL, 100000LL})
        forced_bad += wide_slots(S, cu, true, n) != (n < S ? n : S);
    }
  }
  CHECK(over == 0);
  CHECK(above == 0);
  CHECK(unordered == 0);
  CHECK(forced_bad == 0);
  std::printf("wide_slots: 0 without a permutation, 0 <= H <= S, forced counts kept, S = 1..9000\n");
  return finish();
}
