// Stand-alone print-out of the dispatch key's Gram tables (csrc/scenario_tables.h gram_tables), built
// by tests/test_order_keys.py with the flags of host_tables_check.cpp.  No GPU, no HIP runtime.
// It reads one linear GPC descriptor from stdin (text_descriptor.h), then a count and that many
// (N2, Nu) pairs, builds the scenario and its tables and prints
//   gram_doubles=<size of the table>
//   nonzero_uncovered=<nonzero doubles in the blocks with nu Nu > kGramM or Nu > N2, which stay zero>
//   block <N2> <Nu> <o> <kGramOut numbers>     per pair and output: G_o'G_o (kGramM x kGramM), then G_o'1
// and a last line "ok".  Exit status 1 on a malformed input, 2 when the builder rejects the descriptor.
#include "text_descriptor.h"

using namespace mpct;

int main() {
  TextDescriptor t;
  if (!t.read()) return 1;
  int npair = 0;
  if (!(std::cin >> npair) || npair < 0 || npair > 64) return 1;
  std::vector<int> pairs(2 * (size_t)npair);
  for (int& x : pairs)
    if (!(std::cin >> x)) return 1;
  BuildError err;
  const std::unique_ptr<mpct_scenario> s = build_scenario(t.d, &err);
  if (!s) {
    std::printf("rejected %d \"%s\"\n", err.code, err.msg.c_str());
    return 2;
  }
  std::vector<double> g;
  gram_tables(s.get(), g);
  std::printf("gram_doubles=%zu\n", g.size());
  const size_t blk = (size_t)s->my * kGramOut;
  size_t uncovered = 0;
  for (int N2 = 1; N2 <= s->n2max && !g.empty(); ++N2)
    for (int Nu = 1; Nu <= s->numax; ++Nu) {
      if (s->nu * Nu <= kGramM && Nu <= N2) continue;
      const double* b = g.data() + ((size_t)(N2 - 1) * s->numax + (Nu - 1)) * blk;
      for (size_t k = 0; k < blk; ++k) uncovered += b[k] != 0.0;
    }
  std::printf("nonzero_uncovered=%zu\n", uncovered);
  for (int p = 0; p < npair; ++p) {
    const int N2 = pairs[2 * p], Nu = pairs[2 * p + 1];
    if (g.empty() || N2 < 1 || N2 > s->n2max || Nu < 1 || Nu > s->numax) return 1;
    const double* b = g.data() + ((size_t)(N2 - 1) * s->numax + (Nu - 1)) * blk;
    for (int o = 0; o < s->my; ++o) {
      std::printf("block %d %d %d", N2, Nu, o);
      for (int k = 0; k < kGramOut; ++k) std::printf(" %.17g", b[(size_t)o * kGramOut + k]);
      std::printf("\n");
    }
  }
  std::printf("ok\n");
  return 0;
}
