// Stand-alone check of the staging layout of an ordered launch's cost records (csrc/mpct_dev.h xcd_row,
// stage_row), built with the address, leak and undefined-behaviour sanitizers by
// tests/test_stage_rows.py.  No GPU is used.
//   xcd_row: for every S = 1..2100 the rows of slots k < S are distinct and lie below
//   kXcds * ceil(S / kXcds), the row count order_stage (work_order.hip) allocates: a ragged last XCD
//   block (S no multiple of kXcds) leaves holes, never a collision or a row past the blob.
//   stage_row: for all 64 subsets of the six cost pointers the requested fields take pairwise disjoint
//   ranges of lengths my, my, my, nu, 1, 1 inside [0, w), w is the sum of those lengths and every field
//   that was not requested is -1; at (my, nu) = (1, 1), (3, 3), (7, 5), (2, 3).
// Exit status 0 when every expectation held.
#include "check.h"

#include <vector>

static void check_xcd_rows() {
  long long worst_holes = 0;
  for (long long S = 1; S <= 2100; ++S) {
    const long long rows = kXcds * ((S + kXcds - 1) / kXcds);
    std::vector<char> seen((size_t)rows, 0);
    long long bad_range = 0, collisions = 0;
    for (long long k = 0; k < S; ++k) {
      const long long row = xcd_row(k, S);
      if (row < 0 || row >= rows) {
        ++bad_range;
        continue;
      }
      collisions += seen[(size_t)row];
      seen[(size_t)row] = 1;
    }
    if (bad_range || collisions) std::printf("S = %lld: %lld rows out of range, %lld collisions\n", S, bad_range, collisions);
    CHECK(bad_range == 0);
    CHECK(collisions == 0);
    if (rows - S > worst_holes) worst_holes = rows - S;
  }
  CHECK(worst_holes == kXcds - 1);  // the ragged sizes were among them
  std::printf("xcd_row: injective and inside %d * ceil(S / %d) rows for S = 1..2100\n", kXcds, kXcds);
}

static void check_stage_rows(int my, int nu) {
  // the pointers are only compared with null: one object serves for every requested field
  double d = 0.0;
  int32_t st = 0;
  int64_t it = 0;
  for (int mask = 0; mask < 64; ++mask) {
    DevResult o{};
    o.J1 = (mask & 1) ? &d : nullptr;
    o.j21 = (mask & 2) ? &d : nullptr;
    o.j22 = (mask & 4) ? &d : nullptr;
    o.Jnu = (mask & 8) ? &d : nullptr;
    o.status = (mask & 16) ? &st : nullptr;
    o.qp_iters = (mask & 32) ? &it : nullptr;
    const StageRow R = stage_row(o, my, nu);
    const int off[6] = {R.j1, R.j21, R.j22, R.jnu, R.st, R.it};
    const int len[6] = {my, my, my, nu, 1, 1};
    int sum = 0;
    std::vector<int> owner((size_t)(3 * my + nu + 2), -1);
    bool ok = true;
    for (int f = 0; f < 6; ++f) {
      if (!((mask >> f) & 1)) {
        ok = ok && off[f] == -1;
        continue;
      }
      sum += len[f];
      if (off[f] < 0 || off[f] + len[f] > R.w || off[f] + len[f] > (int)owner.size()) {
        ok = false;
        continue;
      }
      for (int i = 0; i < len[f]; ++i) {
        ok = ok && owner[(size_t)(off[f] + i)] == -1;  // disjoint from every field before it
        owner[(size_t)(off[f] + i)] = f;
      }
    }
    ok = ok && R.w == sum;
    if (!ok)
      std::printf("my %d nu %d mask %d: w %d, offsets %d %d %d %d %d %d\n", my, nu, mask, R.w, R.j1, R.j21, R.j22, R.jnu,
                  R.st, R.it);
    CHECK(ok);
  }
  std::printf("stage_row: 64 subsets at my = %d, nu = %d\n", my, nu);
}

int main() {
  check_xcd_rows();
  const int dims[4][2] = {{1, 1}, {3, 3}, {7, 5}, {2, 3}};
  for (const auto& mn : dims) check_stage_rows(mn[0], mn[1]);
  // no field requested: a row of width 0, for which launch_closed_loop allocates no stage
  const StageRow none = stage_row(DevResult{}, 3, 3);
  CHECK(none.w == 0 && none.j1 == -1 && none.st == -1 && none.it == -1);
  return finish();
}
