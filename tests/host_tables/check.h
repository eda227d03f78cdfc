// What the stand-alone variant-table checks share (small_variants_check.cpp, band_variants_check.cpp):
// the failure counter, CHECK, a build_scenario that counts a rejection as a failure, the expected
// rejection, and the closing "ok" line the tests look for.
#pragma once
#include "scenario_tables.h"

#include <cstdio>

using namespace mpct;

static int g_bad = 0;
#define CHECK(cond)                                                \
  do {                                                             \
    if (!(cond)) {                                                 \
      std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); \
      ++g_bad;                                                     \
    }                                                              \
  } while (0)

[[maybe_unused]] static std::unique_ptr<mpct_scenario> build(const mpct_scenario_desc& d, int est = 0) {
  BuildError err;
  auto s = build_scenario(d, &err, est);
  if (!s) {
    std::printf("FAILED: rejected %d \"%s\"\n", err.code, err.msg.c_str());
    ++g_bad;
  }
  return s;
}

[[maybe_unused]] static void expect_reject(const mpct_scenario_desc& d, int est, int code, const char* msg,
                                           const char* what) {
  BuildError err;
  auto s = build_scenario(d, &err, est);
  CHECK(!s && err.code == code && err.msg == msg);
  std::printf("%s: rejected %d \"%s\"\n", what, err.code, err.msg.c_str());
}

// the last line of main: "ok" and exit status 0 when every expectation held
static int finish() {
  std::printf(g_bad ? "%d expectation(s) failed\n" : "ok\n", g_bad);
  return g_bad ? 1 : 0;
}
