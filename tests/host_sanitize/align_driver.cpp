// Host-side walk of include/dt_hip_align.h under AddressSanitizer and UndefinedBehaviorSanitizer: the workspace queries and
// every argument error of the three entry points.  All of them return before any HIP call, so the program needs no GPU.
// Built by csrc/build.py::build_align_sanitizer_driver from csrc/dt_align.hip and this file alone (host code instrumented);
// run by tests/test_align_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/dt_hip_align.h"
#define EXPECT(expr, want) do { long long g = (long long)(expr); if (g != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, g, (long long)(want)); ++bad; } } while (0)
int main() {
  int bad = 0;
  std::vector<double> buf(64);
  void *p = buf.data();
  float *f = (float *)p; double *d = (double *)p; int *i = (int *)p;
  for (int na : {2, 3, 51, 129, 1024}) for (int nb : {2, 65, 1001, 1024}) for (int wp = 0; wp < 2; ++wp) for (int cg = 0; cg < 2; ++cg) {
    size_t one = dt_align_min_workspace_bytes(na, nb, wp, cg);
    size_t blocks = (size_t)(na + nb - 1 + 7) / 8;
    size_t need = (cg ? 0 : (size_t)8 * na * nb) + (wp ? 8 * blocks * na : 0);
    if (one < need || one == 0 || one % 16) { std::printf("FAIL ws %d %d %d %d\n", na, nb, wp, cg); ++bad; }
    EXPECT(dt_align_workspace_bytes(65535, na, nb, wp, cg), 65535 * one);
  }
  EXPECT(dt_align_workspace_bytes(0, 5, 5, 1, 0), 0);
  EXPECT(dt_align_workspace_bytes(65536, 5, 5, 1, 0), 0);
  EXPECT(dt_align_min_workspace_bytes(1, 5, 1, 0), 0);
  EXPECT(dt_align_min_workspace_bytes(5, 1025, 1, 0), 0);
  EXPECT(dt_align_cost(nullptr, 4, 0, 4, f, 4, 0, 4, 1, 4, d, i, nullptr), DT_E_NULL);
  EXPECT(dt_align_cost(f, 1, 0, 4, f, 4, 0, 4, 1, 4, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_align_cost(f, 4, 0, 4, f, 4, 0, 4, 1, 0, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_align_cost(f, 4, 0, 4, f, 4, 0, 4, 70000, 4, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_align_cost((float *)((char *)p + 2), 4, 0, 4, f, 4, 0, 4, 1, 4, d, i, nullptr), DT_E_ARG);
  EXPECT(dt_align_dp(nullptr, 1, 2, 2, 0, 0, d, nullptr, nullptr, i, p, 64, nullptr), DT_E_NULL);
  EXPECT(dt_align_dp(d, 1, 2, 2, 0, 0, d, i, nullptr, i, p, 64, nullptr), DT_E_NULL);
  EXPECT(dt_align_dp(d, 1, 2, 1025, 0, 0, d, nullptr, nullptr, i, p, 64, nullptr), DT_E_SHAPE);
  EXPECT(dt_align_dp(d, 1, 2, 2, 7, 0, d, nullptr, nullptr, i, p, 64, nullptr), DT_E_ARG);
  EXPECT(dt_align_dp(d, 1, 2, 2, 0, -3, d, nullptr, nullptr, i, p, 64, nullptr), DT_E_ARG);
  EXPECT(dt_align_dp(d, 1, 2, 2, 0, DT_ALIGN_MAX_BAND + 1, d, nullptr, nullptr, i, p, 64, nullptr), DT_E_ARG);
  EXPECT(dt_align_dp(d, 1, 2, 2, 0, 0, d, i, i, i, p, 15, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_align_dp(d, 65535, 1024, 1024, 0, 0, d, i, i, i, p, 64, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 0, 0, nullptr, d, d, nullptr, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_ARG);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 4, 0, nullptr, d, d, nullptr, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_ARG);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 1, 0, nullptr, nullptr, d, nullptr, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_NULL);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 3, 0, nullptr, d, d, i, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_NULL);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 2, 0, nullptr, d, d, i, i, nullptr, nullptr, i, p, 512, nullptr), DT_E_ARG);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 4, 3, 0, nullptr, d, d, i, i, i, i, i, p, 8, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_align(f, 1025, 0, 4, f, 4, 0, 4, 1, 4, 3, 0, nullptr, d, d, nullptr, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_SHAPE);
  EXPECT(dt_align(f, 4, 0, 4, f, 4, 0, 4, 1, 1 << 29, 3, 0, nullptr, d, d, nullptr, nullptr, nullptr, nullptr, i, p, 512, nullptr), DT_E_SHAPE);
  std::printf(bad ? "%d failures\n" : "align host checks clean (%d)\n", bad);
  return bad != 0;
}
