// Host-side walk of include/dt_hip_spectral.h under AddressSanitizer and UndefinedBehaviorSanitizer: the workspace query and
// every argument error of the three entry points.  All of them return before any HIP call, so the program needs no GPU.
// Built by csrc/build.py::build_spectral_sanitizer_driver from csrc/dt_spectral.hip, csrc/dt_profile.hip and this file (host
// code instrumented); run by tests/test_spectral_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/dt_hip_spectral.h"
#define EXPECT(expr, want) do { long long g = (long long)(expr); if (g != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, g, (long long)(want)); ++bad; } } while (0)
int main() {
  int bad = 0;
  std::vector<double> buf(64);
  void *p = buf.data();
  float *f = (float *)p; double *d = (double *)p; int *i = (int *)p;
  float *f2 = (float *)((char *)p + 2); double *d4 = (double *)((char *)p + 4); int *i2 = (int *)((char *)p + 2);
  const size_t big = 1 << 20;
  for (int H : {1, 2, 3, 28, 63, 64}) for (int W : {1, 5, 7, 28, 64}) for (int nb : {1, 46, 256}) {
    size_t ws = dt_spectral_workspace_bytes(H, W, nb);
    if (ws < (size_t)4 * (nb + 1 + H * W) || ws % 16) { std::printf("FAIL ws %d %d %d\n", H, W, nb); ++bad; }
    EXPECT(dt_spectral_workspace_bytes(H, W, 256), ws);   // it holds the widest table's bin starts
  }
  EXPECT(dt_spectral_workspace_bytes(0, 4, 4), 0);
  EXPECT(dt_spectral_workspace_bytes(4, 65, 4), 0);
  EXPECT(dt_spectral_workspace_bytes(4, 4, 0), 0);
  EXPECT(dt_spectral_workspace_bytes(4, 4, 257), 0);
  EXPECT(dt_spectral_workspace_bytes(-1, 4, 4), 0);
  // dt_spectral_power(a, ostride, istride, n_outer, n_inner, C, H, W, bin, n_bins, out, status, ws, ws_bytes, stream)
  EXPECT(dt_spectral_power(nullptr, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, nullptr, 3, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, nullptr, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, nullptr, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_power(f, 0, 16, 0, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 0, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1 << 13, 1 << 12, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 0, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 65, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 0, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 65, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 0, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 257, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, -1, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f, 0, -16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_power(f2, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i2, 3, d, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d4, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i2, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, d4, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, dt_spectral_workspace_bytes(4, 4, 3) - 1, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_spectral_power(f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, 0, nullptr), DT_E_WORKSPACE);
  // dt_spectral_pair(a, a_ostride, a_istride, b, b_ostride, b_istride, n_outer, n_inner, C, H, W, bin, n_bins, out, status, ws, ...)
  EXPECT(dt_spectral_pair(nullptr, 0, 16, f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_pair(f, 0, 16, nullptr, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, 16, 1, 2, 1, 65, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, 16, 1, 2, 64, 64, 64, i, 257, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_pair(f, 0, 16, f, -2, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, -1, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_pair(f, 0, 16, f2, 0, 16, 1, 2, 1, 4, 4, i, 3, d, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, 16, 1, 2, 1, 4, 4, i, 3, d4, i, p, big, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_pair(f, 0, 16, f, 0, 16, 1, 2, 1, 64, 64, i, 3, d, i, p, 4096, nullptr), DT_E_WORKSPACE);
  // dt_spectral_sum(out, status, n_outer, n_inner, C, n_bins, K, sum, count, stream)
  EXPECT(dt_spectral_sum(nullptr, i, 1, 2, 1, 3, 5, d, i, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_sum(d, nullptr, 1, 2, 1, 3, 5, d, i, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 3, 5, nullptr, i, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 3, 5, d, nullptr, nullptr), DT_E_NULL);
  EXPECT(dt_spectral_sum(d, i, 0, 2, 1, 3, 5, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_sum(d, i, 1, (1 << 24) + 1, 1, 3, 5, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 65, 3, 5, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 0, 5, d, i, nullptr), DT_E_SHAPE);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 3, 2, d, i, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_sum(d4, i, 1, 2, 1, 3, 5, d, i, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 3, 1, d4, i, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_sum(d, i2, 1, 2, 1, 3, 1, d, i, nullptr), DT_E_ARG);
  EXPECT(dt_spectral_sum(d, i, 1, 2, 1, 3, 1, d, i2, nullptr), DT_E_ARG);
  std::printf(bad ? "%d failures\n" : "spectral host checks clean (%d)\n", bad);
  return bad != 0;
}
