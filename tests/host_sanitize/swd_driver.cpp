// Host-side walk of include/dt_hip_swd.h under AddressSanitizer and UndefinedBehaviorSanitizer: the size queries and every
// argument error of the three entry points.  All of them return before any HIP call, so the program needs no GPU.
// Built by csrc/build.py::build_swd_sanitizer_driver from csrc/dt_swd.hip, csrc/dt_profile.hip and this file (host code
// instrumented); run by tests/test_swd_host.py.
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/dt_hip_swd.h"
#define EXPECT(expr, want) do { long long g = (long long)(expr); if (g != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, g, (long long)(want)); ++bad; } } while (0)
int main() {
  int bad = 0;
  std::vector<double> buf(64);
  void *v = buf.data();
  float *f = (float *)v; double *d = (double *)v; int *i = (int *)v;
  float *f2 = (float *)((char *)v + 2); double *d4 = (double *)((char *)v + 4); int *i2 = (int *)((char *)v + 2);
  void *v8 = (char *)v + 8;
  const size_t big = (size_t)1 << 30;
  for (int P : {1, 3, 51, 1 << 16}) for (int n : {1, 7, 256, 2048}) for (int L : {1, 65, 512, 4096}) {
    EXPECT(dt_swd_sorted_bytes(P, n, L), (size_t)8 * P * L * n);
    const size_t one = dt_swd_workspace_bytes(1, n, 3, L), all = dt_swd_workspace_bytes(P, n, 3, L);
    if (one < (size_t)8 * L * (n + 3 + 1) || one % 8 || all < one || all - one != (size_t)(P - 1) * 8 * L * (n + 3 + 1)) {
      std::printf("FAIL ws %d %d %d\n", P, n, L); ++bad;
    }
    EXPECT(dt_swd_distance_workspace_bytes(P, L), (size_t)8 * P * L);
  }
  EXPECT(dt_swd_sorted_bytes(0, 4, 4), 0);
  EXPECT(dt_swd_sorted_bytes((1 << 16) + 1, 4, 4), 0);
  EXPECT(dt_swd_sorted_bytes(1, 0, 4), 0);
  EXPECT(dt_swd_sorted_bytes(1, 2049, 4), 0);
  EXPECT(dt_swd_sorted_bytes(1, 4, 0), 0);
  EXPECT(dt_swd_sorted_bytes(1, 4, 4097), 0);
  EXPECT(dt_swd_sorted_bytes(-1, 4, 4), 0);
  EXPECT(dt_swd_workspace_bytes(1, 0, 4, 4), 0);
  EXPECT(dt_swd_workspace_bytes(1, 4, 2049, 4), 0);
  EXPECT(dt_swd_workspace_bytes(0, 4, 4, 4), 0);
  EXPECT(dt_swd_workspace_bytes(1, 4, 4, 4097), 0);
  EXPECT(dt_swd_distance_workspace_bytes(0, 4), 0);
  EXPECT(dt_swd_distance_workspace_bytes(1, 0), 0);
  EXPECT(dt_swd_distance_workspace_bytes(1, 4097), 0);
  // dt_swd_sorted(x, x_ps, x_rs, n, E, theta, theta_rs, L, P, sorted, status, ws, ws_bytes, stream)
  EXPECT(dt_swd_sorted(nullptr, 0, 4, 2, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, nullptr, 4, 3, 1, d, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, nullptr, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d, nullptr, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_sorted(f, 0, 4, 0, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2049, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 0, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, (1 << 20) + 1, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 0, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 4097, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 0, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, (1 << 16) + 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, -1, 4, 2, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, -4, 2, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, -4, 3, 1, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_sorted(f2, 0, 4, 2, 4, f, 4, 3, 1, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f2, 4, 3, 1, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d4, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d, i2, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d, i, v8, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_sorted(f, 0, 4, 2, 4, f, 4, 3, 1, d, i, v, DT_SWD_SORTED_WORKSPACE_BYTES - 1, nullptr), DT_E_WORKSPACE);
  // dt_swd_distance(sa, sa_ps, status_a, n_a, sb, sb_ps, status_b, n_b, L, P, p, w, mean_w, max_w, argmax, status, ws, ws_bytes, stream)
  EXPECT(dt_swd_distance(nullptr, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, nullptr, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, nullptr, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, nullptr, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, nullptr, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, nullptr, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, d, nullptr, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, nullptr, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd_distance(d, 0, i, 0, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 2049, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 0, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 0, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_distance(d, 7, i, 2, d, 0, i, 3, 4, 2, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);   // 0 < stride < L*n_a
  EXPECT(dt_swd_distance(d, 0, i, 2, d, -12, i, 3, 4, 2, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 0, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 3, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d4, 0, i, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i2, 2, d, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d4, 0, i, 3, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, d4, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, nullptr, d4, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, nullptr, d, d, i2, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, nullptr, d, d, i, i, v8, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd_distance(d, 0, i, 2, d, 0, i, 3, 4, 1, 2, nullptr, d, d, i, i, v, dt_swd_distance_workspace_bytes(1, 4) - 1, nullptr), DT_E_WORKSPACE);
  // dt_swd(a, a_ps, a_rs, n_a, b, b_ps, b_rs, n_b, E, theta, theta_rs, L, P, p, w, mean_w, max_w, argmax, status, ws, ws_bytes, stream)
  EXPECT(dt_swd(nullptr, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 2, nullptr, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, nullptr, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, nullptr, d, i, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, nullptr, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_swd(f, 0, 4, 0, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 2049, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 0, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, (1 << 20) + 1, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4097, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, (1 << 16) + 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, -1, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, -1, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, -4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 0, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 3, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f2, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f2, 0, 4, 3, 4, f, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f2, 4, 4, 1, 2, d, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, d4, d, d, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, nullptr, d, d4, i, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, nullptr, d, d, i, i2, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, nullptr, d, d, i, i, v8, big, nullptr), DT_E_ARG);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 1, 2, nullptr, d, d, i, i, v, dt_swd_workspace_bytes(1, 2, 3, 4) - 1, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_swd(f, 0, 4, 2, f, 0, 4, 3, 4, f, 4, 4, 7, 2, nullptr, d, d, i, i, v, 0, nullptr), DT_E_WORKSPACE);
  std::printf(bad ? "%d failures\n" : "swd host checks clean (%d)\n", bad);
  return bad != 0;
}
