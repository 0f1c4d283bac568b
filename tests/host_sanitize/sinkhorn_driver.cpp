// Host-side walk of include/dt_hip_sinkhorn.h under AddressSanitizer and UndefinedBehaviorSanitizer: the size query and
// every argument error of the two entry points.  All of them return before any HIP call, so the program needs no GPU.
// Built by csrc/build.py::build_sinkhorn_sanitizer_driver from csrc/dt_sinkhorn.hip, csrc/dt_profile.hip and this file (host
// code instrumented); run by tests/test_sinkhorn_host.py.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include "../../include/dt_hip_sinkhorn.h"
#define EXPECT(expr, want) do { long long g_ = (long long)(expr); if (g_ != (long long)(want)) { std::printf("FAIL %s = %lld, want %lld\n", #expr, g_, (long long)(want)); ++bad; } } while (0)
int main() {
  int bad = 0;
  std::vector<double> buf(64);
  void *v = buf.data();
  float *f = (float *)v; double *d = (double *)v; int *i = (int *)v;
  float *f2 = (float *)((char *)v + 2); double *d4 = (double *)((char *)v + 4); int *i2 = (int *)((char *)v + 2);
  void *v8 = (char *)v + 8;
  const size_t big = (size_t)1 << 30;
  for (int P : {1, 3, 51, 1 << 16}) for (int na : {1, 7, 256, 2048}) for (int nb : {1, 5, 2048}) {
    const size_t one = dt_sinkhorn_workspace_bytes(1, na, nb), all = dt_sinkhorn_workspace_bytes(P, na, nb);
    if (one < (size_t)8 * ((size_t)na * nb + na + 2 * nb) || one % 8 || all != (size_t)P * one) {
      std::printf("FAIL ws %d %d %d\n", P, na, nb); ++bad;
    }
  }
  EXPECT(dt_sinkhorn_workspace_bytes(0, 4, 4), 0);
  EXPECT(dt_sinkhorn_workspace_bytes(-1, 4, 4), 0);
  EXPECT(dt_sinkhorn_workspace_bytes((1 << 16) + 1, 4, 4), 0);
  EXPECT(dt_sinkhorn_workspace_bytes(1, 0, 4), 0);
  EXPECT(dt_sinkhorn_workspace_bytes(1, 2049, 4), 0);
  EXPECT(dt_sinkhorn_workspace_bytes(1, 4, 0), 0);
  EXPECT(dt_sinkhorn_workspace_bytes(1, 4, 2049), 0);
  const size_t least = dt_sinkhorn_workspace_bytes(1, 2, 3);
  // dt_sinkhorn_mean_cost(a, a_ps, a_rs, n_a, b, b_ps, b_rs, n_b, E, P, p, mean_cost, status, ws, ws_bytes, stream)
  EXPECT(dt_sinkhorn_mean_cost(nullptr, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, nullptr, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, nullptr, i, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, nullptr, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 0, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2049, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 0, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 2049, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 0, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, (1 << 20) + 1, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 0, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, (1 << 16) + 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, -1, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, -4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, -1, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, -4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_mean_cost(f2, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f2, 0, 4, 3, 4, 1, 2, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 0, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 3, d, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d4, i, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i2, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v8, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, i, v, least - 1, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_sinkhorn_mean_cost(f, 0, 4, 2, f, 0, 4, 3, 4, 7, 2, d, i, v, 0, nullptr), DT_E_WORKSPACE);
  // dt_sinkhorn_ot(a, a_ps, a_rs, n_a, b, b_ps, b_rs, n_b, E, P, p, eps, max_iter, tol, ot, err, iters, status, f, g, ws, ws_bytes, stream)
  EXPECT(dt_sinkhorn_ot(nullptr, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, nullptr, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, nullptr, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, nullptr, d, i, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, nullptr, i, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, nullptr, i, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, nullptr, d, d, v, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, nullptr, nullptr, nullptr, big, nullptr), DT_E_NULL);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 0, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2049, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 0, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 2049, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 0, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, (1 << 20) + 1, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 0, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, (1 << 16) + 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 0, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, DT_SINKHORN_MAX_ITER + 1, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, -1, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, -4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_SHAPE);
  EXPECT(dt_sinkhorn_ot(f2, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f2, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 0, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 3, d, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, -1e-9, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, (double)INFINITY, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, (double)NAN, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d4, 5, 0.0, d, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d4, d, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d4, i, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i2, i, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i2, d, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, d4, d, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, nullptr, d4, v, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 0.0, d, d, i, i, nullptr, nullptr, v8, big, nullptr), DT_E_ARG);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 1, 2, d, 5, 1e-9, d, d, i, i, nullptr, nullptr, v, least - 1, nullptr), DT_E_WORKSPACE);
  EXPECT(dt_sinkhorn_ot(f, 0, 4, 2, f, 0, 4, 3, 4, 7, 2, d, 5, 1e-9, d, d, i, i, d, d, v, 0, nullptr), DT_E_WORKSPACE);
  std::printf(bad ? "%d failures\n" : "sinkhorn host checks clean (%d)\n", bad);
  return bad != 0;
}
