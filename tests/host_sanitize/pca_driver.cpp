// Host-side sanitizer driver of include/dt_hip_pca.h (the dimensionality-analysis PCA): links the library's own translation
// units compiled with -Xarch_host -fsanitize=address,undefined (device code is NOT instrumented) and calls every entry point
// of that header on valid arguments and on each argument-error path.  The fit of a small two-set problem is checked for
// unit-norm, mutually orthogonal components, ordered variances, the sign rule, and scores that dt_pca_project reproduces.
// Exit status 0 and "pca driver ok" on stdout mean no sanitizer report and no unexpected status or value.
// Built by distillation_trajectories_amd/csrc/build.py (build_pca_sanitizer_driver); run by tests/test_hip_pca.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/dt_hip_pca.h"

#define CHECK(expr, want)                                                                      \
  do {                                                                                         \
    const int _st = (expr);                                                                    \
    if (_st != (want)) { fprintf(stderr, "%s:%d: %s -> %d (%s), wanted %d\n", __FILE__, __LINE__, #expr, _st, dt_status_string(_st), (want)); return 1; } \
  } while (0)
#define HIP(expr)                                                                              \
  do {                                                                                         \
    const hipError_t _e = (expr);                                                              \
    if (_e != hipSuccess) { fprintf(stderr, "%s:%d: %s -> %s\n", __FILE__, __LINE__, #expr, hipGetErrorString(_e)); return 1; } \
  } while (0)
#define EXPECT(cond)                                                                           \
  do {                                                                                         \
    if (!(cond)) { fprintf(stderr, "%s:%d: %s does not hold\n", __FILE__, __LINE__, #cond); return 1; } \
  } while (0)

int main() {
  int n_dev = 0;
  HIP(hipGetDeviceCount(&n_dev));
  if (n_dev < 1) { fprintf(stderr, "no HIP device\n"); return 2; }
  // P = 3 problems of step-major sets X [nx][P][E], Y [ny][P][E]: random walks
  const int P = 3, nx = 9, ny = 6, n = nx + ny, E = 48, k = 3;
  std::mt19937 rng(7);
  std::normal_distribution<float> g(0.f, 1.f);
  std::vector<float> x((size_t)nx * P * E), y((size_t)ny * P * E);
  for (int p = 0; p < P; ++p)
    for (int e = 0; e < E; ++e) {
      float a = 0.f, b = 0.f;
      for (int i = 0; i < nx; ++i) x[((size_t)i * P + p) * E + e] = a += g(rng);
      for (int i = 0; i < ny; ++i) y[((size_t)i * P + p) * E + e] = b += g(rng);
    }
  float *x_d, *y_d, *mean_d, *comp_d, *scores_d, *proj_d;
  double *sv_d, *var_d, *ratio_d;
  int *st_d;
  HIP(hipMalloc((void **)&x_d, x.size() * 4)); HIP(hipMalloc((void **)&y_d, y.size() * 4));
  HIP(hipMalloc((void **)&mean_d, (size_t)P * E * 4)); HIP(hipMalloc((void **)&comp_d, (size_t)P * k * E * 4));
  HIP(hipMalloc((void **)&scores_d, (size_t)P * n * k * 4)); HIP(hipMalloc((void **)&proj_d, (size_t)P * n * k * 4));
  HIP(hipMalloc((void **)&sv_d, P * k * 8)); HIP(hipMalloc((void **)&var_d, P * k * 8));
  HIP(hipMalloc((void **)&ratio_d, P * k * 8)); HIP(hipMalloc((void **)&st_d, P * 4));
  HIP(hipMemcpy(x_d, x.data(), x.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(y_d, y.data(), y.size() * 4, hipMemcpyHostToDevice));
  const size_t ws_bytes = dt_pca_workspace_bytes(P, n, E, k);
  EXPECT(ws_bytes > 0);
  void *ws;
  HIP(hipMalloc(&ws, ws_bytes));
  hipStream_t s;
  HIP(hipStreamCreate(&s));
  hipEvent_t ev[4];
  for (auto &e : ev) HIP(hipEventCreate(&e));
  void *evp[4] = {ev[0], ev[1], ev[2], ev[3]};
  const long long ps = E, rs = (long long)P * E;

  CHECK(dt_pca_fit(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d, ws,
                   ws_bytes, evp, s), DT_OK);
  CHECK(dt_pca_project(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d, E, comp_d, (long long)k * E, proj_d, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  float ms = -1.f;
  HIP(hipEventElapsedTime(&ms, ev[0], ev[3]));
  EXPECT(ms >= 0.f);
  std::vector<float> comp((size_t)P * k * E), scores((size_t)P * n * k), proj(scores.size());
  std::vector<double> sv(P * k), ratio(P * k);
  std::vector<int> st(P);
  HIP(hipMemcpy(comp.data(), comp_d, comp.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(scores.data(), scores_d, scores.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(proj.data(), proj_d, proj.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(sv.data(), sv_d, sv.size() * 8, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(ratio.data(), ratio_d, ratio.size() * 8, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(st.data(), st_d, st.size() * 4, hipMemcpyDeviceToHost));
  for (int p = 0; p < P; ++p) {
    EXPECT(st[p] == DT_PCA_OK);
    double rsum = 0.0;
    for (int j = 0; j < k; ++j) {
      EXPECT(sv[p * k + j] > 0.0 && (j == 0 || sv[p * k + j] <= sv[p * k + j - 1]));
      rsum += ratio[p * k + j];
      const float *c = comp.data() + ((size_t)p * k + j) * E;
      int imax = 0;
      for (int e = 1; e < E; ++e)
        if (std::fabs(c[e]) > std::fabs(c[imax])) imax = e;
      EXPECT(c[imax] > 0.f);
      for (int jj = 0; jj <= j; ++jj) {
        const float *c2 = comp.data() + ((size_t)p * k + jj) * E;
        double dot = 0.0;
        for (int e = 0; e < E; ++e) dot += (double)c[e] * c2[e];
        EXPECT(std::fabs(dot - (jj == j ? 1.0 : 0.0)) < 1e-5);
      }
    }
    EXPECT(rsum > 0.0 && rsum <= 1.0 + 1e-12);
    float smax = 0.f;
    for (int q = 0; q < n * k; ++q) smax = std::fmax(smax, std::fabs(scores[(size_t)p * n * k + q]));
    for (int q = 0; q < n * k; ++q) EXPECT(std::fabs(scores[(size_t)p * n * k + q] - proj[(size_t)p * n * k + q]) <= 1e-5f * smax);
  }

  // argument errors: nothing is launched
  CHECK(dt_pca_fit(nullptr, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   ws, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_pca_fit(x_d, nx, ps, rs, nullptr, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   ws, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_pca_fit(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   nullptr, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_pca_fit(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, 17, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_pca_fit(x_d, 1, ps, rs, nullptr, 0, 0, 0, P, E, 1, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d, ws,
                   ws_bytes, nullptr, s), DT_E_SHAPE);                                            // n < 2
  CHECK(dt_pca_fit(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E - 2, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   ws, ws_bytes, nullptr, s), DT_E_SHAPE);                                        // E % 4
  CHECK(dt_pca_fit(x_d + 1, nx, ps, rs, y_d, ny, ps, rs, P, E - 4, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d,
                   st_d, ws, ws_bytes, nullptr, s), DT_E_ARG);                                    // not 16-byte aligned
  CHECK(dt_pca_fit(x_d, nx, ps, rs + 2, y_d, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d,
                   ws, ws_bytes, nullptr, s), DT_E_ARG);                                          // stride not a multiple of 4
  CHECK(dt_pca_fit(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d, comp_d, scores_d, sv_d, var_d, ratio_d, st_d, ws,
                   ws_bytes - 8, nullptr, s), DT_E_WORKSPACE);
  CHECK(dt_pca_project(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, 0, mean_d, E, comp_d, 0, proj_d, s), DT_E_SHAPE);
  CHECK(dt_pca_project(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, nullptr, E, comp_d, 0, proj_d, s), DT_E_NULL);
  CHECK(dt_pca_project(x_d, nx, ps, rs, y_d, ny, ps, rs, P, E, k, mean_d + 1, 0, comp_d, 0, proj_d, s), DT_E_ARG);
  EXPECT(dt_pca_workspace_bytes(P, n, E, 0) == 0 && dt_pca_workspace_bytes(P, 1, E, 1) == 0);
  HIP(hipStreamSynchronize(s));
  for (auto &e : ev) HIP(hipEventDestroy(e));
  (void)hipFree(x_d); (void)hipFree(y_d); (void)hipFree(mean_d); (void)hipFree(comp_d); (void)hipFree(scores_d);
  (void)hipFree(proj_d); (void)hipFree(sv_d); (void)hipFree(var_d); (void)hipFree(ratio_d); (void)hipFree(st_d);
  (void)hipFree(ws);
  HIP(hipStreamDestroy(s));
  printf("pca driver ok (abi %d)\n", dt_abi_version());
  return 0;
}
