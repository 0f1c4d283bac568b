// Host-side sanitizer driver of include/dt_hip_fid.h (the Fréchet distance of the FID stage): links the library's own
// translation units compiled with -Xarch_host -fsanitize=address,undefined (device code is NOT instrumented) and calls every
// entry point of that header on valid arguments, on each rejected shape and on each argument-error path.  The distance of
// three students against one shared teacher set is checked against a host restatement of the means and traces, against the
// bounds 0 <= cross <= sqrt(tr S_A tr S_B), and against the exact answer for a student that is the teacher shifted.
// Exit status 0 and "fid driver ok" on stdout mean no sanitizer report and no unexpected status or value.
// Built by distillation_trajectories_amd/csrc/build.py (build_fid_sanitizer_driver); run by tests/test_hip_fid.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <random>
#include <vector>

#include "../../include/dt_hip_fid.h"

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
  // one teacher set [nt][D] shared by P = 3 student sets [P][ns][D]; student 2 is the teacher's first ns rows plus 0.5
  const int P = 3, nt = 12, ns = 9, D = 40;
  std::mt19937 rng(7);
  std::normal_distribution<float> g(0.f, 1.f);
  std::vector<float> tch((size_t)nt * D), stu((size_t)P * ns * D);
  for (auto &x : tch) x = 3.f + g(rng);
  for (auto &x : stu) x = 3.2f + 1.5f * g(rng);
  for (int i = 0; i < ns; ++i)
    for (int e = 0; e < D; ++e) stu[((size_t)2 * ns + i) * D + e] = tch[(size_t)i * D + e] + 0.5f;
  float *t_d, *s_d;
  double *fid_d, *parts_d;
  int *st_d;
  HIP(hipMalloc((void **)&t_d, tch.size() * 4)); HIP(hipMalloc((void **)&s_d, stu.size() * 4));
  HIP(hipMalloc((void **)&fid_d, P * 8)); HIP(hipMalloc((void **)&parts_d, P * 4 * 8)); HIP(hipMalloc((void **)&st_d, P * 4));
  HIP(hipMemcpy(t_d, tch.data(), tch.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(s_d, stu.data(), stu.size() * 4, hipMemcpyHostToDevice));
  const size_t ws_bytes = dt_fid_workspace_bytes(P, nt, ns, D);
  EXPECT(ws_bytes > (size_t)P * (nt * ns + ns * ns) * 8);
  void *ws;
  HIP(hipMalloc(&ws, ws_bytes));
  HIP(hipMemset(ws, 0xff, ws_bytes));
  hipStream_t s;
  HIP(hipStreamCreate(&s));
  hipEvent_t ev[DT_FID_EVENTS];
  for (auto &e : ev) HIP(hipEventCreate(&e));
  void *evp[DT_FID_EVENTS];
  for (int i = 0; i < DT_FID_EVENTS; ++i) evp[i] = ev[i];
  const long long sp = (long long)ns * D;

  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, evp, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  float ms = -1.f;
  HIP(hipEventElapsedTime(&ms, ev[0], ev[DT_FID_EVENTS - 1]));
  EXPECT(ms >= 0.f);
  std::vector<double> fid(P), parts(P * 4);
  std::vector<int> st(P);
  HIP(hipMemcpy(fid.data(), fid_d, P * 8, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(parts.data(), parts_d, P * 4 * 8, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(st.data(), st_d, P * 4, hipMemcpyDeviceToHost));
  auto stats = [&](const float *x, int n, std::vector<double> &mu) {
    mu.assign(D, 0.0);
    for (int i = 0; i < n; ++i)
      for (int e = 0; e < D; ++e) mu[e] += x[(size_t)i * D + e];
    for (auto &m : mu) m /= n;
    double tr = 0.0;
    for (int i = 0; i < n; ++i)
      for (int e = 0; e < D; ++e) tr += (x[(size_t)i * D + e] - mu[e]) * (x[(size_t)i * D + e] - mu[e]);
    return tr / (n - 1);
  };
  std::vector<double> mu_t, mu_s;
  const double tr_t = stats(tch.data(), nt, mu_t);
  for (int p = 0; p < P; ++p) {
    EXPECT(st[p] == DT_FID_OK);
    const double tr_s = stats(stu.data() + (size_t)p * ns * D, ns, mu_s);
    double dmu = 0.0;
    for (int e = 0; e < D; ++e) dmu += (mu_t[e] - mu_s[e]) * (mu_t[e] - mu_s[e]);
    const double *q = parts.data() + 4 * p;
    EXPECT(std::fabs(q[0] - dmu) <= 1e-12 * (dmu + 1.0));
    EXPECT(std::fabs(q[1] - tr_t) <= 1e-12 * tr_t && std::fabs(q[2] - tr_s) <= 1e-12 * tr_s);
    EXPECT(q[3] >= 0.0 && q[3] <= std::sqrt(tr_t * tr_s) * (1.0 + 1e-9));
    EXPECT(fid[p] == q[0] + q[1] + q[2] - 2.0 * q[3]);
  }
  // the same set against itself shifted by a constant: the covariances are equal, so fid = |shift|^2 = 0.25 D
  CHECK(dt_fid_distance(t_d, ns, 0, D, s_d + 2 * sp, ns, 0, D, 1, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  HIP(hipMemcpy(fid.data(), fid_d, 8, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(parts.data(), parts_d, 4 * 8, hipMemcpyDeviceToHost));
  EXPECT(std::fabs(fid[0] - 0.25 * D) <= 1e-5 * (parts[1] + parts[2]));

  // rejected shapes: the query returns 0 and the entry DT_E_SHAPE; nothing is launched
  EXPECT(dt_fid_workspace_bytes(0, nt, ns, D) == 0 && dt_fid_workspace_bytes(65536, nt, ns, D) == 0);
  EXPECT(dt_fid_workspace_bytes(P, 1, ns, D) == 0 && dt_fid_workspace_bytes(P, nt, 1, D) == 0);
  EXPECT(dt_fid_workspace_bytes(1, 2049, 2049, D) == 0 && dt_fid_workspace_bytes(1, 4000, 2048, D) > 0);
  EXPECT(dt_fid_workspace_bytes(P, nt, ns, D + 2) == 0 && dt_fid_workspace_bytes(P, nt, ns, 0) == 0);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, 0, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_fid_distance(t_d, 1, 0, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, 1, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_fid_distance(t_d, 2049, 0, D, s_d, 2049, sp, D, 1, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, P, D - 2, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  CHECK(dt_fid_distance(t_d, nt, -4, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_SHAPE);
  // argument errors
  CHECK(dt_fid_distance(nullptr, nt, 0, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_fid_distance(t_d, nt, 0, D, nullptr, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, P, D, nullptr, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, nullptr, ws_bytes, nullptr, s), DT_E_NULL);
  CHECK(dt_fid_distance(t_d + 1, nt, 0, D, s_d, ns, sp, D, P, D - 4, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_ARG);
  CHECK(dt_fid_distance(t_d, nt, 0, D + 2, s_d, ns, sp, D, P, D - 4, fid_d, parts_d, st_d, ws, ws_bytes, nullptr, s), DT_E_ARG);
  CHECK(dt_fid_distance(t_d, nt, 0, D, s_d, ns, sp, D, P, D, fid_d, parts_d, st_d, ws, ws_bytes - 8, nullptr, s), DT_E_WORKSPACE);
  HIP(hipStreamSynchronize(s));
  for (auto &e : ev) HIP(hipEventDestroy(e));
  (void)hipFree(t_d); (void)hipFree(s_d); (void)hipFree(fid_d); (void)hipFree(parts_d); (void)hipFree(st_d); (void)hipFree(ws);
  HIP(hipStreamDestroy(s));
  printf("fid driver ok (abi %d)\n", dt_abi_version());
  return 0;
}
