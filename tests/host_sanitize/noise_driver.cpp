// Host-side sanitizer driver of include/dt_hip_noise.h (the noise-prediction entry points): links the library's own translation
// units compiled with -Xarch_host -fsanitize=address,undefined (device code is NOT instrumented) and calls every entry point of
// that header on valid arguments and on each argument-error path, checking the noised rows against a host computation.
// Exit status 0 and "noise driver ok" on stdout mean no sanitizer report and no unexpected status or value.
// Built by distillation_trajectories_amd/csrc/build.py (build_noise_sanitizer_driver); run by tests/test_hip_noise_analysis.py.
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/dt_hip_noise.h"

#pragma clang fp contract(off)

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

int main() {
  int n_dev = 0;
  HIP(hipGetDeviceCount(&n_dev));
  if (n_dev < 1) { fprintf(stderr, "no HIP device\n"); return 2; }
  const int G = 5, B = 3, E = 3 * 16 * 16;
  std::mt19937 rng(99);
  std::uniform_real_distribution<float> d(-2.f, 2.f), u(0.f, 1.f);
  std::vector<float> x0(B * E), z((size_t)G * B * E), coef(2 * G), out((size_t)G * B * E);
  for (float &v : x0) v = d(rng);
  for (float &v : z) v = d(rng);
  for (float &v : coef) v = u(rng);
  float *x0_d, *z_d, *coef_d, *out_d;
  HIP(hipMalloc((void **)&x0_d, x0.size() * 4)); HIP(hipMalloc((void **)&z_d, z.size() * 4));
  HIP(hipMalloc((void **)&coef_d, coef.size() * 4)); HIP(hipMalloc((void **)&out_d, out.size() * 4));
  HIP(hipMemcpy(x0_d, x0.data(), x0.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(z_d, z.data(), z.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMemcpy(coef_d, coef.data(), coef.size() * 4, hipMemcpyHostToDevice));
  hipStream_t s;
  HIP(hipStreamCreate(&s));

  CHECK(dt_q_sample(x0_d, z_d, coef_d, G, B, E, out_d, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  HIP(hipMemcpy(out.data(), out_d, out.size() * 4, hipMemcpyDeviceToHost));
  for (int g = 0; g < G; ++g)
    for (int i = 0; i < B * E; ++i) {
      const float a = coef[2 * g] * x0[i], b = coef[2 * g + 1] * z[(size_t)g * B * E + i], want = a + b;
      const float got = out[(size_t)g * B * E + i];
      if (memcmp(&got, &want, 4)) { fprintf(stderr, "group %d element %d: %.9g vs %.9g\n", g, i, got, want); return 1; }
    }
  // argument errors: nothing is launched
  CHECK(dt_q_sample(nullptr, z_d, coef_d, G, B, E, out_d, s), DT_E_NULL);
  CHECK(dt_q_sample(x0_d, z_d, nullptr, G, B, E, out_d, s), DT_E_NULL);
  CHECK(dt_q_sample(x0_d, z_d, coef_d, 0, B, E, out_d, s), DT_E_SHAPE);
  CHECK(dt_q_sample(x0_d, z_d, coef_d, G, B, E - 2, out_d, s), DT_E_SHAPE);
  CHECK(dt_q_sample(x0_d + 1, z_d, coef_d, G, B, E - 4, out_d, s), DT_E_ARG);        // not 16-byte aligned
  HIP(hipStreamSynchronize(s));
  (void)hipFree(x0_d); (void)hipFree(z_d); (void)hipFree(coef_d); (void)hipFree(out_d);
  HIP(hipStreamDestroy(s));
  printf("noise driver ok (abi %d)\n", dt_abi_version());
  return 0;
}
