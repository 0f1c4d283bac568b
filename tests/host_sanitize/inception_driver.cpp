// Host-side sanitizer driver of include/dt_hip_inception.h (the FID feature extractor): links the library's own translation
// units compiled with -Xarch_host -fsanitize=address,undefined (device code is NOT instrumented) and calls every entry point of
// that header on valid arguments and on each argument-error path: a null handle, C != 3, H > 299, B < 1, a short workspace.
// On valid arguments it checks that the features are finite and that preprocessing + the module-range entry over all modules
// gives the features bit for bit.  Exit status 0 and "inception driver ok" on stdout mean no sanitizer report and no
// unexpected status or value.
// Built by distillation_trajectories_amd/csrc/build.py (build_inception_sanitizer_driver); run by tests/test_hip_inception.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/dt_hip_inception.h"

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
  std::mt19937 rng(7);
  std::normal_distribution<float> nd(0.f, 1.f);
  std::uniform_real_distribution<float> u(0.5f, 1.5f);
  hipStream_t s;
  HIP(hipStreamCreate(&s));

  // table queries and their argument errors
  int desc[7], in_hwc[3], out_hwc[3];
  CHECK(dt_inception_conv_desc(0, desc), DT_OK);
  if (desc[0] != 3 || desc[1] != 32 || desc[4] != 2) { fprintf(stderr, "conv 0: %d %d %d\n", desc[0], desc[1], desc[4]); return 1; }
  CHECK(dt_inception_conv_desc(DT_INCEPTION_N_CONVS, desc), DT_E_ARG);
  CHECK(dt_inception_conv_desc(-1, desc), DT_E_ARG);
  CHECK(dt_inception_conv_desc(0, nullptr), DT_E_NULL);
  CHECK(dt_inception_module_shape(DT_INCEPTION_N_MODULES - 1, in_hwc, out_hwc), DT_OK);
  if (in_hwc[2] != 2048 || out_hwc[2] != DT_INCEPTION_FEATURES) { fprintf(stderr, "avgpool shape\n"); return 1; }
  CHECK(dt_inception_module_shape(DT_INCEPTION_N_MODULES, in_hwc, out_hwc), DT_E_ARG);
  CHECK(dt_inception_module_shape(0, nullptr, out_hwc), DT_E_NULL);

  // random weights, He-scaled, BatchNorm near identity
  std::vector<float *> bufs;
  std::vector<const float *> params;
  for (int i = 0; i < DT_INCEPTION_N_CONVS; ++i) {
    CHECK(dt_inception_conv_desc(i, desc), DT_OK);
    const int cout = desc[1], fan = desc[0] * desc[2] * desc[3];
    std::vector<std::vector<float>> host(5);
    host[0].resize((size_t)cout * fan);
    for (float &v : host[0]) v = nd(rng) * std::sqrt(2.f / fan);
    for (int k = 1; k < 5; ++k) host[k].resize(cout);
    for (int c = 0; c < cout; ++c) host[1][c] = u(rng), host[2][c] = 0.1f * nd(rng), host[3][c] = 0.f, host[4][c] = u(rng);
    for (int k = 0; k < 5; ++k) {
      float *d;
      HIP(hipMalloc((void **)&d, host[k].size() * 4));
      HIP(hipMemcpy(d, host[k].data(), host[k].size() * 4, hipMemcpyHostToDevice));
      bufs.push_back(d);
      params.push_back(d);
    }
  }
  dt_inception *h = nullptr;
  CHECK(dt_inception_create(nullptr, (int)params.size(), s, &h), DT_E_NULL);
  CHECK(dt_inception_create(params.data(), (int)params.size() - 1, s, &h), DT_E_ARG);
  CHECK(dt_inception_create(params.data(), (int)params.size(), s, nullptr), DT_E_NULL);
  CHECK(dt_inception_create(params.data(), (int)params.size(), s, &h), DT_OK);
  for (float *d : bufs) HIP(hipFree(d));       // the handle owns copies

  const int B = 2, C = 3, H = 16, W = 24;
  std::vector<float> img((size_t)B * C * H * W);
  for (float &v : img) v = std::tanh(nd(rng));
  float *img_d, *pre_d, *feat_d, *feat2_d;
  HIP(hipMalloc((void **)&img_d, img.size() * 4));
  HIP(hipMemcpy(img_d, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMalloc((void **)&pre_d, (size_t)B * DT_INCEPTION_SIZE * DT_INCEPTION_SIZE * 3 * 4));
  HIP(hipMalloc((void **)&feat_d, (size_t)B * DT_INCEPTION_FEATURES * 4));
  HIP(hipMalloc((void **)&feat2_d, (size_t)B * DT_INCEPTION_FEATURES * 4));
  const size_t ws_bytes = dt_inception_workspace_bytes(h, B);
  if (ws_bytes == 0 || dt_inception_workspace_bytes(nullptr, B) != 0 || dt_inception_workspace_bytes(h, 0) != 0) {
    fprintf(stderr, "workspace_bytes\n");
    return 1;
  }
  void *ws;
  HIP(hipMalloc(&ws, ws_bytes));

  CHECK(dt_inception_features(h, img_d, B, C, H, W, 0.5f, 0.5f, feat_d, ws, ws_bytes, s), DT_OK);
  CHECK(dt_inception_preprocess(img_d, B, C, H, W, 0.5f, 0.5f, pre_d, s), DT_OK);
  CHECK(dt_inception_run_modules(h, 0, DT_INCEPTION_N_MODULES, pre_d, B, feat2_d, ws, ws_bytes, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  std::vector<float> f1((size_t)B * DT_INCEPTION_FEATURES), f2(f1.size());
  HIP(hipMemcpy(f1.data(), feat_d, f1.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(f2.data(), feat2_d, f2.size() * 4, hipMemcpyDeviceToHost));
  int nonzero = 0;
  for (size_t i = 0; i < f1.size(); ++i) {
    if (!std::isfinite(f1[i])) { fprintf(stderr, "feature %zu not finite\n", i); return 1; }
    nonzero += f1[i] != 0.f;
  }
  if (nonzero == 0) { fprintf(stderr, "all features zero\n"); return 1; }
  if (memcmp(f1.data(), f2.data(), f1.size() * 4)) { fprintf(stderr, "module range != features\n"); return 1; }

  // argument errors: nothing is launched
  CHECK(dt_inception_features(nullptr, img_d, B, C, H, W, 1.f, 0.f, feat_d, ws, ws_bytes, s), DT_E_NULL);
  CHECK(dt_inception_features(h, img_d, B, 1, H, W, 1.f, 0.f, feat_d, ws, ws_bytes, s), DT_E_SHAPE);     // C != 3
  CHECK(dt_inception_features(h, img_d, B, C, 300, W, 1.f, 0.f, feat_d, ws, ws_bytes, s), DT_E_SHAPE);   // H > 299
  CHECK(dt_inception_features(h, img_d, B, C, H, 300, 1.f, 0.f, feat_d, ws, ws_bytes, s), DT_E_SHAPE);   // W > 299
  CHECK(dt_inception_features(h, img_d, 0, C, H, W, 1.f, 0.f, feat_d, ws, ws_bytes, s), DT_E_SHAPE);     // B < 1
  CHECK(dt_inception_features(h, img_d, B, C, H, W, 1.f, 0.f, feat_d, ws, ws_bytes - 4, s), DT_E_WORKSPACE);
  CHECK(dt_inception_features(h, img_d, B, C, H, W, 1.f, 0.f, feat_d, nullptr, ws_bytes, s), DT_E_NULL);
  CHECK(dt_inception_preprocess(nullptr, B, C, H, W, 1.f, 0.f, pre_d, s), DT_E_NULL);
  CHECK(dt_inception_preprocess(img_d, B, 4, H, W, 1.f, 0.f, pre_d, s), DT_E_SHAPE);
  CHECK(dt_inception_preprocess(img_d, B, C, 0, W, 1.f, 0.f, pre_d, s), DT_E_SHAPE);
  CHECK(dt_inception_run_modules(nullptr, 0, 1, pre_d, B, feat2_d, ws, ws_bytes, s), DT_E_NULL);
  CHECK(dt_inception_run_modules(h, 3, 3, pre_d, B, feat2_d, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_inception_run_modules(h, 0, DT_INCEPTION_N_MODULES + 1, pre_d, B, feat2_d, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_inception_run_modules(h, 0, 1, pre_d, 0, feat2_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_inception_run_modules(h, 0, 1, pre_d, B, feat2_d, ws, ws_bytes - 4, s), DT_E_WORKSPACE);
  CHECK(dt_inception_run_modules(h, 0, 1, pre_d + 1, B, feat2_d, ws, ws_bytes, s), DT_E_ARG);           // not 16-byte aligned
  HIP(hipStreamSynchronize(s));

  dt_inception_destroy(h);
  dt_inception_destroy(nullptr);
  (void)hipFree(img_d); (void)hipFree(pre_d); (void)hipFree(feat_d); (void)hipFree(feat2_d); (void)hipFree(ws);
  HIP(hipStreamDestroy(s));
  printf("inception driver ok (abi %d)\n", dt_abi_version());
  return 0;
}
