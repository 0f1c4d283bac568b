// Host-side sanitizer driver of include/dt_hip_lpips.h (the perceptual distance): links the library's own translation
// units compiled with -Xarch_host -fsanitize=address,undefined (device code is NOT instrumented) and calls every entry point of
// that header on valid arguments and on each argument-error path: null pointers, C != 3, sizes outside 31..299, N < 1, a short
// workspace, misaligned and overlapping buffers, n0 that is neither 1 nor n1.
// On valid arguments it checks that the packs are finite and not all zero, that the layer-range entry over all layers gives
// the pack's last tap bit for bit, that d(x, x) == 0, and that the shared, the expanded and the many-groups calls agree bit for bit.
// Exit status 0 and "lpips driver ok" on stdout mean no sanitizer report and no unexpected status or value.
// Built by distillation_trajectories_amd/csrc/build.py (build_lpips_sanitizer_driver); run by tests/test_hip_lpips.py.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "../../include/dt_hip_lpips.h"

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
  std::uniform_real_distribution<float> u(0.f, 1.f);
  hipStream_t s;
  HIP(hipStreamCreate(&s));

  // table queries and their argument errors
  const int H = 35, W = 47;
  int hwc[3];
  CHECK(dt_lpips_layer_shape(H, W, 0, hwc), DT_OK);
  if (hwc[0] != 8 || hwc[1] != 11 || hwc[2] != 64) { fprintf(stderr, "tap 0: %d %d %d\n", hwc[0], hwc[1], hwc[2]); return 1; }
  CHECK(dt_lpips_layer_shape(H, W, 4, hwc), DT_OK);
  if (hwc[0] != 1 || hwc[1] != 2 || hwc[2] != 256) { fprintf(stderr, "tap 4: %d %d %d\n", hwc[0], hwc[1], hwc[2]); return 1; }
  CHECK(dt_lpips_layer_shape(30, W, 0, hwc), DT_E_SHAPE);
  CHECK(dt_lpips_layer_shape(H, 300, 0, hwc), DT_E_SHAPE);
  CHECK(dt_lpips_layer_shape(H, W, DT_LPIPS_N_LAYERS, hwc), DT_E_ARG);
  CHECK(dt_lpips_layer_shape(H, W, 0, nullptr), DT_E_NULL);
  const size_t F = dt_lpips_feature_floats(H, W);
  if (F != (size_t)8 * 11 * 64 + 3 * 5 * 192 + 2 * (384 + 256 + 256) || dt_lpips_feature_floats(30, 30) != 0) {
    fprintf(stderr, "feature_floats %zu\n", F);
    return 1;
  }

  // random weights: He-scaled convs, small biases, lin weights in [0, 1)
  const int desc[DT_LPIPS_N_LAYERS][3] = {{3, 64, 11}, {64, 192, 5}, {192, 384, 3}, {384, 256, 3}, {256, 256, 3}};
  std::vector<std::vector<float>> host;
  for (int l = 0; l < DT_LPIPS_N_LAYERS; ++l) {
    const int fan = desc[l][0] * desc[l][2] * desc[l][2];
    std::vector<float> w((size_t)desc[l][1] * fan), b(desc[l][1]);
    for (float &v : w) v = nd(rng) * std::sqrt(2.f / fan);
    for (float &v : b) v = 0.1f * nd(rng);
    host.push_back(w);
    host.push_back(b);
  }
  for (int l = 0; l < DT_LPIPS_N_LAYERS; ++l) {
    std::vector<float> w(desc[l][1]);
    for (float &v : w) v = u(rng);
    host.push_back(w);
  }
  std::vector<float *> bufs;
  std::vector<const float *> params;
  for (const std::vector<float> &v : host) {
    float *d;
    HIP(hipMalloc((void **)&d, v.size() * 4));
    HIP(hipMemcpy(d, v.data(), v.size() * 4, hipMemcpyHostToDevice));
    bufs.push_back(d);
    params.push_back(d);
  }
  dt_lpips *h = nullptr;
  CHECK(dt_lpips_create(nullptr, (int)params.size(), s, &h), DT_E_NULL);
  CHECK(dt_lpips_create(params.data(), (int)params.size() - 1, s, &h), DT_E_ARG);
  CHECK(dt_lpips_create(params.data(), (int)params.size(), s, nullptr), DT_E_NULL);
  CHECK(dt_lpips_create(params.data(), (int)params.size(), s, &h), DT_OK);
  for (float *d : bufs) HIP(hipFree(d));       // the handle owns copies

  const int N = 3, C = 3;
  std::vector<float> img((size_t)N * C * H * W), scaled((size_t)N * H * W * 3);
  for (float &v : img) v = std::tanh(1.5f * nd(rng));
  const float shift[3] = {-.030f, -.088f, -.188f}, scale[3] = {.458f, .448f, .450f};
  for (int b = 0; b < N; ++b)
    for (int c = 0; c < 3; ++c)
      for (int p = 0; p < H * W; ++p)
        scaled[((size_t)b * H * W + p) * 3 + c] = (img[((size_t)b * 3 + c) * H * W + p] - shift[c]) / scale[c];
  float *img_d, *scaled_d, *pack_d, *pack2_d, *tap4_d, *dist_d, *layers_d;
  HIP(hipMalloc((void **)&img_d, img.size() * 4));
  HIP(hipMemcpy(img_d, img.data(), img.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMalloc((void **)&scaled_d, scaled.size() * 4));
  HIP(hipMemcpy(scaled_d, scaled.data(), scaled.size() * 4, hipMemcpyHostToDevice));
  HIP(hipMalloc((void **)&pack_d, (size_t)N * F * 4));
  HIP(hipMalloc((void **)&pack2_d, (size_t)2 * N * F * 4));
  HIP(hipMalloc((void **)&tap4_d, (size_t)N * 2 * 256 * 4));
  HIP(hipMalloc((void **)&dist_d, (size_t)4 * N * 4));
  HIP(hipMalloc((void **)&layers_d, (size_t)4 * N * DT_LPIPS_N_LAYERS * 4));
  const size_t ws_bytes = dt_lpips_workspace_bytes(h, N, H, W);
  if (ws_bytes == 0 || dt_lpips_workspace_bytes(nullptr, N, H, W) != 0 || dt_lpips_workspace_bytes(h, 0, H, W) != 0 ||
      dt_lpips_workspace_bytes(h, N, 30, W) != 0) {
    fprintf(stderr, "workspace_bytes\n");
    return 1;
  }
  void *ws;
  HIP(hipMalloc(&ws, ws_bytes));

  CHECK(dt_lpips_features(h, img_d, N, C, H, W, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_OK);
  CHECK(dt_lpips_run_layers(h, 0, DT_LPIPS_N_LAYERS, scaled_d, N, H, W, tap4_d, ws, ws_bytes, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  std::vector<float> pack((size_t)N * F), tap4((size_t)N * 2 * 256);
  HIP(hipMemcpy(pack.data(), pack_d, pack.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(tap4.data(), tap4_d, tap4.size() * 4, hipMemcpyDeviceToHost));
  int nonzero = 0;
  for (size_t i = 0; i < pack.size(); ++i) {
    if (!std::isfinite(pack[i])) { fprintf(stderr, "feature %zu not finite\n", i); return 1; }
    nonzero += pack[i] != 0.f;
  }
  if (nonzero == 0) { fprintf(stderr, "all features zero\n"); return 1; }
  for (int b = 0; b < N; ++b)
    if (memcmp(&pack[(size_t)b * F + F - 512], &tap4[(size_t)b * 512], 512 * 4)) { fprintf(stderr, "layer range != features (image %d)\n", b); return 1; }

  // pack2 = two groups: [pack reversed | pack]; distances shared / expanded / many
  for (int g = 0; g < 2; ++g)
    for (int b = 0; b < N; ++b)
      HIP(hipMemcpy(pack2_d + ((size_t)g * N + b) * F, pack_d + (size_t)(g == 0 ? N - 1 - b : b) * F, F * 4, hipMemcpyDeviceToDevice));
  std::vector<float> many(2 * N), lay(2 * N * DT_LPIPS_N_LAYERS), one(N), shared(N), expanded(N);
  CHECK(dt_lpips_distance_many(h, pack_d, pack2_d, N, 2, H, W, dist_d, layers_d, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  HIP(hipMemcpy(many.data(), dist_d, many.size() * 4, hipMemcpyDeviceToHost));
  HIP(hipMemcpy(lay.data(), layers_d, lay.size() * 4, hipMemcpyDeviceToHost));
  CHECK(dt_lpips_distance(h, pack_d, N, pack2_d, N, H, W, dist_d, nullptr, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  HIP(hipMemcpy(one.data(), dist_d, one.size() * 4, hipMemcpyDeviceToHost));
  CHECK(dt_lpips_distance(h, pack_d, 1, pack2_d, N, H, W, dist_d, nullptr, s), DT_OK);
  HIP(hipStreamSynchronize(s));
  HIP(hipMemcpy(shared.data(), dist_d, shared.size() * 4, hipMemcpyDeviceToHost));
  for (int b = 0; b < N; ++b) {
    if (many[N + b] != 0.f) { fprintf(stderr, "d(x, x) = %g\n", many[N + b]); return 1; }
    if (memcmp(&many[b], &one[b], 4)) { fprintf(stderr, "many != distance at %d\n", b); return 1; }
    if (b != N - 1 - b && !(many[b] > 0.f && std::isfinite(many[b]))) { fprintf(stderr, "d[%d] = %g\n", b, many[b]); return 1; }
    float sum = 0.f;
    for (int l = 0; l < DT_LPIPS_N_LAYERS; ++l) sum += lay[(size_t)b * DT_LPIPS_N_LAYERS + l];
    if (std::fabs(sum - many[b]) > 1e-5f * many[b]) { fprintf(stderr, "layers do not sum to the distance at %d\n", b); return 1; }
  }
  if (memcmp(&many[0], &many[N - 1], 4)) { fprintf(stderr, "d(a, b) != d(b, a)\n"); return 1; }     // pairs (0, N-1) and (N-1, 0)
  // shared: pack[0] against pack2[0][b] = pack[N - 1 - b], so pair N - 1 is (pack[0], pack[0]) and pair 0 the expanded call's
  if (shared[N - 1] != 0.f || memcmp(&shared[0], &one[0], 4)) { fprintf(stderr, "shared reference\n"); return 1; }

  // argument errors: nothing is launched
  CHECK(dt_lpips_features(nullptr, img_d, N, C, H, W, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_E_NULL);
  CHECK(dt_lpips_features(h, img_d, N, C, H, W, 1.f, 0.f, pack_d, nullptr, ws_bytes, s), DT_E_NULL);
  CHECK(dt_lpips_features(h, img_d, N, 1, H, W, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_E_SHAPE);      // C != 3
  CHECK(dt_lpips_features(h, img_d, N, C, 30, W, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_lpips_features(h, img_d, N, C, H, 300, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_lpips_features(h, img_d, 0, C, H, W, 1.f, 0.f, pack_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_lpips_features(h, img_d, N, C, H, W, 1.f, 0.f, pack_d, ws, ws_bytes - 4, s), DT_E_WORKSPACE);
  CHECK(dt_lpips_features(h, img_d, N, C, H, W, 1.f, 0.f, pack_d + 1, ws, ws_bytes, s), DT_E_ARG);    // not 16-byte aligned
  CHECK(dt_lpips_features(h, img_d, N, C, H, W, 1.f, 0.f, (float *)ws, ws, ws_bytes, s), DT_E_ARG);   // pack inside the workspace
  CHECK(dt_lpips_run_layers(nullptr, 0, 1, scaled_d, N, H, W, tap4_d, ws, ws_bytes, s), DT_E_NULL);
  CHECK(dt_lpips_run_layers(h, 3, 3, scaled_d, N, H, W, tap4_d, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_lpips_run_layers(h, 0, DT_LPIPS_N_LAYERS + 1, scaled_d, N, H, W, tap4_d, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_lpips_run_layers(h, 0, 1, scaled_d, 0, H, W, pack_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_lpips_run_layers(h, 0, 1, scaled_d, N, 30, 30, pack_d, ws, ws_bytes, s), DT_E_SHAPE);
  CHECK(dt_lpips_run_layers(h, 0, 1, scaled_d, N, H, W, pack_d, ws, ws_bytes - 4, s), DT_E_WORKSPACE);
  CHECK(dt_lpips_run_layers(h, 0, 1, scaled_d + 1, N, H, W, pack_d, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_lpips_run_layers(h, 0, 1, scaled_d, N, H, W, (float *)ws, ws, ws_bytes, s), DT_E_ARG);
  CHECK(dt_lpips_distance(nullptr, pack_d, N, pack2_d, N, H, W, dist_d, nullptr, s), DT_E_NULL);
  CHECK(dt_lpips_distance(h, pack_d, N, pack2_d, N, H, W, nullptr, nullptr, s), DT_E_NULL);
  CHECK(dt_lpips_distance(h, pack_d, 2, pack2_d, 3, H, W, dist_d, nullptr, s), DT_E_ARG);
  CHECK(dt_lpips_distance(h, pack_d, 1, pack2_d, 0, H, W, dist_d, nullptr, s), DT_E_ARG);
  CHECK(dt_lpips_distance(h, pack_d, N, pack2_d, N, 30, W, dist_d, nullptr, s), DT_E_SHAPE);
  CHECK(dt_lpips_distance(h, pack_d, N, pack2_d, N, H, W, pack_d, nullptr, s), DT_E_ARG);             // output over an input
  CHECK(dt_lpips_distance_many(h, pack_d, pack2_d, N, 0, H, W, dist_d, layers_d, s), DT_E_ARG);
  CHECK(dt_lpips_distance_many(h, pack_d, nullptr, N, 2, H, W, dist_d, layers_d, s), DT_E_NULL);
  CHECK(dt_lpips_distance_many(h, pack_d, pack2_d, N, 2, 300, W, dist_d, layers_d, s), DT_E_SHAPE);
  CHECK(dt_lpips_distance_many(h, pack_d, pack2_d, N, 2, H, W, dist_d, dist_d, s), DT_E_ARG);         // the two outputs overlap
  HIP(hipStreamSynchronize(s));

  dt_lpips_destroy(h);
  dt_lpips_destroy(nullptr);
  (void)hipFree(img_d); (void)hipFree(scaled_d); (void)hipFree(pack_d); (void)hipFree(pack2_d); (void)hipFree(tap4_d);
  (void)hipFree(dist_d); (void)hipFree(layers_d); (void)hipFree(ws);
  HIP(hipStreamDestroy(s));
  printf("lpips driver ok (abi %d)\n", dt_abi_version());
  return 0;
}
