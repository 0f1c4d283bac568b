/*
 * dt_hip_lpips.h -- entry points of libdt_hip.so for the perceptual distance (evaluation/metrics.py compute_lpips,
 * analysis/metrics/perceptual.py): LPIPS v0.1 with net='alex', i.e. torchvision AlexNet `features` up to the fifth ReLU,
 * channel-normalised differences of the five ReLU maps weighted by the 1x1 "lin" layers, averaged over pixels and summed
 * over layers.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32, a stream argument, asynchronous (dt_lpips_create
 * excepted), int status (0 ok, <0 DT_E_*, >0 a hipError_t); only dt_lpips_create allocates device memory; scratch comes
 * from the caller (workspace).  An argument error launches nothing.
 *
 * The network.  Input x in [-1, 1], [N][3][H][W]; scaling layer (x - shift) / scale with shift (-.030, -.088, -.188) and
 * scale (.458, .448, .450).  Layers, each ending in bias + ReLU (the five "taps"):
 *    0 conv 3->64 k11 s4 p2            1 max pool 3x3 s2, conv 64->192 k5 p2    2 max pool 3x3 s2, conv 192->384 k3 p1
 *    3 conv 384->256 k3 p1             4 conv 256->256 k3 p1
 * Layer 0 takes the scaled image NHWC [N][H][W][3]; layer l > 0 takes tap l - 1.  31 <= H, W <= 299 (at 30 the second
 * pool has nothing to pool).
 *
 * Layouts.  Images are NCHW as the package holds them.  Every activation is NHWC.  The feature pack of one image is
 * its five taps, NHWC, one after another: dt_lpips_feature_floats(H, W) floats (a multiple of 64); a batch is [N][floats].
 * Every output element of a conv is one k-ordered fp32 fma chain (no split-K, no atomics), so an image's pack does not
 * depend on N or on the other images.
 */
#ifndef DT_HIP_LPIPS_H
#define DT_HIP_LPIPS_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_LPIPS_N_LAYERS 5
#define DT_LPIPS_N_PARAMS 15
#define DT_LPIPS_MIN_SIZE 31
#define DT_LPIPS_MAX_SIZE 299

typedef struct dt_lpips dt_lpips;

/* params: host array of 15 device pointers in forward order: conv_k.weight [cout][cin][kh][kw], conv_k.bias [cout] for
 * k = 1..5, then lin_0..lin_4 ([1][C_l][1][1], no bias).  The weights are copied and re-laid out into memory the handle
 * owns; the call synchronises `stream` before it returns, so the caller may free the inputs afterwards. */
int dt_lpips_create(const float *const *params, int n_params, void *stream, dt_lpips **out);
void dt_lpips_destroy(dt_lpips *h);

/* hwc = {H_l, W_l, C_l} of tap l for an H x W image.  DT_E_SHAPE for H or W outside 31..299, DT_E_ARG for l outside 0..4. */
int dt_lpips_layer_shape(int H, int W, int l, int *hwc);

/* Floats of one image's feature pack (0 for H or W outside 31..299). */
size_t dt_lpips_feature_floats(int H, int W);

/* Bytes of workspace dt_lpips_features and dt_lpips_run_layers need for N images of H x W (0 if h is NULL, N < 1 or the
 * size is out of range). */
size_t dt_lpips_workspace_bytes(const dt_lpips *h, int N, int H, int W);

/* images [N][C][H][W] -> pack_out [N][feature_floats]: v = in_scale * x + in_shift, the scaling layer, the five layers.
 * (in_scale, in_shift) = (2, -1) is compute_lpips' map from [0, 1]; (1, 0) takes [-1, 1] states as they are.
 * C must be 3.  pack_out and ws 16-byte aligned; images, pack_out and the workspace must not overlap. */
int dt_lpips_features(const dt_lpips *h, const float *images_dev, int N, int C, int H, int W, float in_scale,
                      float in_shift, float *pack_out, void *ws, size_t ws_bytes, void *stream);

/* Layers [first, last) for images of H x W on in_dev, the NHWC input of layer `first` (contiguous [N][..]); out_dev
 * receives tap last - 1, [N][H_l][W_l][C_l].  0 <= first < last <= 5; in_dev, out_dev 16-byte aligned, not inside the workspace. */
int dt_lpips_run_layers(const dt_lpips *h, int first, int last, const float *in_dev, int N, int H, int W, float *out_dev,
                        void *ws, size_t ws_bytes, void *stream);

/* dist_out[i] = sum_l mean_pixels sum_c w_lc (n0_c - n1_c)^2 with n = f / (sqrt(sum_c f_c^2) + 1e-10), between pack0[i]
 * (pack0[0] when n0 == 1) and pack1[i], i < n1; n0 must be 1 or n1.  layers_out: NULL or [n1][5], the five terms.
 * One pass: every feature value is read once; the difference form, fp64 sums in a fixed order rounded once, so that
 * d(x, x) == 0, d(a, b) == d(b, a) bit for bit, and a pair's bits do not depend on the batch or on sharing. */
int dt_lpips_distance(const dt_lpips *h, const float *pack0, int n0, const float *pack1, int n1, int H, int W,
                      float *dist_out, float *layers_out, void *stream);

/* pack0 [n][floats], pack1 [G][n][floats]: dist_out [G][n], layers_out NULL or [G][n][5]; pair (g, i) compares pack0[i]
 * with pack1[g][i], bit for bit as dt_lpips_distance would.  One launch. */
int dt_lpips_distance_many(const dt_lpips *h, const float *pack0, const float *pack1, int n, int G, int H, int W,
                           float *dist_out, float *layers_out, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_LPIPS_H */
