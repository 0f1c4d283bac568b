/*
 * dt_hip_inception.h -- entry points of libdt_hip.so for the FID feature extractor
 * (analysis/metrics/fid_score.py, evaluation/metrics.py): torchvision's Inception3 in eval mode with
 * transform_input=False and fc = Identity, i.e. the 2048 avgpool values per image.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32, a stream argument, asynchronous
 * (dt_inception_create excepted), int status (0 ok, <0 DT_E_*, >0 a hipError_t); only
 * dt_inception_create allocates device memory; scratch comes from the caller (workspace).
 *
 * Layouts.  Images are NCHW [B][3][H][W] as the reference holds them, 1 <= H, W <= 299 (upsampling only).
 * Every activation between modules is NHWC [B][H][W][C], contiguous, 16-byte aligned.  Modules, in forward order
 * (dt_inception_module_shape gives each one's input and output H, W, C):
 *    0 Conv2d_1a_3x3   1 Conv2d_2a_3x3   2 Conv2d_2b_3x3   3 max pool 3x3 s2   4 Conv2d_3b_1x1
 *    5 Conv2d_4a_3x3   6 max pool 3x3 s2 7 Mixed_5b  8 Mixed_5c  9 Mixed_5d  10 Mixed_6a  11 Mixed_6b
 *   12 Mixed_6c       13 Mixed_6d       14 Mixed_6e  15 Mixed_7a 16 Mixed_7b 17 Mixed_7c  18 avgpool ([B][2048])
 * Module 0 takes the preprocessed image [B][299][299][3] (dt_inception_preprocess).
 */
#ifndef DT_HIP_INCEPTION_H
#define DT_HIP_INCEPTION_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_INCEPTION_N_CONVS 94     /* BasicConv2d layers (conv without bias + BatchNorm eps 1e-3 + ReLU) */
#define DT_INCEPTION_N_MODULES 19
#define DT_INCEPTION_SIZE 299       /* every image is resized to 299 x 299 */
#define DT_INCEPTION_FEATURES 2048

typedef struct dt_inception dt_inception;

/* Shape of BasicConv2d i (0 <= i < DT_INCEPTION_N_CONVS, forward order = torchvision's module order):
 * desc = {cin, cout, kh, kw, stride, pad_h, pad_w}. */
int dt_inception_conv_desc(int i, int *desc7);

/* Input and output {H, W, C} of module m (the table above). */
int dt_inception_module_shape(int m, int *in_hwc, int *out_hwc);

/* params: host array of 5 * DT_INCEPTION_N_CONVS device pointers, five per BasicConv2d in conv_desc order:
 *   conv.weight [cout][cin][kh][kw], bn.weight, bn.bias, bn.running_mean, bn.running_var (each [cout]).
 * The weights are copied, re-laid out and BatchNorm-folded into memory the handle owns; the call synchronises
 * `stream` before it returns, so the caller may free the inputs afterwards. */
int dt_inception_create(const float *const *params, int n_params, void *stream, dt_inception **out);
void dt_inception_destroy(dt_inception *h);

/* Bytes of workspace dt_inception_features and dt_inception_run_modules need for a batch of B (0 if h is NULL or B < 1). */
size_t dt_inception_workspace_bytes(const dt_inception *h, int B);

/* images [B][C][H][W] -> out [B][299][299][3] NHWC:  v = in_scale * x + in_shift, half-pixel bilinear resize to 299 x 299
 * (align_corners=False), then (v - mean[c]) / std[c] with ImageNet's mean (0.485, 0.456, 0.406), std (0.229, 0.224, 0.225).
 * C must be 3 and 1 <= H, W <= 299. */
int dt_inception_preprocess(const float *images_dev, int B, int C, int H, int W, float in_scale, float in_shift,
                            float *out_dev, void *stream);

/* out [B][2048]: preprocessing and every module.  (in_scale, in_shift) = (0.5, 0.5) is InceptionModel.get_features'
 * (x + 1) / 2, (1, 0) compute_fid's input as given.  An image's features do not depend on B or on the other images. */
int dt_inception_features(const dt_inception *h, const float *images_dev, int B, int C, int H, int W, float in_scale,
                          float in_shift, float *out_dev, void *ws, size_t ws_bytes, void *stream);

/* Modules [first, last) on in_dev (the NHWC input of module `first`); out_dev receives the output of module last - 1.
 * 0 <= first < last <= DT_INCEPTION_N_MODULES; in_dev and out_dev 16-byte aligned and not inside the workspace. */
int dt_inception_run_modules(const dt_inception *h, int first, int last, const float *in_dev, int B, float *out_dev,
                             void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_INCEPTION_H */
