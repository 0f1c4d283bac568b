// InceptionV3 feature extractor of the FID stage (include/dt_hip_inception.h): torchvision's Inception3 in eval mode,
// transform_input=False, fc = Identity -- the 2048 avgpool values per image.
//
// Activations are NHWC fp32 between modules.  Every BasicConv2d (conv without bias + BatchNorm + ReLU) is one launch of
// featnet_conv (dt_featnet.hip), whose epilogue applies the BatchNorm folded at create time and the ReLU and writes into a
// channel slice of the module's concat buffer, so concatenation costs no copy.  Every conv runs on a picture no smaller
// than its kernel, so an aligned layer's tap list is the full list.  Pools are separate small kernels.
#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#include "../../include/dt_hip_inception.h"
#include "dt_featnet.h"

namespace {

using namespace featnet;

// avg pool 3x3 stride 1 padding 1, count_include_pad: every window divides by 9.  x, y [B][H][W][C]
__global__ void inc_avgpool(const float *x, int B, int H, int W, int C, float *y) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)B * H * W * C) return;
  const int c = (int)(e % C);
  const size_t pix = e / C;
  const int w = (int)(pix % W), h = (int)(pix / W % H), b = (int)(pix / W / H);
  const float *xb = x + ((size_t)b * H * W) * C + c;
  float s = 0.f;
  for (int i = h - 1; i <= h + 1; ++i)
    for (int j = w - 1; j <= w + 1; ++j)
      if (i >= 0 && i < H && j >= 0 && j < W) s += xb[((size_t)i * W + j) * C];
  y[e] = s / 9.f;
}

// adaptive avg pool to 1 x 1: x [B][HW][C] -> y [B][C]
__global__ void inc_mean(const float *x, int B, int HW, int C, float *y) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * C) return;
  const int c = e % C, b = e / C;
  const float *xb = x + (size_t)b * HW * C + c;
  float s = 0.f;
  for (int i = 0; i < HW; ++i) s += xb[(size_t)i * C];
  y[e] = s / (float)HW;
}

__constant__ float kMean[3] = {0.485f, 0.456f, 0.406f};
__constant__ float kStd[3] = {0.229f, 0.224f, 0.225f};

// images [B][3][H][W] -> [B][299][299][3]: affine map, half-pixel bilinear upsample (align_corners=False), normalise
__global__ void inc_preprocess(const float *x, int B, int H, int W, float in_scale, float in_shift, float *y) {
  const int S = DT_INCEPTION_SIZE;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= B * S * S) return;
  const int ox = e % S, oy = e / S % S, b = e / (S * S);
  // half-pixel source coordinate max(H / S * (o + 0.5) - 0.5, 0) = max(H * (2o + 1) - S, 0) / 2S, split exactly in
  // integers: the interpolation weight is rounded once (a float32 coordinate would be off by up to ulp(H))
  const int ny = max(H * (2 * oy + 1) - S, 0), nx = max(W * (2 * ox + 1) - S, 0);
  const int y0 = ny / (2 * S), x0 = nx / (2 * S);
  const int y1 = y0 + (y0 < H - 1), x1 = x0 + (x0 < W - 1);
  const float ly = (float)(ny - y0 * 2 * S) / (float)(2 * S), lx = (float)(nx - x0 * 2 * S) / (float)(2 * S);
  for (int c = 0; c < 3; ++c) {
    const float *p = x + ((size_t)b * 3 + c) * H * W;
    const float v00 = in_scale * p[y0 * W + x0] + in_shift, v01 = in_scale * p[y0 * W + x1] + in_shift;
    const float v10 = in_scale * p[y1 * W + x0] + in_shift, v11 = in_scale * p[y1 * W + x1] + in_shift;
    const float v = (1.f - ly) * ((1.f - lx) * v00 + lx * v01) + ly * ((1.f - lx) * v10 + lx * v11);
    y[(size_t)e * 3 + c] = (v - kMean[c]) / kStd[c];
  }
}

// BatchNorm (eps 1e-3, running statistics) as a per-channel scale and shift, in float64
__global__ void inc_fold_bn(const float *g, const float *bta, const float *mean, const float *var, int n, float *scale,
                            float *shift) {
  const int c = blockIdx.x * blockDim.x + threadIdx.x;
  if (c >= n) return;
  const double s = (double)g[c] / sqrt((double)var[c] + 1e-3);
  scale[c] = (float)s;
  shift[c] = (float)((double)bta[c] - (double)mean[c] * s);
}

// ------------------------------------------------------------------------------------------------ the network table
struct ConvDesc { int cin, cout, kh, kw, stride, ph, pw; };

enum { OP_CONV, OP_MAXPOOL, OP_AVGPOOL, OP_MEAN };
enum { BUF_IN, BUF_OUT, BUF_T0, BUF_T1, BUF_T2, N_BUF };     // T0..T2: a module's branch intermediates

struct Op { int kind, conv, src, dst, H, W, C, yoff; };       // H, W, C: the op's input

struct Module { int H, W, C, OH, OW, OC, op_begin, op_end; };

struct Net {
  std::vector<ConvDesc> convs;
  std::vector<Op> ops;
  std::vector<Module> mods;
  size_t scratch[N_BUF] = {0, 0, 0, 0, 0};    // floats per image of BUF_IN/OUT (ping-pong) and T0..T2

  int conv(int cin, int cout, int kh, int kw, int stride = 1, int ph = 0, int pw = 0) {
    convs.push_back({cin, cout, kh, kw, stride, ph, pw});
    return (int)convs.size() - 1;
  }
  void need(int buf, size_t floats) { scratch[buf] = floats > scratch[buf] ? floats : scratch[buf]; }
  // one BasicConv2d from buffer src (H x W x cin) to dst, channel offset yoff; returns the output size
  void op_conv(int ci, int src, int dst, int H, int W, int yoff = 0) {
    const ConvDesc &d = convs[ci];
    ops.push_back({OP_CONV, ci, src, dst, H, W, d.cin, yoff});
    if (dst != BUF_OUT) need(dst, (size_t)out_size(H, d.kh, d.stride, d.ph) * out_size(W, d.kw, d.stride, d.pw) * d.cout);
  }
  void begin(int H, int W, int C) { mods.push_back({H, W, C, 0, 0, 0, (int)ops.size(), 0}); }
  void end(int OH, int OW, int OC) {
    Module &m = mods.back();
    m.OH = OH, m.OW = OW, m.OC = OC, m.op_end = (int)ops.size();
    need(BUF_IN, (size_t)m.H * m.W * m.C);
    need(BUF_OUT, (size_t)OH * OW * OC);
  }
  void basic(int H, int W, int cin, int cout, int k, int stride, int pad) {
    begin(H, W, cin);
    op_conv(conv(cin, cout, k, k, stride, pad, pad), BUF_IN, BUF_OUT, H, W);
    end(out_size(H, k, stride, pad), out_size(W, k, stride, pad), cout);
  }
  void maxpool(int H, int W, int C) {
    begin(H, W, C);
    ops.push_back({OP_MAXPOOL, -1, BUF_IN, BUF_OUT, H, W, C, 0});
    end(out_size(H, 3, 2, 0), out_size(W, 3, 2, 0), C);
  }
  void avgpool_then_1x1(int H, int W, int cin, int cout, int yoff) {
    ops.push_back({OP_AVGPOOL, -1, BUF_IN, BUF_T2, H, W, cin, 0});
    need(BUF_T2, (size_t)H * W * cin);
    op_conv(conv(cin, cout, 1, 1), BUF_T2, BUF_OUT, H, W, yoff);
  }
  void inception_a(int S, int cin, int pool_features) {
    begin(S, S, cin);
    op_conv(conv(cin, 64, 1, 1), BUF_IN, BUF_OUT, S, S, 0);                      // branch1x1
    op_conv(conv(cin, 48, 1, 1), BUF_IN, BUF_T0, S, S);                          // branch5x5_1
    op_conv(conv(48, 64, 5, 5, 1, 2, 2), BUF_T0, BUF_OUT, S, S, 64);             // branch5x5_2
    op_conv(conv(cin, 64, 1, 1), BUF_IN, BUF_T0, S, S);                          // branch3x3dbl_1
    op_conv(conv(64, 96, 3, 3, 1, 1, 1), BUF_T0, BUF_T1, S, S);                  // branch3x3dbl_2
    op_conv(conv(96, 96, 3, 3, 1, 1, 1), BUF_T1, BUF_OUT, S, S, 128);            // branch3x3dbl_3
    avgpool_then_1x1(S, S, cin, pool_features, 224);                             // branch_pool
    end(S, S, 224 + pool_features);
  }
  void inception_b(int S, int cin) {
    const int O = out_size(S, 3, 2, 0);
    begin(S, S, cin);
    op_conv(conv(cin, 384, 3, 3, 2), BUF_IN, BUF_OUT, S, S, 0);                  // branch3x3
    op_conv(conv(cin, 64, 1, 1), BUF_IN, BUF_T0, S, S);                          // branch3x3dbl_1
    op_conv(conv(64, 96, 3, 3, 1, 1, 1), BUF_T0, BUF_T1, S, S);                  // branch3x3dbl_2
    op_conv(conv(96, 96, 3, 3, 2), BUF_T1, BUF_OUT, S, S, 384);                  // branch3x3dbl_3
    ops.push_back({OP_MAXPOOL, -1, BUF_IN, BUF_OUT, S, S, cin, 480});
    end(O, O, 480 + cin);
  }
  void inception_c(int S, int c7) {
    begin(S, S, 768);
    op_conv(conv(768, 192, 1, 1), BUF_IN, BUF_OUT, S, S, 0);                     // branch1x1
    op_conv(conv(768, c7, 1, 1), BUF_IN, BUF_T0, S, S);                          // branch7x7_1
    op_conv(conv(c7, c7, 1, 7, 1, 0, 3), BUF_T0, BUF_T1, S, S);                  // branch7x7_2
    op_conv(conv(c7, 192, 7, 1, 1, 3, 0), BUF_T1, BUF_OUT, S, S, 192);           // branch7x7_3
    op_conv(conv(768, c7, 1, 1), BUF_IN, BUF_T0, S, S);                          // branch7x7dbl_1
    op_conv(conv(c7, c7, 7, 1, 1, 3, 0), BUF_T0, BUF_T1, S, S);                  // branch7x7dbl_2
    op_conv(conv(c7, c7, 1, 7, 1, 0, 3), BUF_T1, BUF_T0, S, S);                  // branch7x7dbl_3
    op_conv(conv(c7, c7, 7, 1, 1, 3, 0), BUF_T0, BUF_T1, S, S);                  // branch7x7dbl_4
    op_conv(conv(c7, 192, 1, 7, 1, 0, 3), BUF_T1, BUF_OUT, S, S, 384);           // branch7x7dbl_5
    avgpool_then_1x1(S, S, 768, 192, 576);                                       // branch_pool
    end(S, S, 768);
  }
  void inception_d(int S, int cin) {
    const int O = out_size(S, 3, 2, 0);
    begin(S, S, cin);
    op_conv(conv(cin, 192, 1, 1), BUF_IN, BUF_T0, S, S);                         // branch3x3_1
    op_conv(conv(192, 320, 3, 3, 2), BUF_T0, BUF_OUT, S, S, 0);                  // branch3x3_2
    op_conv(conv(cin, 192, 1, 1), BUF_IN, BUF_T0, S, S);                         // branch7x7x3_1
    op_conv(conv(192, 192, 1, 7, 1, 0, 3), BUF_T0, BUF_T1, S, S);                // branch7x7x3_2
    op_conv(conv(192, 192, 7, 1, 1, 3, 0), BUF_T1, BUF_T0, S, S);                // branch7x7x3_3
    op_conv(conv(192, 192, 3, 3, 2), BUF_T0, BUF_OUT, S, S, 320);                // branch7x7x3_4
    ops.push_back({OP_MAXPOOL, -1, BUF_IN, BUF_OUT, S, S, cin, 512});
    end(O, O, 512 + cin);
  }
  void inception_e(int S, int cin) {
    begin(S, S, cin);
    op_conv(conv(cin, 320, 1, 1), BUF_IN, BUF_OUT, S, S, 0);                     // branch1x1
    op_conv(conv(cin, 384, 1, 1), BUF_IN, BUF_T0, S, S);                         // branch3x3_1
    op_conv(conv(384, 384, 1, 3, 1, 0, 1), BUF_T0, BUF_OUT, S, S, 320);          // branch3x3_2a
    op_conv(conv(384, 384, 3, 1, 1, 1, 0), BUF_T0, BUF_OUT, S, S, 704);          // branch3x3_2b
    op_conv(conv(cin, 448, 1, 1), BUF_IN, BUF_T0, S, S);                         // branch3x3dbl_1
    op_conv(conv(448, 384, 3, 3, 1, 1, 1), BUF_T0, BUF_T1, S, S);                // branch3x3dbl_2
    op_conv(conv(384, 384, 1, 3, 1, 0, 1), BUF_T1, BUF_OUT, S, S, 1088);         // branch3x3dbl_3a
    op_conv(conv(384, 384, 3, 1, 1, 1, 0), BUF_T1, BUF_OUT, S, S, 1472);         // branch3x3dbl_3b
    avgpool_then_1x1(S, S, cin, 192, 1856);                                      // branch_pool
    end(S, S, 2048);
  }

  Net() {
    const int S = DT_INCEPTION_SIZE;
    basic(S, S, 3, 32, 3, 2, 0);        // Conv2d_1a_3x3  299 -> 149
    basic(149, 149, 32, 32, 3, 1, 0);   // Conv2d_2a_3x3  -> 147
    basic(147, 147, 32, 64, 3, 1, 1);   // Conv2d_2b_3x3
    maxpool(147, 147, 64);              // -> 73
    basic(73, 73, 64, 80, 1, 1, 0);     // Conv2d_3b_1x1
    basic(73, 73, 80, 192, 3, 1, 0);    // Conv2d_4a_3x3  -> 71
    maxpool(71, 71, 192);               // -> 35
    inception_a(35, 192, 32);           // Mixed_5b
    inception_a(35, 256, 64);           // Mixed_5c
    inception_a(35, 288, 64);           // Mixed_5d
    inception_b(35, 288);               // Mixed_6a -> 17
    inception_c(17, 128);               // Mixed_6b
    inception_c(17, 160);               // Mixed_6c
    inception_c(17, 160);               // Mixed_6d
    inception_c(17, 192);               // Mixed_6e
    inception_d(17, 768);               // Mixed_7a -> 8
    inception_e(8, 1280);               // Mixed_7b
    inception_e(8, 2048);               // Mixed_7c
    begin(8, 8, 2048);                  // avgpool
    ops.push_back({OP_MEAN, -1, BUF_IN, BUF_OUT, 8, 8, 2048, 0});
    end(1, 1, 2048);
    for (int b = 0; b < N_BUF; ++b) scratch[b] = round64(scratch[b]);
    scratch[BUF_IN] = scratch[BUF_OUT] = scratch[BUF_IN] > scratch[BUF_OUT] ? scratch[BUF_IN] : scratch[BUF_OUT];
  }
};

const Net &net() {
  static const Net n;
  return n;
}

size_t ws_floats(int B) {
  const Net &n = net();
  size_t f = 0;
  for (int b = 0; b < N_BUF; ++b) f += n.scratch[b] * (size_t)B;
  return f;
}

}  // namespace

struct dt_inception {
  float *slab = nullptr;
  size_t w_off[DT_INCEPTION_N_CONVS], s_off[DT_INCEPTION_N_CONVS], t_off[DT_INCEPTION_N_CONVS];
};

namespace {

int launch_conv(const dt_inception *h, int ci, const float *x, int B, int H, int W, float *y, int ldy, int yoff,
                hipStream_t s) {
  const ConvDesc &d = net().convs[ci];
  ConvArgs a;
  a.x = x, a.w = h->slab + h->w_off[ci], a.scale = h->slab + h->s_off[ci], a.shift = h->slab + h->t_off[ci], a.y = y;
  a.B = B, a.H = H, a.W = W, a.cin = d.cin, a.cout = d.cout, a.KH = d.kh, a.KW = d.kw, a.stride = d.stride, a.ph = d.ph, a.pw = d.pw;
  a.ldy = ldy, a.yoff = yoff, a.xs = (long long)H * W * d.cin;
  a.ys = (long long)out_size(H, d.kh, d.stride, d.ph) * out_size(W, d.kw, d.stride, d.pw) * ldy;
  return featnet_launch_conv(a, s);
}

int run(const dt_inception *h, int first, int last, const float *in, int B, float *out, float *ws, hipStream_t s) {
  const Net &n = net();
  float *ping[2] = {ws, ws + n.scratch[BUF_IN] * (size_t)B};
  float *tmp[3];
  tmp[0] = ping[1] + n.scratch[BUF_OUT] * (size_t)B;
  tmp[1] = tmp[0] + n.scratch[BUF_T0] * (size_t)B;
  tmp[2] = tmp[1] + n.scratch[BUF_T1] * (size_t)B;
  const float *cur = in;
  for (int mi = first; mi < last; ++mi) {
    const Module &m = n.mods[mi];
    float *dst = mi == last - 1 ? out : (cur == ping[0] ? ping[1] : ping[0]);
    for (int oi = m.op_begin; oi < m.op_end; ++oi) {
      const Op &o = n.ops[oi];
      const float *src = o.src == BUF_IN ? cur : tmp[o.src - BUF_T0];
      float *y = o.dst == BUF_OUT ? dst : tmp[o.dst - BUF_T0];
      int st = DT_OK;
      if (o.kind == OP_CONV) {
        const int ldy = o.dst == BUF_OUT ? m.OC : n.convs[o.conv].cout;
        st = launch_conv(h, o.conv, src, B, o.H, o.W, y, ldy, o.yoff, s);
      } else if (o.kind == OP_MAXPOOL) {
        st = featnet_launch_maxpool(src, (size_t)o.H * o.W * o.C, B, o.H, o.W, o.C, y, m.OC, o.yoff, s);
      } else if (o.kind == OP_AVGPOOL) {
        hipLaunchKernelGGL(inc_avgpool, dim3(blocks((size_t)B * o.H * o.W * o.C, 256)), dim3(256), 0, s, src, B, o.H,
                           o.W, o.C, y);
        st = hip_status(hipGetLastError());
      } else {
        hipLaunchKernelGGL(inc_mean, dim3(blocks((size_t)B * o.C, 256)), dim3(256), 0, s, src, B, o.H * o.W, o.C, y);
        st = hip_status(hipGetLastError());
      }
      if (st != DT_OK) return st;
    }
    cur = dst;
  }
  return DT_OK;
}

bool image_shape_ok(int B, int C, int H, int W) {
  return B >= 1 && C == 3 && H >= 1 && W >= 1 && H <= DT_INCEPTION_SIZE && W <= DT_INCEPTION_SIZE &&
         (size_t)B * DT_INCEPTION_SIZE * DT_INCEPTION_SIZE <= (size_t)INT32_MAX && (size_t)B * H * W * C <= (size_t)INT32_MAX;
}

}  // namespace

extern "C" {

int dt_inception_conv_desc(int i, int *desc7) {
  if (!desc7) return DT_E_NULL;
  if (i < 0 || i >= DT_INCEPTION_N_CONVS) return DT_E_ARG;
  const ConvDesc &d = net().convs[i];
  const int v[7] = {d.cin, d.cout, d.kh, d.kw, d.stride, d.ph, d.pw};
  for (int j = 0; j < 7; ++j) desc7[j] = v[j];
  return DT_OK;
}

int dt_inception_module_shape(int m, int *in_hwc, int *out_hwc) {
  if (!in_hwc || !out_hwc) return DT_E_NULL;
  if (m < 0 || m >= DT_INCEPTION_N_MODULES) return DT_E_ARG;
  const Module &d = net().mods[m];
  in_hwc[0] = d.H, in_hwc[1] = d.W, in_hwc[2] = d.C;
  out_hwc[0] = d.OH, out_hwc[1] = d.OW, out_hwc[2] = d.OC;
  return DT_OK;
}

int dt_inception_create(const float *const *params, int n_params, void *stream, dt_inception **out) {
  if (!params || !out) return DT_E_NULL;
  *out = nullptr;
  if (n_params != 5 * DT_INCEPTION_N_CONVS) return DT_E_ARG;
  for (int i = 0; i < n_params; ++i)
    if (!params[i]) return DT_E_NULL;
  const Net &n = net();
  if ((int)n.convs.size() != DT_INCEPTION_N_CONVS || (int)n.mods.size() != DT_INCEPTION_N_MODULES) return DT_E_ARG;
  dt_inception *h = new dt_inception;
  Slab slab;
  for (int i = 0; i < DT_INCEPTION_N_CONVS; ++i) {
    const ConvDesc &d = n.convs[i];
    h->w_off[i] = slab.take((size_t)d.cout * d.cin * d.kh * d.kw);
    h->s_off[i] = slab.take(d.cout);
    h->t_off[i] = slab.take(d.cout);
  }
  hipError_t e = hipMalloc((void **)&h->slab, slab.floats * sizeof(float));
  if (e != hipSuccess) { delete h; return (int)e; }
  hipStream_t s = (hipStream_t)stream;
  for (int i = 0; i < DT_INCEPTION_N_CONVS && e == hipSuccess; ++i) {
    const ConvDesc &d = n.convs[i];
    const float *const *p = params + 5 * i;
    featnet_launch_relayout(p[0], d.cout, d.cin, d.kh, d.kw, h->slab + h->w_off[i], s);
    hipLaunchKernelGGL(inc_fold_bn, dim3(blocks(d.cout, 256)), dim3(256), 0, s, p[1], p[2], p[3], p[4], d.cout,
                       h->slab + h->s_off[i], h->slab + h->t_off[i]);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { (void)hipFree(h->slab); delete h; return (int)e; }
  *out = h;
  return DT_OK;
}

void dt_inception_destroy(dt_inception *h) {
  if (!h) return;
  if (h->slab) (void)hipFree(h->slab);
  delete h;
}

size_t dt_inception_workspace_bytes(const dt_inception *h, int B) {
  if (!h || B < 1) return 0;
  return ws_floats(B) * sizeof(float);
}

int dt_inception_preprocess(const float *images_dev, int B, int C, int H, int W, float in_scale, float in_shift,
                            float *out_dev, void *stream) {
  if (!images_dev || !out_dev) return DT_E_NULL;
  if (!image_shape_ok(B, C, H, W)) return DT_E_SHAPE;
  const size_t n = (size_t)B * DT_INCEPTION_SIZE * DT_INCEPTION_SIZE;
  hipLaunchKernelGGL(inc_preprocess, dim3(blocks(n, 256)), dim3(256), 0, (hipStream_t)stream, images_dev, B, H, W,
                     in_scale, in_shift, out_dev);
  return hip_status(hipGetLastError());
}

int dt_inception_features(const dt_inception *h, const float *images_dev, int B, int C, int H, int W, float in_scale,
                          float in_shift, float *out_dev, void *ws, size_t ws_bytes, void *stream) {
  if (!h || !images_dev || !out_dev || !ws) return DT_E_NULL;
  if (!image_shape_ok(B, C, H, W)) return DT_E_SHAPE;
  if (!aligned16(ws) || !aligned16(out_dev)) return DT_E_ARG;
  if (ws_bytes < dt_inception_workspace_bytes(h, B)) return DT_E_WORKSPACE;
  float *img = (float *)ws;      // the preprocessed image sits in the first ping-pong buffer; module 0 writes the second
  const int st = dt_inception_preprocess(images_dev, B, C, H, W, in_scale, in_shift, img, stream);
  if (st != DT_OK) return st;
  return run(h, 0, DT_INCEPTION_N_MODULES, img, B, out_dev, (float *)ws, (hipStream_t)stream);
}

int dt_inception_run_modules(const dt_inception *h, int first, int last, const float *in_dev, int B, float *out_dev,
                             void *ws, size_t ws_bytes, void *stream) {
  if (!h || !in_dev || !out_dev || !ws) return DT_E_NULL;
  if (first < 0 || last > DT_INCEPTION_N_MODULES || first >= last) return DT_E_ARG;
  if (B < 1 || (size_t)B * net().scratch[BUF_IN] > (size_t)INT32_MAX) return DT_E_SHAPE;
  if (!aligned16(in_dev) || !aligned16(out_dev) || !aligned16(ws)) return DT_E_ARG;
  if (ws_bytes < dt_inception_workspace_bytes(h, B)) return DT_E_WORKSPACE;
  return run(h, first, last, in_dev, B, out_dev, (float *)ws, (hipStream_t)stream);
}

}  // extern "C"
