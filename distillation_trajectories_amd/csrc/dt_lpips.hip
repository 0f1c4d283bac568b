// LPIPS v0.1, net='alex' (include/dt_hip_lpips.h): AlexNet features up to the fifth ReLU and the perceptual distance.
//
// Activations are NHWC fp32.  Every conv is one launch of featnet_conv (dt_featnet.hip) with the bias as its shift and no
// scale; it reads its images through a per-image stride (the taps live inside the packs) and writes straight into the
// image's feature pack.  conv1 has cin 3 and K = 363 (the unaligned gather); conv2..5 walk the host's tap list, which on
// small pictures leaves out the taps that lie in the padding for every pixel of the launch.
// The distance (lp_distance) is one pass over both packs, one workgroup per pair, in the difference form, in fp64.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdint>

#include "../../include/dt_hip_lpips.h"
#include "dt_featnet.h"

namespace {

using namespace featnet;

constexpr int NT = 256;             // threads of a distance block: 4 waves
constexpr int NL = DT_LPIPS_N_LAYERS;

struct LayerDesc { int cin, cout, k, stride, pad, pool; };     // pool: a 3x3 s2 max pool in front of the conv
constexpr LayerDesc kLayers[NL] = {{3, 64, 11, 4, 2, 0}, {64, 192, 5, 1, 2, 1}, {192, 384, 3, 1, 1, 1},
                                   {384, 256, 3, 1, 1, 0}, {256, 256, 3, 1, 1, 0}};

__constant__ float kShift[3] = {-.030f, -.088f, -.188f};
__constant__ float kScale[3] = {.458f, .448f, .450f};

// images [N][3][H][W] -> [N][H][W][3]: the affine input map, then the scaling layer
__global__ void lp_scale(const float *x, int N, int HW, float in_scale, float in_shift, float *y) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= (size_t)N * HW) return;
  const size_t b = e / HW, p = e - b * HW;
  for (int c = 0; c < 3; ++c) {
    const float v = fmaf(in_scale, x[(b * 3 + c) * HW + p], in_shift);
    y[e * 3 + c] = (v - kShift[c]) / kScale[c];
  }
}

// ------------------------------------------------------------------------------------------------------ the distance
__device__ inline double wave_sum(double v) {      // xor butterfly: every lane ends with the same bits
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// sum over the pixels this wave takes (wave, wave + 4, ..) of sum_c w_c (a_c / (|a| + eps) - b_c / (|b| + eps))^2, C = 64 * CJ.
// No contraction: the two normalised values are each rounded before they are subtracted, so swapping a and b negates
// the difference exactly and equal inputs give exactly zero.
template <int CJ>
__device__ double layer_sum(const float *a, const float *b, const float *w, int npix, int lane, int wave) {
#pragma clang fp contract(off)
  double wl[CJ];
  for (int j = 0; j < CJ; ++j) wl[j] = (double)w[lane + 64 * j];
  double acc = 0.0;
  for (int p = wave; p < npix; p += NT / 64) {
    const float *pa = a + (size_t)p * (64 * CJ) + lane, *pb = b + (size_t)p * (64 * CJ) + lane;
    double fa[CJ], fb[CJ];
    double sa = 0.0, sb = 0.0;
    for (int j = 0; j < CJ; ++j) {
      fa[j] = (double)pa[64 * j];
      fb[j] = (double)pb[64 * j];
      sa += fa[j] * fa[j];
      sb += fb[j] * fb[j];
    }
    sa = wave_sum(sa);
    sb = wave_sum(sb);
    const double ra = 1.0 / (sqrt(sa) + 1e-10), rb = 1.0 / (sqrt(sb) + 1e-10);
    double s = 0.0;
    for (int j = 0; j < CJ; ++j) {
      const double na = fa[j] * ra, nb = fb[j] * rb;
      const double d = na - nb;
      s += (wl[j] * d) * d;
    }
    acc += wave_sum(s);
  }
  return acc;
}

struct DistArgs {
  const float *pack0, *pack1, *lin;      // lin: the five weight vectors one after another
  float *dist, *layers;                  // [G * n], NULL or [G * n][5]
  long long stride0, F;                  // floats between the images of pack0 (0: one shared image) and of pack1
  int n;
  int off[NL], npix[NL], loff[NL];       // float offset of tap l in a pack, its pixels, float offset of its weights in lin
};

// one workgroup per pair (g, i) = (block / n, block % n): pack0[i] against pack1[g][i]
__global__ __launch_bounds__(NT) void lp_distance(DistArgs a) {
  __shared__ double part[NT / 64][NL];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int i = blockIdx.x % a.n;
  const float *p0 = a.pack0 + (size_t)i * a.stride0, *p1 = a.pack1 + (size_t)blockIdx.x * a.F;
  const double s0 = layer_sum<1>(p0 + a.off[0], p1 + a.off[0], a.lin + a.loff[0], a.npix[0], lane, wave);
  const double s1 = layer_sum<3>(p0 + a.off[1], p1 + a.off[1], a.lin + a.loff[1], a.npix[1], lane, wave);
  const double s2 = layer_sum<6>(p0 + a.off[2], p1 + a.off[2], a.lin + a.loff[2], a.npix[2], lane, wave);
  const double s3 = layer_sum<4>(p0 + a.off[3], p1 + a.off[3], a.lin + a.loff[3], a.npix[3], lane, wave);
  const double s4 = layer_sum<4>(p0 + a.off[4], p1 + a.off[4], a.lin + a.loff[4], a.npix[4], lane, wave);
  if (lane == 0) part[wave][0] = s0, part[wave][1] = s1, part[wave][2] = s2, part[wave][3] = s3, part[wave][4] = s4;
  __syncthreads();
  if (threadIdx.x == 0) {
    double total = 0.0;
    for (int l = 0; l < NL; ++l) {
      double s = 0.0;
      for (int v = 0; v < NT / 64; ++v) s += part[v][l];
      s /= (double)a.npix[l];
      if (a.layers) a.layers[(size_t)blockIdx.x * NL + l] = (float)s;
      total += s;
    }
    a.dist[blockIdx.x] = (float)total;
  }
}

// ------------------------------------------------------------------------------------------------------- host side
bool size_ok(int H, int W) {
  return H >= DT_LPIPS_MIN_SIZE && H <= DT_LPIPS_MAX_SIZE && W >= DT_LPIPS_MIN_SIZE && W <= DT_LPIPS_MAX_SIZE;
}

// every size of the network for an H x W image
struct Shapes {
  int ih[NL], iw[NL];       // the conv's input (after the layer's pool)
  int ph[NL], pw[NL];       // the pool's input (= the tap before), where the layer has one
  int oh[NL], ow[NL];       // the tap
  size_t off[NL], F;        // float offset of tap l in a pack, floats of a pack
  Shapes(int H, int W) {
    int h = H, w = W;
    F = 0;
    for (int l = 0; l < NL; ++l) {
      const LayerDesc &d = kLayers[l];
      ph[l] = h, pw[l] = w;
      if (d.pool) h = out_size(h, 3, 2, 0), w = out_size(w, 3, 2, 0);
      ih[l] = h, iw[l] = w;
      h = out_size(h, d.k, d.stride, d.pad), w = out_size(w, d.k, d.stride, d.pad);
      oh[l] = h, ow[l] = w;
      off[l] = F;
      F += (size_t)h * w * d.cout;
    }
  }
  size_t tap_floats(int l) const { return (size_t)oh[l] * ow[l] * kLayers[l].cout; }
  size_t in_floats(int l) const { return l == 0 ? (size_t)ph[0] * pw[0] * 3 : tap_floats(l - 1); }
  size_t pool_floats(int l) const { return kLayers[l].pool ? (size_t)ih[l] * iw[l] * kLayers[l].cin : 0; }
  size_t max_tap() const {
    size_t m = 0;
    for (int l = 0; l < NL; ++l) m = tap_floats(l) > m ? tap_floats(l) : m;
    return m;
  }
};

// workspace, floats per image: the scaled image, the two pool outputs, two tap buffers for dt_lpips_run_layers
enum { WS_IMG, WS_POOL1, WS_POOL2, WS_TAP0, WS_TAP1, WS_N };
void ws_layout(const Shapes &s, size_t per_image[WS_N]) {
  per_image[WS_IMG] = round64(s.in_floats(0));
  per_image[WS_POOL1] = round64(s.pool_floats(1));
  per_image[WS_POOL2] = round64(s.pool_floats(2));
  per_image[WS_TAP0] = per_image[WS_TAP1] = round64(s.max_tap());
}

}  // namespace

struct dt_lpips {
  float *slab = nullptr;
  size_t w_off[NL], b_off[NL], lin_off[NL];
};

namespace {

int launch_conv(const dt_lpips *h, int l, const float *x, size_t xs, int N, int H, int W, float *y, size_t ys,
                hipStream_t s) {
  const LayerDesc &d = kLayers[l];
  ConvArgs a;
  a.x = x, a.w = h->slab + h->w_off[l], a.scale = nullptr, a.shift = h->slab + h->b_off[l], a.y = y;
  a.xs = (long long)xs, a.ys = (long long)ys;
  a.B = N, a.H = H, a.W = W, a.cin = d.cin, a.cout = d.cout, a.KH = a.KW = d.k, a.stride = d.stride, a.ph = a.pw = d.pad;
  a.ldy = d.cout, a.yoff = 0;
  return featnet_launch_conv(a, s);
}

// layers [first, last): layer l reads `in` (stride in_stride) when l == first, else tap l - 1, and writes tap[l] (stride ts[l])
int run(const dt_lpips *h, int first, int last, const float *in, size_t in_stride, int N, const Shapes &sh,
        float *const tap[NL], const size_t ts[NL], float *ws, hipStream_t s) {
  size_t per[WS_N];
  ws_layout(sh, per);
  float *pool[NL] = {nullptr, ws + per[WS_IMG] * (size_t)N, ws + (per[WS_IMG] + per[WS_POOL1]) * (size_t)N, nullptr, nullptr};
  for (int l = first; l < last; ++l) {
    const LayerDesc &d = kLayers[l];
    const float *x = l == first ? in : tap[l - 1];
    size_t xs = l == first ? in_stride : ts[l - 1];
    if (d.pool) {
      const int st = featnet_launch_maxpool(x, xs, N, sh.ph[l], sh.pw[l], d.cin, pool[l], d.cin, 0, s);
      if (st != DT_OK) return st;
      x = pool[l], xs = sh.pool_floats(l);
    }
    const int st = launch_conv(h, l, x, xs, N, sh.ih[l], sh.iw[l], tap[l], ts[l], s);
    if (st != DT_OK) return st;
  }
  return DT_OK;
}

size_t ws_bytes_for(int N, const Shapes &sh) {
  size_t per[WS_N], f = 0;
  ws_layout(sh, per);
  for (int i = 0; i < WS_N; ++i) f += per[i] * (size_t)N;
  return f * sizeof(float);
}

bool batch_ok(int N, const Shapes &sh) {       // M and every element index of a launch fit an int
  return N >= 1 && (size_t)N * sh.F <= (size_t)INT32_MAX && (size_t)N * round64(sh.in_floats(0)) <= (size_t)INT32_MAX;
}

int distance(const dt_lpips *h, const float *pack0, size_t stride0, const float *pack1, int n, int G, int H, int W,
             float *dist_out, float *layers_out, hipStream_t s) {
  const Shapes sh(H, W);
  DistArgs a;
  a.pack0 = pack0, a.pack1 = pack1, a.lin = h->slab + h->lin_off[0], a.dist = dist_out, a.layers = layers_out;
  a.stride0 = (long long)stride0, a.F = (long long)sh.F, a.n = n;
  for (int l = 0; l < NL; ++l) {
    a.off[l] = (int)sh.off[l], a.npix[l] = sh.oh[l] * sh.ow[l];
    a.loff[l] = (int)(h->lin_off[l] - h->lin_off[0]);
  }
  hipLaunchKernelGGL(lp_distance, dim3((unsigned)(n * G)), dim3(NT), 0, s, a);
  return hip_status(hipGetLastError());
}

}  // namespace

extern "C" {

int dt_lpips_layer_shape(int H, int W, int l, int *hwc) {
  if (!hwc) return DT_E_NULL;
  if (!size_ok(H, W)) return DT_E_SHAPE;
  if (l < 0 || l >= NL) return DT_E_ARG;
  const Shapes sh(H, W);
  hwc[0] = sh.oh[l], hwc[1] = sh.ow[l], hwc[2] = kLayers[l].cout;
  return DT_OK;
}

size_t dt_lpips_feature_floats(int H, int W) { return size_ok(H, W) ? Shapes(H, W).F : 0; }

int dt_lpips_create(const float *const *params, int n_params, void *stream, dt_lpips **out) {
  if (!params || !out) return DT_E_NULL;
  *out = nullptr;
  if (n_params != DT_LPIPS_N_PARAMS) return DT_E_ARG;
  for (int i = 0; i < n_params; ++i)
    if (!params[i]) return DT_E_NULL;
  dt_lpips *h = new dt_lpips;
  Slab slab;
  for (int l = 0; l < NL; ++l) {
    const LayerDesc &d = kLayers[l];
    h->w_off[l] = slab.take((size_t)d.cout * d.cin * d.k * d.k);
    h->b_off[l] = slab.take(d.cout);
  }
  for (int l = 0; l < NL; ++l) h->lin_off[l] = slab.take(kLayers[l].cout);
  hipError_t e = hipMalloc((void **)&h->slab, slab.floats * sizeof(float));
  if (e != hipSuccess) { delete h; return (int)e; }
  hipStream_t s = (hipStream_t)stream;
  for (int l = 0; l < NL && e == hipSuccess; ++l) {
    const LayerDesc &d = kLayers[l];
    featnet_launch_relayout(params[2 * l], d.cout, d.cin, d.k, d.k, h->slab + h->w_off[l], s);
    e = hipGetLastError();
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->slab + h->b_off[l], params[2 * l + 1], d.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
    if (e == hipSuccess)
      e = hipMemcpyAsync(h->slab + h->lin_off[l], params[2 * NL + l], d.cout * sizeof(float), hipMemcpyDeviceToDevice, s);
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) { (void)hipFree(h->slab); delete h; return (int)e; }
  *out = h;
  return DT_OK;
}

void dt_lpips_destroy(dt_lpips *h) {
  if (!h) return;
  if (h->slab) (void)hipFree(h->slab);
  delete h;
}

size_t dt_lpips_workspace_bytes(const dt_lpips *h, int N, int H, int W) {
  if (!h || N < 1 || !size_ok(H, W)) return 0;
  return ws_bytes_for(N, Shapes(H, W));
}

int dt_lpips_features(const dt_lpips *h, const float *images_dev, int N, int C, int H, int W, float in_scale,
                      float in_shift, float *pack_out, void *ws, size_t ws_bytes, void *stream) {
  if (!h || !images_dev || !pack_out || !ws) return DT_E_NULL;
  if (C != 3 || !size_ok(H, W)) return DT_E_SHAPE;
  const Shapes sh(H, W);
  if (!batch_ok(N, sh)) return DT_E_SHAPE;
  if (!aligned16(ws) || !aligned16(pack_out)) return DT_E_ARG;
  const size_t need = ws_bytes_for(N, sh), img_bytes = (size_t)N * 3 * H * W * 4, pack_bytes = (size_t)N * sh.F * 4;
  if (ws_bytes < need) return DT_E_WORKSPACE;
  if (overlap(images_dev, img_bytes, pack_out, pack_bytes) || overlap(images_dev, img_bytes, ws, need) ||
      overlap(pack_out, pack_bytes, ws, need))
    return DT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  float *img = (float *)ws;
  hipLaunchKernelGGL(lp_scale, dim3(blocks((size_t)N * H * W, 256)), dim3(256), 0, s, images_dev, N, H * W, in_scale,
                     in_shift, img);
  const int st = hip_status(hipGetLastError());
  if (st != DT_OK) return st;
  float *tap[NL];
  size_t ts[NL];
  for (int l = 0; l < NL; ++l) tap[l] = pack_out + sh.off[l], ts[l] = sh.F;
  return run(h, 0, NL, img, sh.in_floats(0), N, sh, tap, ts, (float *)ws, s);
}

int dt_lpips_run_layers(const dt_lpips *h, int first, int last, const float *in_dev, int N, int H, int W, float *out_dev,
                        void *ws, size_t ws_bytes, void *stream) {
  if (!h || !in_dev || !out_dev || !ws) return DT_E_NULL;
  if (first < 0 || last > NL || first >= last) return DT_E_ARG;
  if (!size_ok(H, W)) return DT_E_SHAPE;
  const Shapes sh(H, W);
  if (!batch_ok(N, sh)) return DT_E_SHAPE;
  if (!aligned16(in_dev) || !aligned16(out_dev) || !aligned16(ws)) return DT_E_ARG;
  const size_t need = ws_bytes_for(N, sh);
  if (ws_bytes < need) return DT_E_WORKSPACE;
  const size_t in_bytes = (size_t)N * sh.in_floats(first) * 4, out_bytes = (size_t)N * sh.tap_floats(last - 1) * 4;
  if (overlap(in_dev, in_bytes, ws, need) || overlap(out_dev, out_bytes, ws, need) ||
      overlap(in_dev, in_bytes, out_dev, out_bytes))
    return DT_E_ARG;
  size_t per[WS_N];
  ws_layout(sh, per);
  float *t0 = (float *)ws + (per[WS_IMG] + per[WS_POOL1] + per[WS_POOL2]) * (size_t)N;
  float *t1 = t0 + per[WS_TAP0] * (size_t)N;
  float *tap[NL];
  size_t ts[NL];
  for (int l = 0; l < NL; ++l) tap[l] = (l & 1) ? t1 : t0, ts[l] = sh.tap_floats(l);
  tap[last - 1] = out_dev;
  return run(h, first, last, in_dev, sh.in_floats(first), N, sh, tap, ts, (float *)ws, (hipStream_t)stream);
}

int dt_lpips_distance(const dt_lpips *h, const float *pack0, int n0, const float *pack1, int n1, int H, int W,
                      float *dist_out, float *layers_out, void *stream) {
  if (!h || !pack0 || !pack1 || !dist_out) return DT_E_NULL;
  if (!size_ok(H, W)) return DT_E_SHAPE;
  if (n1 < 1 || (n0 != 1 && n0 != n1)) return DT_E_ARG;
  if (!aligned16(pack0) || !aligned16(pack1)) return DT_E_ARG;
  const Shapes sh(H, W);
  const size_t b0 = (size_t)n0 * sh.F * 4, b1 = (size_t)n1 * sh.F * 4;
  if (overlap(dist_out, (size_t)n1 * 4, pack0, b0) || overlap(dist_out, (size_t)n1 * 4, pack1, b1)) return DT_E_ARG;
  if (layers_out && (overlap(layers_out, (size_t)n1 * NL * 4, pack0, b0) || overlap(layers_out, (size_t)n1 * NL * 4, pack1, b1) ||
                     overlap(layers_out, (size_t)n1 * NL * 4, dist_out, (size_t)n1 * 4)))
    return DT_E_ARG;
  return distance(h, pack0, n0 == 1 ? 0 : sh.F, pack1, n1, 1, H, W, dist_out, layers_out, (hipStream_t)stream);
}

int dt_lpips_distance_many(const dt_lpips *h, const float *pack0, const float *pack1, int n, int G, int H, int W,
                           float *dist_out, float *layers_out, void *stream) {
  if (!h || !pack0 || !pack1 || !dist_out) return DT_E_NULL;
  if (!size_ok(H, W)) return DT_E_SHAPE;
  if (n < 1 || G < 1 || (size_t)n * G > (size_t)INT32_MAX / NL) return DT_E_ARG;
  if (!aligned16(pack0) || !aligned16(pack1)) return DT_E_ARG;
  const Shapes sh(H, W);
  const size_t pairs = (size_t)n * G, b0 = (size_t)n * sh.F * 4, b1 = pairs * sh.F * 4;
  if (overlap(dist_out, pairs * 4, pack0, b0) || overlap(dist_out, pairs * 4, pack1, b1)) return DT_E_ARG;
  if (layers_out && (overlap(layers_out, pairs * NL * 4, pack0, b0) || overlap(layers_out, pairs * NL * 4, pack1, b1) ||
                     overlap(layers_out, pairs * NL * 4, dist_out, pairs * 4)))
    return DT_E_ARG;
  return distance(h, pack0, sh.F, pack1, n, G, H, W, dist_out, layers_out, (hipStream_t)stream);
}

}  // extern "C"
