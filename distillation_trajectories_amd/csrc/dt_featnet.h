// What the two fp32 feature networks (dt_inception.hip, dt_lpips.hip) share: the convolution, the 3x3 stride-2 max pool,
// the weight relayout (dt_featnet.hip) and the small host helpers.  Internal: nothing of it is in include/.
#pragma once

#include <hip/hip_runtime.h>

#include <cstddef>
#include <cstdint>

#include "../../include/dt_hip.h"

namespace featnet {

constexpr int MAX_TAPS = 25;        // tap lists are kept for kernels of up to 25 taps (5 x 5); they are bits of one word

// One convolution launch.  The caller fills everything down to yoff; featnet_launch_conv fills the rest.
struct ConvArgs {
  const float *x;       // image b at x + b * xs: [H][W][cin]
  const float *w;       // [(kh, kw, ci)][cout]
  const float *scale;   // y = relu(fma(conv, scale[n], shift[n])): a folded BatchNorm, or NULL (scale 1) and the bias
  const float *shift;
  float *y;             // (image b, pixel p, channel n) at y + b * ys + p * ldy + yoff + n
  long long xs, ys;
  int B, H, W, cin, cout, KH, KW, stride, ph, pw, ldy, yoff;
  int M, P, OW;         // B * P output pixels, P = OH * OW per image
  int K;                // walked K: ntaps * cin with a tap list (aligned), KH * KW * cin without
  unsigned taps;        // bit kh * KW + kw: a walked tap; walked in ascending order
};

int featnet_launch_conv(ConvArgs a, hipStream_t s);
// max pool 3x3 stride 2, no padding (C % 4 == 0): image b at x + b * xs [H][W][C] -> y [N][OH][OW][ldy], channels [yoff, yoff + C)
int featnet_launch_maxpool(const float *x, size_t xs, int N, int H, int W, int C, float *y, int ldy, int yoff, hipStream_t s);
// [cout][cin][kh][kw] -> [(kh, kw, ci)][cout]; the caller reads hipGetLastError
void featnet_launch_relayout(const float *src, int cout, int cin, int KH, int KW, float *dst, hipStream_t s);

inline int hip_status(hipError_t e) { return e == hipSuccess ? DT_OK : (int)e; }
inline bool aligned16(const void *p) { return ((uintptr_t)p & 15) == 0; }
inline unsigned blocks(size_t n, int t) { return (unsigned)((n + t - 1) / t); }
inline int out_size(int n, int k, int s, int p) { return (n + 2 * p - k) / s + 1; }
inline size_t round64(size_t f) { return (f + 63) / 64 * 64; }     // 256-byte aligned slices
inline bool overlap(const void *p, size_t pb, const void *q, size_t qb) {
  const uintptr_t a = (uintptr_t)p, b = (uintptr_t)q;
  return a < b + qb && b < a + pb;
}

// float offsets into one device allocation, each slice rounded up to 64 floats
struct Slab {
  size_t floats = 0;
  size_t take(size_t n) {
    const size_t o = floats;
    floats += round64(n);
    return o;
  }
};

}  // namespace featnet
