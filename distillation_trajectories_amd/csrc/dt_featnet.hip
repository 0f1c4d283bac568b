// The convolution of the two fp32 feature networks (InceptionV3 of FID, AlexNet of LPIPS), their max pool and their weight
// relayout (dt_featnet.h).
//
// featnet_conv is an implicit GEMM on exact fp32 MFMA (v_mfma_f32_32x32x2_f32): M = B*OH*OW output pixels, N = cout,
// K = kh*kw*cin in (kh, kw, ci) order, so that with NHWC a 16-wide K chunk of an aligned layer is 16 contiguous input
// channels of one tap.  Images are addressed through a per-image stride and the output through a row pitch and a channel
// offset, so a launch writes straight into a channel slice of a concat buffer or into an image's feature pack.  The
// epilogue is a per-channel scale and shift (a folded BatchNorm, or no scale and a bias) and the ReLU.
// There is no split-K: every output element is one k-ordered fma chain whatever the batch, so an image's features do
// not depend on the other images in the launch.
// An aligned layer walks a tap list: the host lists the taps that touch the picture for at least one output pixel and
// the kernel walks only those; a skipped tap would have added fma(0, w, acc) to every chain.  On pictures no smaller
// than the kernel that is every tap; on LPIPS's small pictures most taps of conv2..5 lie in the padding for EVERY pixel
// of the launch (at 31..34-pixel inputs conv3..5 see a 1 x 1 picture: 8 of 9 taps).
#include "dt_featnet.h"

namespace featnet {
namespace {

constexpr int NT = 256;             // threads of a conv block: 4 waves, 2 x 2 of 32 x 32 output tiles
constexpr int BM = 64, BN = 64;     // block tile: output pixels x output channels
constexpr int KC = 16;              // K chunk staged in LDS per step (8 MFMA k-steps of 2)

typedef float f32x16 __attribute__((ext_vector_type(16)));

// ALIGNED: cin % KC == 0 (every chunk lies in one tap and is 16 contiguous channels), x and xs 16-byte aligned; walks a.taps.
template <bool ALIGNED>
__global__ __launch_bounds__(NT) void featnet_conv(ConvArgs a) {
  __shared__ float As[KC][BM];
  __shared__ float Bs[KC][BN];
  const int t = threadIdx.x, lane = t & 63;
  const int wave = __builtin_amdgcn_readfirstlane(t >> 6);      // uniform: the tile offsets it gives stay in SGPRs
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;

  // A staging role: output pixel am of the tile, K elements 4 * akq .. 4 * akq + 3 of the chunk
  const int am = t & (BM - 1), akq = t >> 6;
  const int m = m0 + am;
  const bool mvalid = m < a.M;
  int b = 0, oh = 0, ow = 0;
  if (mvalid) {
    b = m / a.P;
    const int pix = m - b * a.P;
    oh = pix / a.OW;
    ow = pix - oh * a.OW;
  }
  const int ih0 = oh * a.stride - a.ph, iw0 = ow * a.stride - a.pw;
  const float *xb = a.x + (size_t)b * a.xs;
  // B staging role: K row bk of the chunk, output channels 4 * (t & 15) .. + 3 (cout % 4 == 0)
  const int bk = t >> 4, bn = (t & 15) * 4;
  const bool nvalid = n0 + bn < a.cout;

  float4 ra, rb;
  unsigned taps = a.taps;                     // ALIGNED: the taps still to walk, lowest bit first
  int c0 = 0;                                 // ALIGNED: the first channel, within that tap, of the chunk load() fetches next
  auto load = [&](int k0) {
    ra = make_float4(0.f, 0.f, 0.f, 0.f);
    int wrow;                                 // row of a.w that K element k0 + bk is
    if (ALIGNED) {
      const int tap = __ffs(taps) - 1;
      const int kh = tap / a.KW, kw = tap - kh * a.KW;
      const int ih = ih0 + kh, iw = iw0 + kw;
      if (mvalid && ih >= 0 && ih < a.H && iw >= 0 && iw < a.W)
        ra = *reinterpret_cast<const float4 *>(xb + ((size_t)ih * a.W + iw) * a.cin + c0 + akq * 4);
      wrow = tap * a.cin + c0 + bk;
      c0 += KC;
      if (c0 == a.cin) c0 = 0, taps &= taps - 1;
    } else {
      float v[4];
      for (int j = 0; j < 4; ++j) {
        const int k = k0 + akq * 4 + j;
        v[j] = 0.f;
        if (mvalid && k < a.K) {
          const int tap = k / a.cin, ci = k - tap * a.cin;
          const int kh = tap / a.KW, kw = tap - kh * a.KW;
          const int ih = ih0 + kh, iw = iw0 + kw;
          if (ih >= 0 && ih < a.H && iw >= 0 && iw < a.W) v[j] = xb[((size_t)ih * a.W + iw) * a.cin + ci];
        }
      }
      ra = make_float4(v[0], v[1], v[2], v[3]);
      wrow = k0 + bk;
    }
    rb = (nvalid && k0 + bk < a.K) ? *reinterpret_cast<const float4 *>(a.w + (size_t)wrow * a.cout + n0 + bn)
                                  : make_float4(0.f, 0.f, 0.f, 0.f);
  };
  auto stage = [&]() {
    As[akq * 4 + 0][am] = ra.x;
    As[akq * 4 + 1][am] = ra.y;
    As[akq * 4 + 2][am] = ra.z;
    As[akq * 4 + 3][am] = ra.w;
    *reinterpret_cast<float4 *>(&Bs[bk][bn]) = rb;
  };

  const int wm = wave & 1, wn = wave >> 1;
  const int row = lane & 31, half = lane >> 5;
  f32x16 acc;
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;

  load(0);
  for (int k0 = 0; k0 < a.K; k0 += KC) {
    stage();
    __syncthreads();
    if (k0 + KC < a.K) load(k0 + KC);      // next chunk's global loads overlap this chunk's MFMAs
#pragma unroll
    for (int s = 0; s < KC / 2; ++s) {
      const float av = As[2 * s + half][wm * 32 + row];
      const float bv = Bs[2 * s + half][wn * 32 + row];
      acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av, bv, acc, 0, 0, 0);
    }
    __syncthreads();
  }

  // D map of the 32x32 MFMA: column (output channel) = lane & 31, row (pixel) = (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5)
  const int n = n0 + wn * 32 + row;
  if (n >= a.cout) return;
  const float sc = a.scale ? a.scale[n] : 1.f, sh = a.shift[n];      // fma(acc, 1, shift) is acc + shift, rounded once
  const int mb = m0 + wm * 32 + 4 * half;      // the lane's first row
  const int b0 = mb / a.P;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int mm = mb + (r & 3) + 8 * (r >> 2);
    if (mm < a.M) {
      int bb = b0, pix = mm - b0 * a.P;
      if (pix >= a.P) bb = mm / a.P, pix = mm - bb * a.P;      // a row of a later image: divide again
      a.y[(size_t)bb * a.ys + (size_t)pix * a.ldy + a.yoff + n] = fmaxf(fmaf(acc[r], sc, sh), 0.f);
    }
  }
}

// four channels per thread
__global__ void featnet_maxpool(const float *x, long long xs, int N, int H, int W, int C, int OH, int OW, float *y, int ldy,
                                int yoff) {
  const size_t e = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int C4 = C / 4;
  if (e >= (size_t)N * OH * OW * C4) return;
  const int c = (int)(e % C4) * 4;
  const size_t pix = e / C4;
  const int ow = (int)(pix % OW), oh = (int)(pix / OW % OH), b = (int)(pix / OW / OH);
  const float *xb = x + (size_t)b * xs + c;
  float4 v = *reinterpret_cast<const float4 *>(xb + ((size_t)(2 * oh) * W + 2 * ow) * C);
  for (int i = 0; i < 3; ++i)
    for (int j = 0; j < 3; ++j) {
      const float4 u = *reinterpret_cast<const float4 *>(xb + ((size_t)(2 * oh + i) * W + 2 * ow + j) * C);
      v.x = fmaxf(v.x, u.x), v.y = fmaxf(v.y, u.y), v.z = fmaxf(v.z, u.z), v.w = fmaxf(v.w, u.w);
    }
  *reinterpret_cast<float4 *>(y + pix * ldy + yoff + c) = v;
}

__global__ void featnet_relayout(const float *src, int cout, int cin, int KH, int KW, float *dst) {
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= cout * cin * KH * KW) return;
  const int kw = e % KW, kh = e / KW % KH, ci = e / (KW * KH) % cin, co = e / (KW * KH * cin);
  dst[((size_t)(kh * KW + kw) * cin + ci) * cout + co] = src[e];
}

// the taps (bit kh * KW + kw) of which at least one output pixel's input lies inside the picture
unsigned tap_list(const ConvArgs &a, int OH) {
  unsigned taps = 0;
  for (int kh = 0; kh < a.KH; ++kh) {
    bool vh = false;
    for (int o = 0; o < OH && !vh; ++o) vh = o * a.stride - a.ph + kh >= 0 && o * a.stride - a.ph + kh < a.H;
    if (!vh) continue;
    for (int kw = 0; kw < a.KW; ++kw) {
      bool vw = false;
      for (int o = 0; o < a.OW && !vw; ++o) vw = o * a.stride - a.pw + kw >= 0 && o * a.stride - a.pw + kw < a.W;
      if (vw) taps |= 1u << (kh * a.KW + kw);
    }
  }
  return taps;
}

}  // namespace

int featnet_launch_conv(ConvArgs a, hipStream_t s) {
  const int OH = out_size(a.H, a.KH, a.stride, a.ph);
  a.OW = out_size(a.W, a.KW, a.stride, a.pw);
  a.P = OH * a.OW, a.M = a.B * a.P;
  const bool aligned = a.cin % KC == 0 && a.KH * a.KW <= MAX_TAPS && aligned16(a.x) && a.xs % 4 == 0;
  a.taps = aligned ? tap_list(a, OH) : 0;
  a.K = aligned ? __builtin_popcount(a.taps) * a.cin : a.KH * a.KW * a.cin;
  const dim3 grid((a.M + BM - 1) / BM, (a.cout + BN - 1) / BN);
  if (aligned)
    hipLaunchKernelGGL(featnet_conv<true>, grid, dim3(NT), 0, s, a);
  else
    hipLaunchKernelGGL(featnet_conv<false>, grid, dim3(NT), 0, s, a);
  return hip_status(hipGetLastError());
}

int featnet_launch_maxpool(const float *x, size_t xs, int N, int H, int W, int C, float *y, int ldy, int yoff, hipStream_t s) {
  const int OH = out_size(H, 3, 2, 0), OW = out_size(W, 3, 2, 0);
  hipLaunchKernelGGL(featnet_maxpool, dim3(blocks((size_t)N * OH * OW * (C / 4), 256)), dim3(256), 0, s, x, (long long)xs, N, H,
                     W, C, OH, OW, y, ldy, yoff);
  return hip_status(hipGetLastError());
}

void featnet_launch_relayout(const float *src, int cout, int cin, int KH, int KW, float *dst, hipStream_t s) {
  hipLaunchKernelGGL(featnet_relayout, dim3(blocks((size_t)cout * cin * KH * KW, 256)), dim3(256), 0, s, src, cout, cin, KH, KW,
                     dst);
}

}  // namespace featnet
