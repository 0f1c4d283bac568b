// Implicit-GEMM convolution with fp32-accurate arithmetic on the bf16 matrix cores ("split-bf16").
//
// gfx950 has no reduced-precision fast path for fp32 inputs (no xf32/TF32); its exact fp32 MFMA runs at
// 1/16 of the bf16 rate.  This kernel keeps fp32 ACCURACY while using v_mfma_f32_32x32x16_bf16:
// every fp32 operand is split EXACTLY into three bf16 planes
//      a = a1 + a2 + a3,   a1 = bf16(a), a2 = bf16(a - a1), a3 = bf16(a - a1 - a2)
// (round-to-nearest at each step; the residuals are exact in fp32 and the third one fits in 8 bits, so
// the three planes carry all 24 significand bits), and a*b is evaluated as the six plane products whose
// magnitude can reach 2^-24 of |a*b|:
//      a1b1 + (a1b2 + a2b1) + (a1b3 + a2b2 + a3b1)          [dropped: a2b3, a3b2, a3b3 <= 2^-26 |ab|]
// Each bf16 x bf16 product is exact in the fp32 accumulator, so the result differs from an exact-product
// fp32 accumulation by < 2^-25 relative per term -- below fp32's own rounding.  Six bf16 MFMAs (6 x 32
// cycles for 32x32x16) replace eight fp32 MFMAs (8 x 64 cycles): 2.67x fewer matrix-pipe cycles.
//
// Weights are split once at pack time ([K/16][3 planes][N_pad][16 k], LDS-ready).  Activations stay fp32
// in HBM; a thread splits the 8 consecutive k it stages (2 x dwordx4 -> 3 x ds_write_b128, ~45 VALU).
// Tiling, tap walk, split-K and epilogue are those of dt_conv.hip (the walk's slice arithmetic: KWalk, dt_conv_walk.h).
// LDS: per stage 3 planes x (BM+BN) rows x 32 B; the two 16-B halves of a row are swapped on rows with bit 3 set, which
// makes ds_read_b128's 16-lane groups conflict-free (rows 32 B apart would otherwise collide two-way).
#include "dt_conv_walk.h"

namespace dt {

// Wave layout: 2 x 2 waves tile the BM x BN block; each wave owns (BM/2) x (BN/2), at most 64 x 64.  256-row tiles
// (2x4 waves of 128x64, 4x2 of 64x64, 2x2 of 128x64) were measured at 81 / 145 / 103 TF/s against 179 for 128x128
//  and are not built.
template <int BM, int BN>
__global__ __launch_bounds__(256, BM * BN > 128 * 128 ? 2 : 3) void conv_gemm_bf16x6_kernel(const ConvParams p) {
  constexpr ConvForm F = *find_conv_form(KIND_BF16, BM, BN);
  constexpr int WM = F.wm(), WN = F.wn();                          // 2x2 waves
  constexpr int MI = F.mi(), NI = F.ni();
  static_assert(WM == 2 && WN == 2 && MI * 64 == BM && NI * 64 == BN, "wave layout");
  constexpr int PLANE_A = BM * 16, PLANE_B = BN * 16;            // bf16 elements per plane per stage
  constexpr int STAGE = 3 * (PLANE_A + PLANE_B);                  // bf16 elements per stage
  __shared__ __attribute__((aligned(16))) __bf16 lds[2 * STAGE];

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int wm = wave / WN, wn = wave % WN;
  const int half = lane >> 5, l31 = lane & 31;
  const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
  const int HW = p.H * p.W;
  const ConvRowMath rm = kernarg_row_math();   // (not p.rm: see kernarg_params)

  // ---- A staging: item -> (row, k-half): 8 consecutive k = 32 contiguous bytes of one pixel; AP items per thread
  constexpr int NT = 64 * WM * WN;
  constexpr int AP = (BM * 2 + NT - 1) / NT, BP = (BN * 2 + NT - 1) / NT;
  bool a_ok[AP];
  int a_y[AP], a_x[AP], a_off[AP], a_off2[AP], a_lds[AP];
#pragma unroll
  for (int i = 0; i < AP; ++i) {
    const int item = tid + i * NT;
    const int rowi = item >> 1, hh = item & 1;
    const int m = m0 + rowi;
    a_ok[i] = item < BM * 2 && m < p.M;
    const int mm = a_ok[i] ? m : 0;
    const RowPixel px = row_pixel(mm, HW, p.W, rm);
    a_y[i] = px.y; a_x[i] = px.x;
    a_off[i] = mm * p.cin_p + hh * 8;
    a_off2[i] = mm * p.cin2_p + hh * 8;                               // fused skip walk
    a_lds[i] = rowi * 16 + ((hh ^ ((rowi >> 3) & 1)) << 3);          // element offset inside a plane
  }
  // ---- B staging: the three plane tiles are contiguous [BN][16] bf16 runs in the packed weights
  const __bf16 *wbase = reinterpret_cast<const __bf16 *>(p.w) + (size_t)n0 * 16 + tid * 8;
  const size_t w_plane = (size_t)p.n_p * 16;                       // elements between planes of one chunk

  f32x16 acc[MI][NI];
  DT_CLEAR_ACC(acc, MI, NI);

  int a_frag[MI], b_frag[NI];
#pragma unroll
  for (int mi = 0; mi < MI; ++mi) {
    const int row = wm * (MI * 32) + mi * 32 + l31;
    a_frag[mi] = row * 16 + ((half ^ ((row >> 3) & 1)) << 3);
  }
#pragma unroll
  for (int ni = 0; ni < NI; ++ni) {
    const int row = wn * (NI * 32) + ni * 32 + l31;
    b_frag[ni] = row * 16 + ((half ^ ((row >> 3) & 1)) << 3);
  }

  // the walk's pipeline, over the chunks of this split-K slice and then the fused 1x1 skip walk's (KWalk, dt_conv_walk.h)
  KWalk k(p);
  const int n_main = k.n_main, n_iter = k.n_iter;
  for (int it = -1; it < n_iter; ++it) {
    const bool more = it + 1 < n_iter;
    f32x4 ra0[AP], ra1[AP];
    u32x4 rb[BP][3];
#pragma unroll
    for (int i = 0; i < AP; ++i) { ra0[i] = f32x4{0.f, 0.f, 0.f, 0.f}; ra1[i] = ra0[i]; }
    if (more && it + 1 >= n_main) {
      const int c2 = it + 1 - n_main;
#pragma unroll
      for (int i = 0; i < AP; ++i)
        if (a_ok[i]) {
          const float *src = p.in2 + a_off2[i] + c2 * 16;
          ra0[i] = *reinterpret_cast<const f32x4 *>(src);
          ra1[i] = *reinterpret_cast<const f32x4 *>(src + 4);
        }
      const __bf16 *wt = reinterpret_cast<const __bf16 *>(p.w2) + (size_t)n0 * 16 + tid * 8 + (size_t)c2 * 3 * w_plane;
#pragma unroll
      for (int i = 0; i < BP; ++i)
        if (tid + i * NT < BN * 2) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) rb[i][pl] = *reinterpret_cast<const u32x4 *>(wt + i * NT * 8 + pl * w_plane);
        }
    } else if (more) {
      int dy = 0, dx = 0;
      if (p.ksize == 3) { dy = k.tap / 3 - 1; dx = k.tap - (k.tap / 3) * 3 - 1; }
#pragma unroll
      for (int i = 0; i < AP; ++i) {
        const int yy = a_y[i] + dy, xx = a_x[i] + dx;
        if (a_ok[i] && yy >= 0 && yy < p.H && xx >= 0 && xx < p.W) {
          const float *src = p.in + a_off[i] + (dy * p.W + dx) * p.cin_p + k.cc * 16;
          ra0[i] = *reinterpret_cast<const f32x4 *>(src);
          ra1[i] = *reinterpret_cast<const f32x4 *>(src + 4);
        }
      }
      const __bf16 *wt = wbase + (size_t)(k.tap * p.ccw + k.cc) * 3 * w_plane;
#pragma unroll
      for (int i = 0; i < BP; ++i)
        if (tid + i * NT < BN * 2) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) rb[i][pl] = *reinterpret_cast<const u32x4 *>(wt + i * NT * 8 + pl * w_plane);
        }
      k.next();
    }
    if (it >= 0) {
      if (k.at_midpoint(p, it)) conv_midpoint<MI, NI>(p, acc, n0, wn, l31);
      const __bf16 *A = lds + (it & 1) * STAGE, *B = A + 3 * PLANE_A;
      bf16x8 fb[NI][3];
#pragma unroll
      for (int ni = 0; ni < NI; ++ni)
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          fb[ni][pl] = *reinterpret_cast<const bf16x8 *>(B + pl * PLANE_B + b_frag[ni]);
#pragma unroll
      for (int mi = 0; mi < MI; ++mi) {
        bf16x8 fa[3];
#pragma unroll
        for (int pl = 0; pl < 3; ++pl)
          fa[pl] = *reinterpret_cast<const bf16x8 *>(A + pl * PLANE_A + a_frag[mi]);
#pragma unroll
        for (int ni = 0; ni < NI; ++ni) mfma_bf16x6(acc[mi][ni], fa, fb[ni]);
      }
    }
    if (more) {
      __bf16 *A = lds + ((it + 1) & 1) * STAGE, *B = A + 3 * PLANE_A;
#pragma unroll
      for (int i = 0; i < AP; ++i)
        if (tid + i * NT < BM * 2) {
          bf16x8 p1, p2, p3;
          split8(ra0[i], ra1[i], p1, p2, p3);
          *reinterpret_cast<bf16x8 *>(A + a_lds[i]) = p1;
          *reinterpret_cast<bf16x8 *>(A + PLANE_A + a_lds[i]) = p2;
          *reinterpret_cast<bf16x8 *>(A + 2 * PLANE_A + a_lds[i]) = p3;
        }
#pragma unroll
      for (int i = 0; i < BP; ++i)
        if (tid + i * NT < BN * 2) {
#pragma unroll
          for (int pl = 0; pl < 3; ++pl) *reinterpret_cast<u32x4 *>(B + pl * PLANE_B + (tid + i * NT) * 8) = rb[i][pl];
        }
    }
    __syncthreads();
  }
  static_assert(2 * STAGE * sizeof(__bf16) >= F.stage_bytes(), "epilogue stage");
  conv_epilogue<BM, BN, 1, true>(p, acc, reinterpret_cast<float *>(lds), m0, n0, wm, wn, half, l31);
}

#define DT_BF16_ROW(cls, kind, bm, bn, kc, wk) {{kind, bm, bn, kc, wk, cls}, conv_gemm_bf16x6_kernel<bm, bn>},
static const ConvKernel kBf16Kernels[] = {DT_CONV_FORMS_BF16(DT_BF16_ROW)};

int launch_conv_bf16x6(const ConvParams &p, hipStream_t s) {
  conv_kernel_of(kBf16Kernels, p).fn<<<dim3((p.M + p.bm - 1) / p.bm, p.n_p / p.bn, p.splits), 256, 0, s>>>(p);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// ---------------------------------------------------------------------------------------------
// Weight split + re-tiling (once per model): wp is bf16 [K/16][3][n_p][16], element k = 8*hh + j of row n
// stored at half (hh ^ ((n>>3)&1)); k = tap*cin_p + cp with the same concat mapping as pack_conv_kernel.
__global__ void pack_conv_bf16x3_kernel(const float *__restrict__ w, __bf16 *__restrict__ wp, int cout, int cin,
                                        int ksize, int cin_p, int cin_w, int n_p, int split_c, int split_cp, size_t total) {
  for (size_t idx = blockIdx.x * (size_t)blockDim.x + threadIdx.x; idx < total; idx += (size_t)gridDim.x * blockDim.x) {
    // idx enumerates (kc, n, phys position 0..15); the three planes are written together
    const int pos = idx & 15;
    const size_t rowi = idx >> 4;
    const int n = rowi % n_p;
    const size_t kc = rowi / n_p;
    const int phh = pos >> 3, j = pos & 7;
    const int hh = phh ^ ((n >> 3) & 1);
    const int k = (int)kc * 16 + hh * 8 + j;
    const int tap = k / cin_w, cp = k - tap * cin_w;       // (channels [cin_p, cin_w) of a tap: zero chunks, see ConvParams::ccw)
    const int c = conv_real_channel(cp, cin, cin_p, split_c, split_cp);
    float v = 0.f;
    if (n < cout && c >= 0) v = w[((size_t)n * cin + c) * (ksize * ksize) + tap];
    const __bf16 a1 = (__bf16)v;
    const float r1 = v - (float)a1;
    const __bf16 a2 = (__bf16)r1;
    const __bf16 a3 = (__bf16)(r1 - (float)a2);
    const size_t base = (kc * 3 * n_p + n) * 16 + pos;
    const size_t plane = (size_t)n_p * 16;
    wp[base] = a1; wp[base + plane] = a2; wp[base + 2 * plane] = a3;
  }
}

int launch_pack_conv_bf16x3(const float *w, void *wp, int cout, int cin, int ksize, int cin_p, int cin_w, int n_p, int split_c,
                            int split_cp, hipStream_t s) {
  if (cin_w < cin_p || cin_w % 16) return DT_E_ARG;
  const size_t total = (size_t)ksize * ksize * cin_w * n_p;
  const int blocks = grid_blocks(total, 4096);
  pack_conv_bf16x3_kernel<<<blocks, 256, 0, s>>>(w, reinterpret_cast<__bf16 *>(wp), cout, cin, ksize, cin_p, cin_w, n_p,
                                                 split_c, split_cp, total);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace dt
