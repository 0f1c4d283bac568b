// Row arithmetic of the convolution kernels: GEMM row m -> time-bias row, picture, (y, x), border class, pooled row.
// The divisors (H * W, W, W / 2, H / 2, ConvParams::m_per_tb, the image count of enc1's skip) are run-time values, and an
// integer division by one is 25-35 VALU instructions on the device.  launch_conv computes one multiply-shift pair per
// divisor on the host (ConvRowMath, carried in ConvParams); the kernels divide with a shift, a 32-bit high multiply and a
// shift.  One form for every case: pictures of any size, a time-bias row per sample or per launch, tiles that hold many
// time-bias rows, rows past M (they only have to be computable, their results are masked by the callers).
// No HIP here: plain C++14 `constexpr`, evaluated alike by host and device code and checked exhaustively by the host-only
// tests/host_sanitize/conv_row_math_check.cpp.
#pragma once

namespace dt {

// n / d for 0 <= n < 2^31 and d >= 1:  with s = ceil(log2 d) and mul = floor(2^(31 + s) / d) + 1 (< 2^32),
// mul * d lies in (2^(31 + s), 2^(31 + s) + 2^s], so n * mul / 2^(31 + s) differs from n / d by less than 1 / d and has
// the same integer part.  Taking 2n instead of n makes the first 32 bits of the shift the high half of a 32 x 32 product.
struct RowDiv {
  unsigned mul;
  int shift;
};
constexpr RowDiv make_row_div(int d) {
  if (d < 1) d = 1;                                   // (absent divisors, e.g. W / 2 of a 1-pixel row: never divided by)
  int s = 0;
  while ((1ll << s) < d) ++s;
  return RowDiv{(unsigned)((1ull << (31 + s)) / (unsigned)d + 1ull), s};
}
constexpr int row_div(int n, RowDiv r) {
  return (int)((unsigned)(((unsigned long long)((unsigned)n << 1) * r.mul) >> 32) >> r.shift);
}

// the pairs of one launch
struct ConvRowMath {
  RowDiv tb;    // / m_per_tb
  RowDiv hw;    // / (H * W)
  RowDiv w;     // / W
  RowDiv wo;    // / (W / 2): pooled pixels of a tile -> pooled row pairs
  RowDiv ho;    // / (H / 2)
  RowDiv x3;    // / x3_imgs
};
constexpr ConvRowMath make_row_math(int H, int W, int m_per_tb, int x3_imgs) {
  return ConvRowMath{make_row_div(m_per_tb), make_row_div(H * W), make_row_div(W), make_row_div(W >> 1), make_row_div(H >> 1),
                     make_row_div(x3_imgs)};
}

struct RowPixel {
  int img, pix, y, x;                                 // picture, pixel inside it (y * W + x), its coordinates
};
constexpr RowPixel row_pixel(int m, int HW, int W, const ConvRowMath &r) {
  const int img = row_div(m, r.hw), pix = m - img * HW;
  const int y = row_div(pix, r.w);
  return RowPixel{img, pix, y, pix - y * W};
}

// time-bias row of GEMM row m
constexpr int row_tb(int m, const ConvRowMath &r) { return row_div(m, r.tb); }
// second pass of a dual-output launch (ConvParams::n_dup == 2): the row that pass 1 of row m writes, which is also the row
// its time-bias row is taken from; rows below dup_skip have no second pass and map to a valid row
constexpr int row_dup1(int m, int dup_rows, int dup_skip) { return dup_rows + (m >= dup_skip ? m - dup_skip : m); }

// border class of a pixel, 3 * (top / middle / bottom) + (left / middle / right): the row of tap_bias_kernel's class table
constexpr int pixel_class(int y, int x, int H, int W) {
  return 3 * (y == 0 ? 0 : (y == H - 1 ? 2 : 1)) + (x == 0 ? 0 : (x == W - 1 ? 2 : 1));
}
// the nine taps of a 3x3 walk that stay inside the picture, bit t = tap (t / 3 - 1, t % 3 - 1)
constexpr unsigned pixel_tap_mask(int y, int x, int H, int W) {
  unsigned mask = 0;
  for (int t = 0; t < 9; ++t) {
    const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
    if (yy >= 0 && yy < H && xx >= 0 && xx < W) mask |= 1u << t;
  }
  return mask;
}

// 2x2 max pool.  A 32-row tile that starts on an even picture row holds eight pooled pixels; pooled pixel j of it has its
// top-left input pixel at tile row pool_window(j): 2 * (j / Wo) * W + 2 * (j % Wo)
constexpr int pool_window(int j, int W, const ConvRowMath &r) {
  const int yy = row_div(j, r.wo);
  return 2 * yy * W + 2 * (j - yy * (W >> 1));
}
// row of the pooled tensor [imgs][H / 2][W / 2] that input pixel (img, y, x) falls into
constexpr int pool_row(const RowPixel &q, int H, int W) { return (q.img * (H >> 1) + (q.y >> 1)) * (W >> 1) + (q.x >> 1); }
// the reverse, for a thread that owns pooled row wq: the GEMM row of its window's top-left pixel
constexpr int pool_first_row(int wq, int H, int W, const ConvRowMath &r) {
  const int rr = row_div(wq, r.wo), xo = wq - rr * (W >> 1);
  const int b = row_div(rr, r.ho), yo = rr - b * (H >> 1);
  return b * (H * W) + 2 * yo * W + 2 * xo;
}

// picture of enc1's image skip behind picture `img` of the launch (the passes share the x3_imgs images)
constexpr int x3_image(int img, int x3_imgs, const ConvRowMath &r) { return img - row_div(img, r.x3) * x3_imgs; }

}  // namespace dt
