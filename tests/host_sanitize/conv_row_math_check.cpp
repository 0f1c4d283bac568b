// Host-only check of csrc/dt_conv_rows.h: the multiply-shift row arithmetic of the convolution kernels against plain / and %.
// Built by tests/test_conv_row_math.py with the host compiler alone.
#include <stdio.h>

#include <initializer_list>

#include "dt_conv_rows.h"

using namespace dt;

static long long checks = 0, mismatches = 0;
static void expect(bool ok, const char *what, long long a, long long b, long long c) {
  ++checks;
  if (!ok && ++mismatches <= 20) printf("MISMATCH %s (%lld, %lld, %lld)\n", what, a, b, c);
}

static void check_div_pairs() {
  // every small divisor against every small numerator, then the edges of the 31-bit range for small and large divisors
  for (int d = 1; d <= 1100; ++d) {
    const RowDiv r = make_row_div(d);
    for (int n = 0; n < 70000; n += (d < 300 ? 1 : 7)) expect(row_div(n, r) == n / d, "row_div", n, d, 0);
  }
  const int ds[] = {1, 2, 3, 5, 7, 9, 15, 16, 24, 36, 255, 256, 257, 292, 768, 1000, 4095, 4096, 4097, 65535, 65536, 65537, 1 << 20,
                    (1 << 20) + 1, 131072 * 3, 1 << 30, (1 << 30) + 1, 2147483647};
  for (int d : ds) {
    const RowDiv r = make_row_div(d);
    const int top = 2147483647;
    for (int k = 0; k < 64; ++k) {
      expect(row_div(top - k, r) == (top - k) / d, "row_div top", top - k, d, 0);
      const long long q = (long long)(top / d) - k;
      if (q < 1) continue;
      const long long n = q * d;
      expect(row_div((int)n, r) == n / d, "row_div multiple", n, d, 0);
      expect(row_div((int)(n - 1), r) == (n - 1) / d, "row_div multiple - 1", n - 1, d, 0);
    }
  }
  expect(row_div(12345, make_row_div(0)) == 12345, "absent divisor", 0, 0, 0);   // (d < 1 is taken as 1: computable, never used)
}

static void check_launch(int BM, int H, int W, int m_per_tb, int dup_skip) {
  const int HW = H * W, M = 2 * BM + 7;                  // rows [0, M): two tiles and a partial third
  const ConvRowMath r = make_row_math(H, W, m_per_tb, 3);
  for (int m = 0; m < M; ++m) {
    // time-bias row: single output, both passes of the paired form, the pass-after-pass form
    expect(row_tb(m, r) == m / m_per_tb, "tb row", m, m_per_tb, BM);
    const int d1 = M + (m >= dup_skip ? m - dup_skip : m);
    expect(row_dup1(m, M, dup_skip) == d1, "second-pass row", m, dup_skip, BM);
    expect(row_tb(row_dup1(m, M, dup_skip), r) == d1 / m_per_tb, "second-pass tb row", m, m_per_tb, dup_skip);
    for (int pass = 1; pass < (dup_skip ? 2 : 3); ++pass)
      if (m >= dup_skip) {
        const int shift = pass * M - dup_skip;
        expect(row_tb(shift + m, r) == (shift + m) / m_per_tb, "pass tb row", m, pass, m_per_tb);
      }
    // picture, coordinates, class, taps
    const int img = m / HW, pix = m % HW, y = pix / W, x = pix % W;
    const RowPixel q = row_pixel(m, HW, W, r);
    expect(q.img == img && q.pix == pix && q.y == y && q.x == x, "pixel", m, H, W);
    const int cls = 3 * (y == 0 ? 0 : (y == H - 1 ? 2 : 1)) + (x == 0 ? 0 : (x == W - 1 ? 2 : 1));
    expect(pixel_class(q.y, q.x, H, W) == cls, "class", m, H, W);
    unsigned mask = 0;
    for (int t = 0; t < 9; ++t) {
      const int yy = y + t / 3 - 1, xx = x + t % 3 - 1;
      if (yy >= 0 && yy < H && xx >= 0 && xx < W) mask |= 1u << t;
    }
    expect(pixel_tap_mask(q.y, q.x, H, W) == mask, "tap mask", m, H, W);
    // pooled destination
    if (H % 2 == 0 && W % 2 == 0) {
      const long long dst = ((long long)img * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
      expect(pool_row(q, H, W) == dst, "pooled row", m, H, W);
    }
  }
  if (H % 2 == 0 && W % 2 == 0) {
    const int Wo = W >> 1, Ho = H >> 1;
    for (int j = 0; j < 8; ++j) expect(pool_window(j, W, r) == 2 * (j / Wo) * W + 2 * (j % Wo), "pool window", j, H, W);
    for (int wq = 0; wq < M; ++wq) {                     // (the separate split-K pass: pooled row -> first row of its window)
      const int xo = wq % Wo, rr = wq / Wo, yo = rr % Ho, b = rr / Ho;
      const int m00 = b * HW + 2 * yo * W + 2 * xo;
      expect(pool_first_row(wq, H, W, r) == m00, "pool first row", wq, H, W);
      expect(pool_row(row_pixel(m00, HW, W, r), H, W) == wq, "pool round trip", wq, H, W);
    }
  }
}

int main() {
  check_div_pairs();
  const int bms[] = {64, 128, 256};
  const int pics[][2] = {{1, 1}, {2, 2}, {4, 4}, {8, 8}, {16, 16}, {6, 6}, {4, 6}, {3, 5}};
  for (int BM : bms)
    for (const auto &hw : pics) {
      const int HW = hw[0] * hw[1];
      const int per_tb[] = {HW, 3 * HW, BM, BM + HW, 2 * BM + 7};
      for (int m_per_tb : per_tb)
        for (int dup_skip : {0, 256}) check_launch(BM, hw[0], hw[1], m_per_tb, dup_skip);
    }
  for (int imgs : {1, 2, 3, 64, 70, 256, 258})
    for (int img = 0; img < 3 * imgs + 5; ++img) {
      const ConvRowMath r = make_row_math(16, 16, 256, imgs);
      expect(x3_image(img, imgs, r) == img % imgs, "skip image", img, imgs, 0);
    }
  printf("conv row math ok: %lld checks, %lld mismatches\n", checks, mismatches);
  return mismatches ? 1 : 0;
}
