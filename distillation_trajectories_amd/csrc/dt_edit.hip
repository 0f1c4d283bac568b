// Editing stage (editing/masked_inpainting.py): the start state of a masked loop and the hole statistics of two
// trajectories.  The blend inside the reverse step lives with the update kernels (dt_update.hip, dt_fused.hip).
#include "dt_update_math.h"
#include "../../include/dt_hip_edit.h"

namespace dt {

// known[i][e] = 2 * img[i][e] - 1                                  masked_inpainting.py:178 (one product, one subtraction)
__global__ __launch_bounds__(256) void edit_known_kernel(const float4 *__restrict__ img, float4 *__restrict__ known, size_t total) {
#pragma clang fp contract(off)
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const float4 v = img[i];
    float4 o;
    o.x = 2.f * v.x - 1.f; o.y = 2.f * v.y - 1.f; o.z = 2.f * v.z - 1.f; o.w = 2.f * v.w - 1.f;
    known[i] = o;
  }
}

// x[b][e] = m * z + (1 - m) * (2 * img - 1)                        masked_inpainting.py:181; the known value is recomputed
// from the image (the same two operations), so the launch does not depend on edit_known_kernel's output
__global__ __launch_bounds__(256) void edit_start_kernel(const float4 *__restrict__ img, const int32_t *__restrict__ img_row,
                                                         const float4 *__restrict__ z, const int32_t *__restrict__ z_row,
                                                         const float4 *__restrict__ mask, const int32_t *__restrict__ mask_row,
                                                         float4 *__restrict__ x, int B, int E4) {
#pragma clang fp contract(off)
  const size_t total = (size_t)B * E4;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < total; i += (size_t)gridDim.x * blockDim.x) {
    const int b = i / E4, e = i - (size_t)b * E4;
    const float4 v = img[(size_t)(img_row ? img_row[b] : b) * E4 + e];
    const float4 zv = z[(size_t)(z_row ? z_row[b] : b) * E4 + e];
    const float4 m = mask[(size_t)(mask_row ? mask_row[b] : b) * E4 + e];
    float4 o;
    o.x = mask_blend(m.x, zv.x, 2.f * v.x - 1.f); o.y = mask_blend(m.y, zv.y, 2.f * v.y - 1.f);
    o.z = mask_blend(m.z, zv.z, 2.f * v.z - 1.f); o.w = mask_blend(m.w, zv.w, 2.f * v.w - 1.f);
    x[i] = o;
  }
}

extern "C" int dt_edit_start(const float *img, const int32_t *img_row, int n_img, const float *z, const int32_t *z_row,
                             const float *mask, const int32_t *mask_row, float *known_out, float *x_out, int B, int E,
                             void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!img || !z || !mask || !known_out || !x_out) return DT_E_NULL;
  if (B < 1 || n_img < 1 || E < 4 || E % 4) return DT_E_SHAPE;
  if (!img_row && n_img < B) return DT_E_ARG;
  if (((uintptr_t)img | (uintptr_t)z | (uintptr_t)mask | (uintptr_t)known_out | (uintptr_t)x_out) & 15) return DT_E_ARG;
  const size_t nk = (size_t)n_img * (E / 4), nx = (size_t)B * (E / 4);
  ProfileScope prof(KC_UPDATE, 0.0, 4.0 * E * (2.0 * n_img + 4.0 * B), s);
  edit_known_kernel<<<grid_blocks(nk, 2048), 256, 0, s>>>(reinterpret_cast<const float4 *>(img), reinterpret_cast<float4 *>(known_out), nk);
  DT_LAUNCH_CHECK();
  edit_start_kernel<<<grid_blocks(nx, 2048), 256, 0, s>>>(reinterpret_cast<const float4 *>(img), img_row, reinterpret_cast<const float4 *>(z),
                                                          z_row, reinterpret_cast<const float4 *>(mask), mask_row,
                                                          reinterpret_cast<float4 *>(x_out), B, E / 4);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

// out[b][i] = { sum m (x-y)^2, sum m (x-k)^2, sum m (y-k)^2, sum (1-m) (x-y)^2 } of state i of pair b: one workgroup per
// (pair, state), fp64 throughout, dt_pair_stats' accumulation scheme (per-thread strided partial sums, __shfl_down over the
// wave, the four waves through LDS in wave order: a fixed order, no atomics).
__global__ __launch_bounds__(256) void masked_pair_stats_kernel(const float *__restrict__ X, const float *__restrict__ Y, int B, int E,
                                                                const float *__restrict__ mask, const int32_t *__restrict__ mask_row,
                                                                const float *__restrict__ known, const int32_t *__restrict__ known_row,
                                                                double *__restrict__ out, int n) {
  __shared__ double sm[16];
  const int b = blockIdx.x, i = blockIdx.y;
  const float4 *x = reinterpret_cast<const float4 *>(X + ((size_t)i * B + b) * E);
  const float4 *y = reinterpret_cast<const float4 *>(Y + ((size_t)i * B + b) * E);
  const float4 *m = reinterpret_cast<const float4 *>(mask + (size_t)(mask_row ? mask_row[b] : b) * E);
  const float4 *k = reinterpret_cast<const float4 *>(known + (size_t)(known_row ? known_row[b] : b) * E);
  double acc[4] = {0.0, 0.0, 0.0, 0.0};
  for (int e = threadIdx.x; e < E / 4; e += 256) {
    const float4 a = x[e], c = y[e], mq = m[e], kq = k[e];
    const float av[4] = {a.x, a.y, a.z, a.w}, cv[4] = {c.x, c.y, c.z, c.w};
    const float mv[4] = {mq.x, mq.y, mq.z, mq.w}, kv[4] = {kq.x, kq.y, kq.z, kq.w};
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const double md = (double)mv[j];
      const double d = (double)av[j] - (double)cv[j], dx = (double)av[j] - (double)kv[j], dy = (double)cv[j] - (double)kv[j];
      acc[0] += md * (d * d);
      acc[1] += md * (dx * dx);
      acc[2] += md * (dy * dy);
      acc[3] += (1.0 - md) * (d * d);
    }
  }
  // wave sums by __shfl_down, then the four waves in order (block_sum of dt_metrics.hip)
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    double v = acc[q];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) sm[wave * 4 + q] = v;
  }
  __syncthreads();
  if (threadIdx.x < 4) {
    const int q = threadIdx.x;
    out[((size_t)b * n + i) * 4 + q] = sm[q] + sm[4 + q] + sm[8 + q] + sm[12 + q];
  }
}

extern "C" int dt_masked_pair_stats(const float *x, const float *y, int n, int B, int E, const float *mask, const int32_t *mask_row,
                                    const float *known, const int32_t *known_row, double *out, void *stream) {
  hipStream_t s = (hipStream_t)stream;
  if (!x || !y || !mask || !known || !out) return DT_E_NULL;
  if (n < 1 || B < 1 || E < 4 || E % 4 || n > 65535 || B > 65535) return DT_E_SHAPE;
  if (((uintptr_t)x | (uintptr_t)y | (uintptr_t)mask | (uintptr_t)known) & 15) return DT_E_ARG;
  ProfileScope prof(KC_METRICS, 0.0, 16.0 * B * E * (double)n, s);
  masked_pair_stats_kernel<<<dim3(B, n), 256, 0, s>>>(x, y, B, E, mask, mask_row, known, known_row, out, n);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace dt
