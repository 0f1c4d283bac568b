// What the two routes of the sample-quality scores share (dt_quality.hip: whole Gram matrices, sets of up to 2048 rows;
// dt_quality_stream.hip: row panels, sets of up to 131072 rows): the plain row loader of tile_product, the squared
// distance and the polynomial kernel from Gram entries, the KID estimator from the three kernel sums, and the integer
// reductions.  Internal: included by those two translation units only, everything in an anonymous namespace.
#ifndef DT_QUALITY_MATH_H
#define DT_QUALITY_MATH_H

#include "dt_dense64.h"

namespace {

constexpr int kWave = 64;

// Loader for tile_product: columns k .. k+3 of an fp32 row (nullptr: no such row) of len % 4 == 0 columns, as they are
struct PlainRow {
  const float *row;
  int len;
  static constexpr int W = 4;
  __device__ void operator()(int k, double (&v)[4]) const {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (row && k < len) {
      const float4 x = *reinterpret_cast<const float4 *>(row + k);
      v[0] = (double)x.x; v[1] = (double)x.y; v[2] = (double)x.z; v[3] = (double)x.w;
    }
  }
};

// squared distance from the three Gram entries; 0 exactly where all three have the same bits
__device__ inline double dist2(double gxx, double gyy, double gxy) { return fmax(0.0, (gxx + gyy) - 2.0 * gxy); }

__device__ inline double kappa(double g, double d) {
  const double t = g / d + 1.0;
  return t * t * t;
}

__device__ inline int wave_sum_int(int s) {
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

__device__ inline double kid_value(double saa, double sbb, double sab, int n_a, int n_b) {
  const double na = (double)n_a, nb = (double)n_b;
  return saa / (na * (na - 1.0)) + sbb / (nb * (nb - 1.0)) - 2.0 * sab / (na * nb);
}

// fixed-tree sum of 64-bit integers over the block; every thread gets the result
__device__ long long block_sum_int(long long s, long long *red) {
  const int t = threadIdx.x;
  red[t] = s;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const long long r = red[0];
  __syncthreads();
  return r;
}

}  // namespace
#endif  // DT_QUALITY_MATH_H
