// Householder tridiagonalisation of a batch of symmetric fp64 matrices that live in a caller's workspace, and the Sturm
// count of the resulting tridiagonal: the part of the eigen stage that dt_pca.hip (top-k eigenpairs) and dt_fid.hip (all
// eigenvalues) share.  Internal: included by those two translation units only, everything in an anonymous namespace.
//
// Unblocked, dsytd2-like, lower: one reflector, one matrix-vector product and one symmetric rank-2 update per column,
// each a launch spread over the chip (an n x n fp64 matrix does not fit in LDS from n ~ 140 up).  Every sum has a fixed
// order, so a problem's result does not depend on the batch it is part of.
#ifndef DT_TRIDIAG_H
#define DT_TRIDIAG_H

#include <hip/hip_runtime.h>
#include <math.h>

#include "dt_internal.h"

namespace {

constexpr int kThreads = 256;

// Problem p works in ws + p * per (doubles): the matrix A [n][n] at offset A, and n doubles each at v (the current
// reflector), pv (tau * A v), e (off-diagonal) and tau.  st[p] != 0 skips the problem.
struct Tri {
  double *ws;
  size_t per, A, v, pv, e, tau;
  const int *st;
  int n;
};

__device__ inline double wave_sum(double s) {
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// fixed-tree sum over the block; every thread gets the result
__device__ double block_sum(double s, double *red) {
  const int t = threadIdx.x;
  red[t] = s;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) red[t] += red[t + h];
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ double block_min(double s, double *red) {
  const int t = threadIdx.x;
  red[t] = s;
  __syncthreads();
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) red[t] = fmin(red[t], red[t + h]);
    __syncthreads();
  }
  const double r = red[0];
  __syncthreads();
  return r;
}

__device__ double block_max(double s, double *red) { return -block_min(-s, red); }

// Step i (0 <= i <= n-3) works on the trailing block [i+1, n).  A stays exactly symmetric (the rank-2 update forms both
// products and adds them un-contracted), so row i is read as column i, and row i's columns i+2.. then hold the
// reflector v (v[i+1] = 1 implied): nothing reads row i of the matrix after step i.
__global__ __launch_bounds__(kThreads) void tri_reflect_kernel(Tri T, int i) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (T.st[p]) return;
  const int n = T.n;
  double *base = T.ws + (size_t)p * T.per;
  double *row = base + T.A + (size_t)i * n;
  const double alpha = row[i + 1];
  double s = 0.0;
  for (int r = i + 2 + threadIdx.x; r < n; r += kThreads) s += row[r] * row[r];
  const double xn2 = block_sum(s, red);
  double tau = 0.0, beta = alpha, scale = 0.0;
  if (xn2 != 0.0) {
    beta = -copysign(sqrt(alpha * alpha + xn2), alpha);
    tau = (beta - alpha) / beta;
    scale = 1.0 / (alpha - beta);
  }
  double *v = base + T.v;
  for (int r = i + 1 + threadIdx.x; r < n; r += kThreads) {
    if (r == i + 1) {
      v[r] = 1.0;
    } else {
      const double vr = row[r] * scale;
      v[r] = vr;
      row[r] = vr;
    }
  }
  if (threadIdx.x == 0) {
    base[T.tau + i] = tau;
    base[T.e + i] = beta;
  }
}

// p = tau * A22 v: one wave per row, 4 rows per wave, lanes over the columns then a butterfly
__global__ __launch_bounds__(kThreads) void tri_matvec_kernel(Tri T, int i) {
  const int p = blockIdx.y;
  if (T.st[p]) return;
  const int n = T.n;
  double *base = T.ws + (size_t)p * T.per;
  const double *A = base + T.A, *v = base + T.v;
  const double tau = base[T.tau + i];
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
  for (int rr = 0; rr < 4; ++rr) {
    const int r = i + 1 + (blockIdx.x * 4 + w) * 4 + rr;
    if (r >= n) break;
    const double *Ar = A + (size_t)r * n;
    double s = 0.0;
    for (int c = i + 1 + lane; c < n; c += 64) s = fma(Ar[c], v[c], s);
    s = wave_sum(s);
    if (lane == 0) base[T.pv + r] = tau * s;
  }
}

// A22 -= v w^T + w v^T, w = p - 0.5 tau (p.v) v; 64 x 64 tile per workgroup; p.v is summed by every workgroup in the
// same order
__global__ __launch_bounds__(kThreads) void tri_update_kernel(Tri T, int i, int tiles) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads];
  const int p = blockIdx.y;
  if (T.st[p]) return;
  const int n = T.n;
  double *base = T.ws + (size_t)p * T.per;
  double *A = base + T.A;
  const double *v = base + T.v, *pv = base + T.pv;
  double s = 0.0;
  for (int r = i + 1 + threadIdx.x; r < n; r += kThreads) s = fma(pv[r], v[r], s);
  const double alpha2 = -0.5 * base[T.tau + i] * block_sum(s, red);
  const int tr = blockIdx.x / tiles, tc = blockIdx.x % tiles;
  for (int q = threadIdx.x; q < 64 * 64; q += kThreads) {
    const int r = i + 1 + tr * 64 + q / 64, c = i + 1 + tc * 64 + q % 64;
    if (r < n && c < n) {
      const double wr = pv[r] + alpha2 * v[r], wc = pv[c] + alpha2 * v[c];
      const double t1 = v[r] * wc, t2 = wr * v[c];
      A[(size_t)r * n + c] -= t1 + t2;
    }
  }
}

// The n - 2 steps for P problems on stream s.  Afterwards the diagonal of A is the tridiagonal's, e[0 .. n-3] its
// off-diagonal (the last one, e[n-2], is still A[n-1][n-2]), and rows 0 .. n-3 of A hold the reflectors.
inline int tridiagonalise(const Tri &T, int P, hipStream_t s) {
  const int n = T.n;
  for (int i = 0; i + 2 < n; ++i) {
    const int m = n - 1 - i, tiles = (m + 63) / 64;
    tri_reflect_kernel<<<P, kThreads, 0, s>>>(T, i);
    DT_LAUNCH_CHECK();
    tri_matvec_kernel<<<dim3((m + 15) / 16, P), kThreads, 0, s>>>(T, i);
    DT_LAUNCH_CHECK();
    tri_update_kernel<<<dim3(tiles * tiles, P), kThreads, 0, s>>>(T, i, tiles);
    DT_LAUNCH_CHECK();
  }
  return DT_OK;
}

// number of eigenvalues of the tridiagonal (d, e) below x
__device__ inline int sturm_below(const double *d, const double *e, int n, double x, double pivmin) {
  int cnt = 0;
  double q = d[0] - x;
  if (fabs(q) < pivmin) q = -pivmin;
  cnt += q < 0.0;
  for (int i = 1; i < n; ++i) {
    q = d[i] - x - e[i - 1] * e[i - 1] / q;
    if (fabs(q) < pivmin) q = -pivmin;
    cnt += q < 0.0;
  }
  return cnt;
}

}  // namespace
#endif  // DT_TRIDIAG_H
