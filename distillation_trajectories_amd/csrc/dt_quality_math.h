// What the two routes of the sample-quality scores share (dt_quality.hip: whole Gram matrices, sets of up to 2048 rows;
// dt_quality_stream.hip: row panels, sets of up to 131072 rows): the plain row loader of tile_product, the squared
// distance, its 63-bit key and the polynomial kernel from Gram entries, the tail of the per-problem workspace, the work of
// one wave on one row of a Gram matrix (the (k+1)-th smallest key, the kernel sum, the counts), the KID estimator from the
// three kernel sums, the integer reductions and the finish.  The routes differ in where a Gram row comes from and in
// nothing else: the definitions and every order of summation are here, once.  Internal: included by those two
// translation units only, everything in an anonymous namespace.
#ifndef DT_QUALITY_MATH_H
#define DT_QUALITY_MATH_H

#include "../../include/dt_hip_quality.h"
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

// The per-problem vectors that both routes' workspace layouts end in (each Layout's last member), as offsets in doubles
// from `first` on; `end` is the first double after them
struct ScoreTail {
  size_t diag, r2, rs, hits;
  __host__ __device__ size_t place(size_t first, size_t na, size_t nb) {
    diag = first;                     // G(a_i, a_i), then G(b_j, b_j)
    r2 = diag + na + nb;              // squared radii, A's then B's
    rs = r2 + na + nb;                // kappa row sums: A x A, B x B, A x B
    hits = rs + 2 * na + nb;          // ints: recall flag [n_a], density count [n_a], precision flag [n_b]
    return hits + (2 * na + nb + 1) / 2;
  }
};

// squared distance from the three Gram entries; 0 exactly where all three have the same bits
__device__ inline double dist2(double gxx, double gyy, double gxy) { return fmax(0.0, (gxx + gyy) - 2.0 * gxy); }

// its 63-bit pattern: a non-negative double orders as its bit pattern
__device__ inline unsigned long long dist2_key(double gxx, double gyy, double gxy) {
  return (unsigned long long)__double_as_longlong(dist2(gxx, gyy, gxy)) & 0x7fffffffffffffffull;
}

__device__ inline double kappa(double g, double d) {
  const double t = g / d + 1.0;
  return t * t * t;
}

__device__ inline int wave_sum_int(int s) {
  for (int m = 32; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// The (k+1)-th smallest of buf[0 .. count), count > k: the largest r with fewer than k + 1 keys below it, built bit by bit
// from the top, each bit one count over the buffer -- 63 passes whatever k is.  One wave of one workgroup.
__device__ inline unsigned long long select_key(const unsigned long long *buf, int count, int k) {
  unsigned long long r = 0;
  for (int bit = 62; bit >= 0; --bit) {
    const unsigned long long trial = r | (1ull << bit);
    int below = 0;
    for (int j = threadIdx.x; j < count; j += kWave) below += buf[j] < trial;
    if (wave_sum_int(below) <= k) r = trial;
  }
  return r;
}

// sum of kappa over the n entries of a Gram row but entry `skip` (-1: none): lanes over the columns in ascending order,
// then the butterfly, so a row's sum does not depend on where the row was formed.  One wave of one workgroup.
__device__ inline double kappa_row_sum(const double *G, int n, int skip, double dd) {
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kWave)
    if (j != skip) s += kappa(G[j], dd);
  return wave_sum(s);
}

// Row G of d2(A, B), a_i against every b_j: *reached = whether some b_j has a_i within its radius (recall), *within = how
// many b_j lie within a_i's (density; coverage is whether any does).  One wave of one workgroup.
__device__ inline void count_row(const double *G, int n_b, double gi, double ri, const double *gb, const double *rb,
                                 int *reached_out, int *within_out) {
  int within = 0, reached = 0;
  for (int j = threadIdx.x; j < n_b; j += kWave) {
    const double d = dist2(gi, gb[j], G[j]);
    within += d < ri;
    reached |= d < rb[j];
  }
  within = wave_sum_int(within);
  reached = wave_sum_int(reached) != 0;
  if (threadIdx.x == 0) {
    *reached_out = reached;
    *within_out = within;
  }
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

// The finish of problem p = blockIdx.x by one workgroup of kThreads: the fixed trees over the row sums and the hits, KID,
// counts, radii and status; `bad`: an input was not finite.  abase / base: the problem's part of the workspace that holds
// the A side's vectors (diag, r2 and rs of A x A) and the one that holds the rest (distinct only for a shared teacher on
// the panel route).  kid_out[p * kid_stride] receives the KID.
__device__ inline void score_finish(bool bad, int n_a, int n_b, const ScoreTail &T, const double *abase, const double *base,
                                    double *kid_out, int kid_stride, long long *counts_out, double *radii_out,
                                    int *status_out) {
  __shared__ double red[kThreads];
  __shared__ long long redi[kThreads];
  const int p = blockIdx.x, t = threadIdx.x;
  double *kid = kid_out + (size_t)p * kid_stride;
  long long *counts = counts_out + 4 * (size_t)p;
  double *radii = radii_out ? radii_out + (size_t)p * (n_a + n_b) : nullptr;
  if (bad) {
    if (radii)
      for (int i = t; i < n_a + n_b; i += kThreads) radii[i] = NAN;
    if (t == 0) {
      kid[0] = NAN;                        // the subsets' entries: quality_subset_kernel
      counts[0] = counts[1] = counts[2] = counts[3] = -1;
      status_out[p] = DT_QUALITY_NONFINITE;
    }
    return;
  }
  const double *rs = base + T.rs, *rsa = abase + T.rs;
  const int *hits = reinterpret_cast<const int *>(base + T.hits);
  double saa = 0.0, sbb = 0.0, sab = 0.0;
  long long recall = 0, density = 0, coverage = 0, precision = 0;
  for (int i = t; i < n_a; i += kThreads) {
    saa += rsa[i];
    sab += rs[n_a + n_b + i];
    recall += hits[i];
    density += hits[n_a + i];
    coverage += hits[n_a + i] > 0;
  }
  for (int j = t; j < n_b; j += kThreads) {
    sbb += rs[n_a + j];
    precision += hits[2 * n_a + j];
  }
  saa = block_sum(saa, red);
  sbb = block_sum(sbb, red);
  sab = block_sum(sab, red);
  precision = block_sum_int(precision, redi);
  recall = block_sum_int(recall, redi);
  density = block_sum_int(density, redi);
  coverage = block_sum_int(coverage, redi);
  if (radii)
    for (int i = t; i < n_a + n_b; i += kThreads) radii[i] = (i < n_a ? abase : base)[T.r2 + i];
  if (t == 0) {
    kid[0] = kid_value(saa, sbb, sab, n_a, n_b);
    counts[0] = precision;
    counts[1] = recall;
    counts[2] = density;
    counts[3] = coverage;
    status_out[p] = DT_QUALITY_OK;
  }
}

}  // namespace
#endif  // DT_QUALITY_MATH_H
