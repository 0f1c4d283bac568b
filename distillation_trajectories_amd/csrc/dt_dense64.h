// The fp64 dense core that dt_pca.hip (top-k eigenpairs of a centred Gram matrix), dt_fid.hip (all eigenvalues of a
// squared cross product), dt_tsne.hip and the two sample-quality routes (dt_quality.hip, dt_quality_stream.hip, through
// dt_quality_math.h) share: strided fp32 row sets and what an entry point checks of them, the column-quad mean, the staged
// 64 x 64 tile product on FMAs with its upper-triangle decode and mirrored store, Householder tridiagonalisation of a batch of symmetric matrices that live in a caller's workspace, the
// bounds of the tridiagonal's spectrum and one eigenvalue of it by Sturm-count bisection.
// Internal: included by those translation units only, everything in an anonymous namespace.
//
// Every sum has a fixed order (tile outputs: one FMA chain over k ascending; means: rows ascending, then one
// division; block reductions: one fixed tree), so a problem's result does not depend on the batch it is part of, and the
// stages cannot drift apart.
#ifndef DT_DENSE64_H
#define DT_DENSE64_H

#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>

#include "dt_internal.h"

namespace {

constexpr int kThreads = 256;

// ---------------------------------------------------------------------------------------------- rows and means
// Two sets of fp32 rows for a batch of problems: row i of problem p is a + p * a_ps + i * a_rs in set a, likewise in b.
struct Rows {
  const float *a, *b;
  long long a_ps, a_rs, b_ps, b_rs;
  int n_a, n_b;
};

// row i of problem p, counting through a's rows and on into b's: for a thread that needs one row (the tile loaders,
// PCA's components and projection); a loop over the rows of a set takes row_set below
__device__ inline const float *row_ptr(const Rows &R, int p, int i) {
  return i < R.n_a ? R.a + p * R.a_ps + i * R.a_rs : R.b + p * R.b_ps + (long long)(i - R.n_a) * R.b_rs;
}

// what the float4 loads below ask of a row set
inline bool aligned16(const void *ptr, long long s1, long long s2) {
  return ((uintptr_t)ptr & 15) == 0 && s1 % 4 == 0 && s2 % 4 == 0;
}

// bytes of the int flags (non-finite input, status) at the head of a workspace, rounded to 256
__host__ __device__ inline size_t flag_head_bytes(int count) { return ((size_t)count * sizeof(int) + 255) / 256 * 256; }

// What the set-pair entries (dt_fid_distance, dt_fid_cov_distance, dt_quality_scores, dt_quality_stream_scores) do once
// their own null and shape tests have passed, in this order: a negative stride is DT_E_SHAPE, rows or a workspace that the
// float4 / double accesses cannot take DT_E_ARG, a workspace shorter than `need` bytes DT_E_WORKSPACE; with rc == DT_OK the
// rows, the flags at the head of the workspace (`head` bytes, flag_head_bytes) and the doubles after them.
struct SetPair {
  int rc;
  Rows R;
  int *flag;
  double *wd;
};

inline SetPair set_pair_open(const float *a, int n_a, long long a_ps, long long a_rs, const float *b, int n_b,
                             long long b_ps, long long b_rs, void *ws, size_t ws_bytes, size_t need, size_t head) {
  const Rows R{a, b, a_ps, a_rs, b_ps, b_rs, n_a, n_b};
  int rc = DT_OK;
  if (a_ps < 0 || b_ps < 0 || a_rs < 0 || b_rs < 0) rc = DT_E_SHAPE;
  else if (!aligned16(a, a_ps, a_rs) || !aligned16(b, b_ps, b_rs) || ((uintptr_t)ws & 15)) rc = DT_E_ARG;
  else if (ws_bytes < need) rc = DT_E_WORKSPACE;
  return SetPair{rc, R, (int *)ws, (double *)((char *)ws + head)};
}

// one set of problem p: first row, row stride, count (a loop over one set steps a pointer; row_ptr would choose per row)
struct RowSet {
  const float *row0;
  long long rs;
  int n;
};

__device__ inline RowSet row_set(const Rows &R, int set, int p) {
  return set == 0 ? RowSet{R.a + p * R.a_ps, R.a_rs, R.n_a} : RowSet{R.b + p * R.b_ps, R.b_rs, R.n_b};
}

// Means of columns 4q .. 4q+3 over the rows of sets first .. last of problem p: a plain sum over the rows in order, then
// one division.  Returns whether any of those entries is not finite.
__device__ inline bool quad_mean(const Rows &R, int p, int first, int last, int q, double (&mean)[4]) {
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  bool bad = false;
  int n = 0;
  for (int set = first; set <= last; ++set) {
    const RowSet S = row_set(R, set, p);
    for (int i = 0; i < S.n; ++i) {
      const float4 x = reinterpret_cast<const float4 *>(S.row0 + i * S.rs)[q];
      bad |= !(isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(x.w));
      s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
    }
    n += S.n;
  }
  const double nr = (double)n;
  mean[0] = s0 / nr; mean[1] = s1 / nr; mean[2] = s2 / nr; mean[3] = s3 / nr;
  return bad;
}

// ---------------------------------------------------------------------------------------------- 64 x 64 tile product
// One 64 x 64 output tile per workgroup of kThreads, 4 x 4 outputs per thread (rows ty + 16u, columns tx + 16w), 16 k
// per LDS stage.  Each output is one fp64 FMA chain over k = 0 .. kdim-1 in order.  Thread t stages k = 4 lq .. 4 lq + 3
// of row lr of both factors' tile rows: la(k, v) / lb(k, v) give v[i] = factor[row][k + i] for i < Load::W (4: one
// float4 of a row; 1: one element), 0.0 where the row or the k is past the end.  Each W loads go to LDS before the next
// are issued: with all four of an element loader in flight the square kernels of dt_fid.hip need 10 more VGPRs.
template <class Load>
__device__ inline void tile_product(int kdim, int lr, int lq, const Load &la, const Load &lb, double (&acc)[4][4]) {
  __shared__ double As[16][64], Bs[16][64];
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  for (int k0 = 0; k0 < kdim; k0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; c += Load::W) {
      double va[Load::W], vb[Load::W];
      la(k0 + 4 * lq + c, va);
      lb(k0 + 4 * lq + c, vb);
#pragma unroll
      for (int i = 0; i < Load::W; ++i) {
        As[4 * lq + c + i][lr] = va[i];
        Bs[4 * lq + c + i][lr] = vb[i];
      }
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; ++kk) {
      double a[4], b[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) { a[u] = As[kk][ty + 16 * u]; b[u] = Bs[kk][tx + 16 * u]; }
#pragma unroll
      for (int u = 0; u < 4; ++u)
#pragma unroll
        for (int w = 0; w < 4; ++w) acc[u][w] = fma(a[u], b[w], acc[u][w]);
    }
    __syncthreads();
  }
}

// Loader for tile_product: columns k .. k+3 of an fp32 row (nullptr: no such row) of len % 4 == 0 columns, centred
struct CentredRow {
  const float *row;
  const double *mean;
  int len;
  static constexpr int W = 4;
  __device__ void operator()(int k, double (&v)[4]) const {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (row && k < len) {
      const float4 x = *reinterpret_cast<const float4 *>(row + k);
      v[0] = (double)x.x - mean[k]; v[1] = (double)x.y - mean[k + 1];
      v[2] = (double)x.z - mean[k + 2]; v[3] = (double)x.w - mean[k + 3];
    }
  }
};

// tile number 0 .. nt (nt + 1) / 2 - 1 of the upper triangle of nt x nt tiles, row by row -> (bi, bj), bi <= bj
__device__ inline void upper_tile(int tile, int nt, int &bi, int &bj) {
  bi = 0;
  while (tile >= nt - bi) { tile -= nt - bi; ++bi; }
  bj = bi + tile;
}

// tile (bi, bj) of C [nr][nc]; MIRROR: C is square and an off-diagonal tile is written to (bj, bi) as well
template <bool MIRROR>
__device__ inline void store_tile(double *C, int nr, int nc, int bi, int bj, const double (&acc)[4][4]) {
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int r = bi * 64 + ty + 16 * u, c = bj * 64 + tx + 16 * w;
      if (r < nr && c < nc) {
        C[(size_t)r * nc + c] = acc[u][w];
        if (MIRROR && bi != bj) C[(size_t)c * nc + r] = acc[u][w];
      }
    }
}

// the accumulator of v_mfma_f64_16x16x4_f64: cov_gram_kernel (dt_fid.hip) and gram_tile (dt_quality_stream.hip) each keep
// their own stage loop on it -- one shared routine was measured and cost the panel route its stage times
typedef double mfma_acc __attribute__((ext_vector_type(4)));

// ---------------------------------------------------------------------------------------------- tridiagonalisation
// Unblocked, dsytd2-like, lower: one reflector, one matrix-vector product and one symmetric rank-2 update per column,
// each a launch spread over the chip (an n x n fp64 matrix does not fit in LDS from n ~ 140 up).
//
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

// ---------------------------------------------------------------------------------------------- eigenvalues
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

// The interval [gl, gu] that holds the spectrum (Gershgorin, widened by the rounding of a Sturm count), the pivot floor
// of the counts and the norm their tolerance is measured in.
struct Spectrum {
  double gl, gu, pivmin, tnorm;
};

// One workgroup of kThreads: reads the tridiagonal out of the reduced matrix A [n][n] that tridiagonalise left (its
// diagonal into d[0 .. n-1], the last off-diagonal into e[n-2]) and bounds its spectrum.  onenrm, where asked for,
// receives max_i (|d_i| + |e_i-1| + |e_i|).
__device__ inline Spectrum tridiagonal_spectrum(const double *A, int n, double *d, double *e, double *red,
                                                double *onenrm = nullptr) {
  const int t = threadIdx.x;
  for (int i = t; i < n; i += kThreads) d[i] = A[(size_t)i * n + i];
  if (t == 0) e[n - 2] = A[(size_t)(n - 1) * n + n - 2];
  __syncthreads();
  double lo = INFINITY, hi = -INFINITY, nrm = 0.0, e2max = 0.0;
  for (int i = t; i < n; i += kThreads) {
    const double off = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i < n - 1 ? fabs(e[i]) : 0.0);
    lo = fmin(lo, d[i] - off);
    hi = fmax(hi, d[i] + off);
    nrm = fmax(nrm, fabs(d[i]) + off);
    if (i < n - 1) e2max = fmax(e2max, e[i] * e[i]);
  }
  Spectrum s;
  s.gl = block_min(lo, red);
  s.gu = block_max(hi, red);
  if (onenrm) *onenrm = block_max(nrm, red);
  s.pivmin = DBL_MIN * fmax(1.0, block_max(e2max, red));
  s.tnorm = fmax(fabs(s.gl), fabs(s.gu));
  s.gl -= 2.0 * DBL_EPSILON * s.tnorm * n + 2.0 * s.pivmin;
  s.gu += 2.0 * DBL_EPSILON * s.tnorm * n + 2.0 * s.pivmin;
  return s;
}

// eigenvalue `index` (ascending, from 0) of the tridiagonal (d, e) by bisection of [gl, gu]
__device__ inline double bisect_eigenvalue(const double *d, const double *e, int n, int index, const Spectrum &s) {
  double a = s.gl, b = s.gu;
  for (int it = 0; it < 256; ++it) {
    const double tol = 2.0 * DBL_EPSILON * fmax(fabs(a), fabs(b)) + DBL_EPSILON * s.tnorm;
    if (b - a <= tol) break;
    const double mid = 0.5 * (a + b);
    if (sturm_below(d, e, n, mid, s.pivmin) > index) b = mid; else a = mid;
  }
  return 0.5 * (a + b);
}

}  // namespace
#endif  // DT_DENSE64_H
