// Fréchet distance between two feature sets for a batch of independent problems (include/dt_hip_fid.h): the arithmetic
// of the FID stage on the device, without a D x D matrix.
//
// Stages, per problem, all in fp64 (every output summed in a fixed order, so a result does not depend on P, on the other
// problems of the launch or on the strides):
//   1. column means of both sets, the non-finite flag and the column sums of squared deviations (fid_mean_kernel);
//      |mu_A - mu_B|^2 and the two traces sum |row - mu|^2 / (n - 1) (fid_stats_kernel);
//   2. the centred cross product M = A_c B_c^T, n_a x n_b, 64 x 64 tiles, rows centred as they are loaded: the features
//      sit on a large common offset that must not reach the product (fid_cross_kernel);
//   3. S = M M^T (n_a <= n_b) or M^T M, side m = min(n_a, n_b), upper-triangle tiles mirrored into full symmetric
//      storage (fid_square_kernel);
//   4. Householder tridiagonalisation of S (dt_tridiag.h, shared with dt_pca.hip), Gershgorin bounds (fid_bounds_kernel)
//      and all m eigenvalues by Sturm-count bisection, one thread per eigenvalue, one wave per workgroup so that the m
//      latency-bound chains spread over m / 64 compute units (fid_bisect_kernel);
//   5. cross = sum sqrt(max(lambda, 0)) / sqrt((n_a - 1)(n_b - 1)) in index order, fid and the outputs (fid_finish_kernel).
#include <float.h>
#include <math.h>

#include "../../include/dt_hip_fid.h"
#include "dt_internal.h"
#include "dt_tridiag.h"

namespace {

constexpr int kWave = 64;
enum { MISC_DMU2 = 0, MISC_TRA, MISC_TRB, MISC_GL, MISC_GU, MISC_PIVMIN, MISC_TNORM, MISC_COUNT = 16 };

struct Sets {
  const float *a, *b;
  long long a_ps, a_rs, b_ps, b_rs;
  int n_a, n_b;
};

__device__ inline const float *set_row(const Sets &R, int set, int p, int i) {
  return set == 0 ? R.a + p * R.a_ps + i * R.a_rs : R.b + p * R.b_ps + i * R.b_rs;
}

// per-problem workspace (doubles), after a head of P ints (the non-finite flag) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t mean, csq, misc, M, S, v, pv, e, tau, d, lam;
  int m;
  __host__ __device__ Layout(int P, int n_a, int n_b, int D) {
    head = ((size_t)P * sizeof(int) + 255) / 256 * 256;
    m = n_a < n_b ? n_a : n_b;
    const size_t N = (size_t)m;
    mean = 0;                                   // [2][D]
    csq = mean + 2 * (size_t)D;                 // [2][D]
    misc = csq + 2 * (size_t)D;
    M = misc + MISC_COUNT;
    S = M + (size_t)n_a * n_b;
    v = S + N * N;
    pv = v + N;
    e = pv + N;
    tau = e + N;
    d = tau + N;
    lam = d + N;
    per = lam + N;
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

// ---------------------------------------------------------------------------------------------- 1. means and traces
// one thread per quad of columns, rows in order; blockIdx.z is the set
__global__ __launch_bounds__(kWave) void fid_mean_kernel(Sets R, int D, double *ws, size_t per, int *flag) {
  const int p = blockIdx.y, set = blockIdx.z;
  const int q = blockIdx.x * kWave + threadIdx.x;
  if (4 * q >= D) return;
  const int n = set == 0 ? R.n_a : R.n_b;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  bool bad = false;
  for (int i = 0; i < n; ++i) {
    const float4 x = reinterpret_cast<const float4 *>(set_row(R, set, p, i))[q];
    bad |= !(isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(x.w));
    s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
  }
  const double nr = (double)n;
  const double m0 = s0 / nr, m1 = s1 / nr, m2 = s2 / nr, m3 = s3 / nr;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  for (int i = 0; i < n; ++i) {
    const float4 x = reinterpret_cast<const float4 *>(set_row(R, set, p, i))[q];
    const double d0 = (double)x.x - m0, d1 = (double)x.y - m1, d2 = (double)x.z - m2, d3 = (double)x.w - m3;
    c0 = fma(d0, d0, c0); c1 = fma(d1, d1, c1); c2 = fma(d2, d2, c2); c3 = fma(d3, d3, c3);
  }
  double *base = ws + (size_t)p * per;
  double *m = base + (size_t)set * D + 4 * (size_t)q;
  double *c = base + (size_t)(2 + set) * D + 4 * (size_t)q;
  m[0] = m0; m[1] = m1; m[2] = m2; m[3] = m3;
  c[0] = c0; c[1] = c1; c[2] = c2; c[3] = c3;
  if (bad) atomicOr(flag + p, 1);
}

__global__ __launch_bounds__(kThreads) void fid_stats_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                             const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (flag[p]) return;
  double *base = ws + (size_t)p * per;
  const double *ma = base, *mb = base + D, *ca = base + 2 * (size_t)D, *cb = base + 3 * (size_t)D;
  double s = 0.0, ta = 0.0, tb = 0.0;
  for (int e = threadIdx.x; e < D; e += kThreads) {
    const double d = ma[e] - mb[e];
    s = fma(d, d, s);
    ta += ca[e];
    tb += cb[e];
  }
  const double dmu2 = block_sum(s, red), sa = block_sum(ta, red), sb = block_sum(tb, red);
  if (threadIdx.x == 0) {
    double *misc = base + Layout(0, n_a, n_b, D).misc;
    misc[MISC_DMU2] = dmu2;
    misc[MISC_TRA] = sa / (double)(n_a - 1);
    misc[MISC_TRB] = sb / (double)(n_b - 1);
  }
}

// ---------------------------------------------------------------------------------------------- 2. M = A_c B_c^T
// 64 x 64 output tile per workgroup, 4 x 4 outputs per thread (rows ty + 16a, columns tx + 16b), 16 columns of D per
// LDS stage.  Each output is one fp64 FMA chain over e = 0 .. D-1 in order.
__global__ __launch_bounds__(kThreads) void fid_cross_kernel(Sets R, int D, double *ws, size_t per, const int *flag,
                                                             int ntb) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const int bi = blockIdx.x / ntb, bj = blockIdx.x % ntb;
  __shared__ double As[16][64], Bs[16][64];
  const int t = threadIdx.x, tx = t % 16, ty = t / 16;
  const int lr = t / 4, lq = t % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  const float *pa = ra < R.n_a ? set_row(R, 0, p, ra) : nullptr;
  const float *pb = rb < R.n_b ? set_row(R, 1, p, rb) : nullptr;
  double *base = ws + (size_t)p * per;
  const double *ma = base, *mb = base + D;
  double acc[4][4] = {};
  for (int e0 = 0; e0 < D; e0 += 16) {
    const int e = e0 + 4 * lq;
    double va[4] = {0.0, 0.0, 0.0, 0.0}, vb[4] = {0.0, 0.0, 0.0, 0.0};
    if (e < D) {
      if (pa) {
        const float4 x = *reinterpret_cast<const float4 *>(pa + e);
        va[0] = (double)x.x - ma[e]; va[1] = (double)x.y - ma[e + 1];
        va[2] = (double)x.z - ma[e + 2]; va[3] = (double)x.w - ma[e + 3];
      }
      if (pb) {
        const float4 x = *reinterpret_cast<const float4 *>(pb + e);
        vb[0] = (double)x.x - mb[e]; vb[1] = (double)x.y - mb[e + 1];
        vb[2] = (double)x.z - mb[e + 2]; vb[3] = (double)x.w - mb[e + 3];
      }
    }
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      As[4 * lq + c][lr] = va[c];
      Bs[4 * lq + c][lr] = vb[c];
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
  double *M = base + Layout(0, R.n_a, R.n_b, D).M;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int r = bi * 64 + ty + 16 * u, c = bj * 64 + tx + 16 * w;
      if (r < R.n_a && c < R.n_b) M[(size_t)r * R.n_b + c] = acc[u][w];
    }
}

// ---------------------------------------------------------------------------------------------- 3. S = M M^T | M^T M
// The same tile, over the upper triangle of S.  Row i of the factor is row i of M (TRANS = false: k runs along the row,
// kdim = n_b) or column i of M (TRANS = true: kdim = n_a); the loads are coalesced along whichever index is contiguous.
// S[i][j] and S[j][i] of a diagonal tile are the same chain of the same products, so S is exactly symmetric.
template <bool TRANS>
__global__ __launch_bounds__(kThreads) void fid_square_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                              const int *flag, int nt) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  int tile = blockIdx.x, bi = 0;
  while (tile >= nt - bi) { tile -= nt - bi; ++bi; }
  const int bj = bi + tile;
  __shared__ double As[16][64], Bs[16][64];
  const Layout L(0, n_a, n_b, D);
  const int m = L.m, kdim = TRANS ? n_a : n_b;
  double *base = ws + (size_t)p * per;
  const double *M = base + L.M;
  const int t = threadIdx.x, tx = t % 16, ty = t / 16;
  const int lr = TRANS ? t % 64 : t / 4, lq = TRANS ? t / 64 : t % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < kdim; k0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + 4 * lq + c;
      double va = 0.0, vb = 0.0;
      if (k < kdim) {
        if (ra < m) va = TRANS ? M[(size_t)k * n_b + ra] : M[(size_t)ra * n_b + k];
        if (rb < m) vb = TRANS ? M[(size_t)k * n_b + rb] : M[(size_t)rb * n_b + k];
      }
      As[4 * lq + c][lr] = va;
      Bs[4 * lq + c][lr] = vb;
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
  double *S = base + L.S;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) {
      const int r = bi * 64 + ty + 16 * u, c = bj * 64 + tx + 16 * w;
      if (r < m && c < m) {
        S[(size_t)r * m + c] = acc[u][w];
        if (bi != bj) S[(size_t)c * m + r] = acc[u][w];
      }
    }
}

// ---------------------------------------------------------------------------------------------- 4. eigenvalues
// the tridiagonal (d, e) out of the reduced matrix, and the Gershgorin interval that holds its spectrum
__global__ __launch_bounds__(kThreads) void fid_bounds_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                              const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b, D);
  const int n = L.m, t = threadIdx.x;
  double *base = ws + (size_t)p * per;
  const double *A = base + L.S;
  double *d = base + L.d, *e = base + L.e;
  for (int i = t; i < n; i += kThreads) d[i] = A[(size_t)i * n + i];
  if (t == 0) e[n - 2] = A[(size_t)(n - 1) * n + n - 2];
  __syncthreads();
  double lo = INFINITY, hi = -INFINITY, e2max = 0.0;
  for (int i = t; i < n; i += kThreads) {
    const double off = (i > 0 ? fabs(e[i - 1]) : 0.0) + (i < n - 1 ? fabs(e[i]) : 0.0);
    lo = fmin(lo, d[i] - off);
    hi = fmax(hi, d[i] + off);
    if (i < n - 1) e2max = fmax(e2max, e[i] * e[i]);
  }
  double gl = block_min(lo, red), gu = block_max(hi, red);
  const double pivmin = DBL_MIN * fmax(1.0, block_max(e2max, red));
  const double tnorm = fmax(fabs(gl), fabs(gu));
  gl -= 2.0 * DBL_EPSILON * tnorm * n + 2.0 * pivmin;
  gu += 2.0 * DBL_EPSILON * tnorm * n + 2.0 * pivmin;
  if (t == 0) {
    double *misc = base + L.misc;
    misc[MISC_GL] = gl;
    misc[MISC_GU] = gu;
    misc[MISC_PIVMIN] = pivmin;
    misc[MISC_TNORM] = tnorm;
  }
}

// eigenvalue j (ascending) by bisection, one thread each; the tridiagonal is staged in LDS
__global__ __launch_bounds__(kWave) void fid_bisect_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                           const int *flag) {
  __shared__ double ds[DT_FID_MAX_SIDE], es[DT_FID_MAX_SIDE];
  const int p = blockIdx.y;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b, D);
  const int n = L.m;
  double *base = ws + (size_t)p * per;
  for (int i = threadIdx.x; i < n; i += kWave) {
    ds[i] = base[L.d + i];
    es[i] = i < n - 1 ? base[L.e + i] : 0.0;
  }
  __syncthreads();
  const int j = blockIdx.x * kWave + threadIdx.x;
  if (j >= n) return;
  const double *misc = base + L.misc;
  const double pivmin = misc[MISC_PIVMIN], tnorm = misc[MISC_TNORM];
  double a = misc[MISC_GL], b = misc[MISC_GU];
  if (tnorm == 0.0) {                            // the zero matrix (a set without variance): every eigenvalue is 0
    base[L.lam + j] = 0.0;
    return;
  }
  for (int it = 0; it < 256; ++it) {
    const double tol = 2.0 * DBL_EPSILON * fmax(fabs(a), fabs(b)) + DBL_EPSILON * tnorm;
    if (b - a <= tol) break;
    const double mid = 0.5 * (a + b);
    if (sturm_below(ds, es, n, mid, pivmin) > j) b = mid; else a = mid;
  }
  base[L.lam + j] = 0.5 * (a + b);
}

// ---------------------------------------------------------------------------------------------- 5. the distance
__global__ __launch_bounds__(kThreads) void fid_finish_kernel(int n_a, int n_b, int D, const double *ws, size_t per,
                                                              const int *flag, double *fid_out, double *parts_out,
                                                              int *status_out) {
  __shared__ double sv[DT_FID_MAX_SIDE];
  const int p = blockIdx.x, t = threadIdx.x;
  double *parts = parts_out + 4 * (size_t)p;
  if (flag[p]) {
    if (t == 0) {
      fid_out[p] = NAN;
      parts[0] = parts[1] = parts[2] = parts[3] = NAN;
      status_out[p] = DT_FID_NONFINITE;
    }
    return;
  }
  const Layout L(0, n_a, n_b, D);
  const double *base = ws + (size_t)p * per;
  for (int j = t; j < L.m; j += kThreads) sv[j] = sqrt(fmax(base[L.lam + j], 0.0));
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < L.m; ++j) s += sv[j];
    const double *misc = base + L.misc;
    const double cross = s / sqrt((double)(n_a - 1) * (double)(n_b - 1));
    parts[0] = misc[MISC_DMU2];
    parts[1] = misc[MISC_TRA];
    parts[2] = misc[MISC_TRB];
    parts[3] = cross;
    fid_out[p] = misc[MISC_DMU2] + misc[MISC_TRA] + misc[MISC_TRB] - 2.0 * cross;
    status_out[p] = DT_FID_OK;
  }
}

bool aligned16(const void *ptr, long long s1, long long s2) {
  return ((uintptr_t)ptr & 15) == 0 && s1 % 4 == 0 && s2 % 4 == 0;
}

bool shape_ok(int P, int n_a, int n_b, int D) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_b >= 2 && n_a <= 32768 && n_b <= 32768 &&
         (n_a < n_b ? n_a : n_b) <= DT_FID_MAX_SIDE && D >= 4 && D % 4 == 0 && D <= (1 << 20);
}

}  // namespace

extern "C" size_t dt_fid_workspace_bytes(int P, int n_a, int n_b, int D) {
  if (!shape_ok(P, n_a, n_b, D)) return 0;
  return Layout(P, n_a, n_b, D).bytes(P);
}

extern "C" int dt_fid_distance(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                               const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P, int D,
                               double *fid_dev, double *parts_dev, int *status_dev, void *ws, size_t ws_bytes,
                               void *const *events, void *stream) {
  if (!a_dev || !b_dev || !fid_dev || !parts_dev || !status_dev || !ws) return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b, D) || a_pstride < 0 || b_pstride < 0 || a_rstride < 0 || b_rstride < 0) return DT_E_SHAPE;
  if (!aligned16(a_dev, a_pstride, a_rstride) || !aligned16(b_dev, b_pstride, b_rstride) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const Layout L(P, n_a, n_b, D);
  if (ws_bytes < L.bytes(P)) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  const Sets R{a_dev, b_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
  int *flag = (int *)ws;
  double *wd = (double *)((char *)ws + L.head);
  const int m = L.m;
  DT_HIP_TRY(hipMemsetAsync(ws, 0, L.head, s));
  fid_mean_kernel<<<dim3((D / 4 + kWave - 1) / kWave, P, 2), kWave, 0, s>>>(R, D, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  fid_stats_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, D, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[1], s));
  const int nta = (n_a + 63) / 64, ntb = (n_b + 63) / 64, nt = (m + 63) / 64;
  fid_cross_kernel<<<dim3(nta * ntb, P), kThreads, 0, s>>>(R, D, wd, L.per, flag, ntb);
  DT_LAUNCH_CHECK();
  if (n_a <= n_b)
    fid_square_kernel<false><<<dim3(nt * (nt + 1) / 2, P), kThreads, 0, s>>>(n_a, n_b, D, wd, L.per, flag, nt);
  else
    fid_square_kernel<true><<<dim3(nt * (nt + 1) / 2, P), kThreads, 0, s>>>(n_a, n_b, D, wd, L.per, flag, nt);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[2], s));
  const Tri T{wd, L.per, L.S, L.v, L.pv, L.e, L.tau, flag, m};
  if (const int rc = tridiagonalise(T, P, s)) return rc;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[3], s));
  fid_bounds_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, D, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  fid_bisect_kernel<<<dim3((m + kWave - 1) / kWave, P), kWave, 0, s>>>(n_a, n_b, D, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  fid_finish_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, D, wd, L.per, flag, fid_dev, parts_dev, status_dev);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[4], s));
  return DT_OK;
}
