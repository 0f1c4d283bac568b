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
//   4. Householder tridiagonalisation of S (dt_dense64.h, shared with dt_pca.hip), Gershgorin bounds (fid_bounds_kernel)
//      and all m eigenvalues by Sturm-count bisection, one thread per eigenvalue, one wave per workgroup so that the m
//      latency-bound chains spread over m / 64 compute units (fid_bisect_kernel);
//   5. cross = sum sqrt(max(lambda, 0)) / sqrt((n_a - 1)(n_b - 1)) in index order, fid and the outputs (fid_finish_kernel).
#include <float.h>
#include <math.h>

#include "../../include/dt_hip_fid.h"
#include "dt_internal.h"
#include "dt_dense64.h"

namespace {

constexpr int kWave = 64;
enum { MISC_DMU2 = 0, MISC_TRA, MISC_TRB, MISC_GL, MISC_GU, MISC_PIVMIN, MISC_TNORM, MISC_COUNT = 16 };

// per-problem workspace (doubles), after a head of P ints (the non-finite flag) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t mean, csq, misc, M, S, v, pv, e, tau, d, lam;
  int m;
  __host__ __device__ Layout(int P, int n_a, int n_b, int D) {
    head = flag_head_bytes(P);
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
__global__ __launch_bounds__(kWave) void fid_mean_kernel(Rows R, int D, double *ws, size_t per, int *flag) {
  const int p = blockIdx.y, set = blockIdx.z;
  const int q = blockIdx.x * kWave + threadIdx.x;
  if (4 * q >= D) return;
  double m[4];
  const bool bad = quad_mean(R, p, set, set, q, m);
  const RowSet S = row_set(R, set, p);
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  for (int i = 0; i < S.n; ++i) {
    const float4 x = reinterpret_cast<const float4 *>(S.row0 + i * S.rs)[q];
    const double d0 = (double)x.x - m[0], d1 = (double)x.y - m[1], d2 = (double)x.z - m[2], d3 = (double)x.w - m[3];
    c0 = fma(d0, d0, c0); c1 = fma(d1, d1, c1); c2 = fma(d2, d2, c2); c3 = fma(d3, d3, c3);
  }
  double *base = ws + (size_t)p * per;
  double *mo = base + (size_t)set * D + 4 * (size_t)q;
  double *c = base + (size_t)(2 + set) * D + 4 * (size_t)q;
  mo[0] = m[0]; mo[1] = m[1]; mo[2] = m[2]; mo[3] = m[3];
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
// 64 x 64 tiles (tile_product, dt_dense64.h) over the D columns, rows centred as they are loaded
__global__ __launch_bounds__(kThreads) void fid_cross_kernel(Rows R, int D, double *ws, size_t per, const int *flag,
                                                             int ntb) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const int bi = blockIdx.x / ntb, bj = blockIdx.x % ntb;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  double *base = ws + (size_t)p * per;
  double acc[4][4] = {};
  tile_product(D, lr, lq, CentredRow{ra < R.n_a ? row_ptr(R, p, ra) : nullptr, base, D},
               CentredRow{rb < R.n_b ? row_ptr(R, p, R.n_a + rb) : nullptr, base + D, D}, acc);
  store_tile<false>(base + Layout(0, R.n_a, R.n_b, D).M, R.n_a, R.n_b, bi, bj, acc);
}

// ---------------------------------------------------------------------------------------------- 3. S = M M^T | M^T M
// The same tile, over the upper triangle of S.  Row i of the factor is row i of M (TRANS = false: k runs along the row,
// kdim = n_b) or column i of M (TRANS = true: kdim = n_a); the loads are coalesced along whichever index is contiguous.
// S[i][j] and S[j][i] of a diagonal tile are the same chain of the same products, so S is exactly symmetric.
// Loader for tile_product: entry k of row r of the factor (live: r < m), one per call
template <bool TRANS>
struct FactorRow {
  const double *M;
  int n_b, kdim, r;
  bool live;
  static constexpr int W = 1;
  __device__ void operator()(int k, double (&v)[1]) const {
    v[0] = live && k < kdim ? (TRANS ? M[(size_t)k * n_b + r] : M[(size_t)r * n_b + k]) : 0.0;
  }
};

template <bool TRANS>
__global__ __launch_bounds__(kThreads) void fid_square_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                              const int *flag, int nt) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  int bi, bj;
  upper_tile(blockIdx.x, nt, bi, bj);
  const Layout L(0, n_a, n_b, D);
  const int m = L.m, kdim = TRANS ? n_a : n_b;
  double *base = ws + (size_t)p * per;
  const int t = threadIdx.x;
  const int lr = TRANS ? t % 64 : t / 4, lq = TRANS ? t / 64 : t % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  double acc[4][4] = {};
  tile_product(kdim, lr, lq, FactorRow<TRANS>{base + L.M, n_b, kdim, ra, ra < m},
               FactorRow<TRANS>{base + L.M, n_b, kdim, rb, rb < m}, acc);
  store_tile<true>(base + L.S, m, m, bi, bj, acc);
}

// ---------------------------------------------------------------------------------------------- 4. eigenvalues
// the tridiagonal (d, e) out of the reduced matrix, and the Gershgorin interval that holds its spectrum
__global__ __launch_bounds__(kThreads) void fid_bounds_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                              const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b, D);
  double *base = ws + (size_t)p * per;
  const Spectrum sp = tridiagonal_spectrum(base + L.S, L.m, base + L.d, base + L.e, red);
  if (threadIdx.x == 0) {
    double *misc = base + L.misc;
    misc[MISC_GL] = sp.gl;
    misc[MISC_GU] = sp.gu;
    misc[MISC_PIVMIN] = sp.pivmin;
    misc[MISC_TNORM] = sp.tnorm;
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
  const Spectrum sp{misc[MISC_GL], misc[MISC_GU], misc[MISC_PIVMIN], misc[MISC_TNORM]};
  // the zero matrix (a set without variance): every eigenvalue is 0
  base[L.lam + j] = sp.tnorm == 0.0 ? 0.0 : bisect_eigenvalue(ds, es, n, j, sp);
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
  const Rows R{a_dev, b_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
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
