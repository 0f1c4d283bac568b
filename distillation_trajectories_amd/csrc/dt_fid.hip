// Fréchet distance between two feature sets for a batch of independent problems (include/dt_hip_fid.h): the arithmetic
// of the FID stage on the device.  Two routes share stages 4 and 5: the sample-space one below, without a D x D matrix,
// for a smaller set of at most 2048 rows, and the feature-space one (include/dt_hip_fid_cov.h) further down, through
// the D x D covariance products, for sets of any length.
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
#include "../../include/dt_hip_fid_cov.h"
#include "dt_internal.h"
#include "dt_dense64.h"

namespace {

constexpr int kWave = 64;
enum { MISC_DMU2 = 0, MISC_TRA, MISC_TRB, MISC_GL, MISC_GU, MISC_PIVMIN, MISC_TNORM, MISC_TOL, MISC_COUNT = 16 };

// what stages 4 and 5 need of a route's per-problem layout: the squared matrix S [m][m], its tridiagonal and eigenvalues
struct Tail {
  size_t misc, S, d, e, lam;
  int m, n_a, n_b;
};

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
__global__ __launch_bounds__(kThreads) void fid_bounds_kernel(Tail L, double *ws, size_t per, const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (flag[p]) return;
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
__global__ __launch_bounds__(kWave) void fid_bisect_kernel(Tail L, double *ws, size_t per, const int *flag) {
  __shared__ double ds[DT_FID_MAX_SIDE], es[DT_FID_MAX_SIDE];
  const int p = blockIdx.y;
  if (flag[p]) return;
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
__global__ __launch_bounds__(kThreads) void fid_finish_kernel(Tail L, const double *ws, size_t per, const int *flag,
                                                              double *fid_out, double *parts_out, int *status_out) {
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
  const double *base = ws + (size_t)p * per;
  for (int j = t; j < L.m; j += kThreads) sv[j] = sqrt(fmax(base[L.lam + j], 0.0));
  __syncthreads();
  if (t == 0) {
    double s = 0.0;
    for (int j = 0; j < L.m; ++j) s += sv[j];
    const double *misc = base + L.misc;
    const double cross = s / sqrt((double)(L.n_a - 1) * (double)(L.n_b - 1));
    parts[0] = misc[MISC_DMU2];
    parts[1] = misc[MISC_TRA];
    parts[2] = misc[MISC_TRB];
    parts[3] = cross;
    fid_out[p] = misc[MISC_DMU2] + misc[MISC_TRA] + misc[MISC_TRB] - 2.0 * cross;
    status_out[p] = DT_FID_OK;
  }
}

// bounds, bisection and the outputs of P problems whose S has been tridiagonalised
int eigen_tail(const Tail &L, int P, double *wd, size_t per, const int *flag, double *fid_dev, double *parts_dev,
               int *status_dev, hipStream_t s) {
  fid_bounds_kernel<<<P, kThreads, 0, s>>>(L, wd, per, flag);
  DT_LAUNCH_CHECK();
  fid_bisect_kernel<<<dim3((L.m + kWave - 1) / kWave, P), kWave, 0, s>>>(L, wd, per, flag);
  DT_LAUNCH_CHECK();
  fid_finish_kernel<<<P, kThreads, 0, s>>>(L, wd, per, flag, fid_dev, parts_dev, status_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

bool shape_ok(int P, int n_a, int n_b, int D) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_b >= 2 && n_a <= 32768 && n_b <= 32768 &&
         (n_a < n_b ? n_a : n_b) <= DT_FID_MAX_SIDE && D >= 4 && D % 4 == 0 && D <= (1 << 20);
}

// ============================================================================================== the feature-space route
// include/dt_hip_fid_cov.h: for sets with more rows than columns.  Per problem, all in fp64 and every sum in an order that
// (n_a, n_b, D) fixes:
//   c1. column sums over chunks of kMeanChunk rows and the non-finite flag (cov_colsum_kernel); the means (chunk sums in
//       chunk order, one division) and the chunks' sums of squared deviations (cov_coldev_kernel); |mu_A - mu_B|^2 and
//       the traces (cov_stats_kernel);
//   c2. C = A_c^T A_c for both sets: the upper triangle of 64 x 64 tiles on v_mfma_f64_16x16x4_f64, mirrored, rows
//       centred as they are loaded, the rows split into slabs (cov_gram_kernel) that are summed in slab order
//       (cov_slab_sum_kernel);
//   c3. C = L L^T in place, 64-wide panels, a pivot that is not > tol = D 2^-52 max diag C gives a zero column
//       (cov_tol_kernel once; cov_chol_diag_kernel, cov_chol_panel_kernel, cov_chol_update_kernel per panel);
//   c4. N = L_A^T L_B (cov_cross_kernel) and S = N N^T (cov_square_kernel), whose eigenvalues are the squared singular
//       values of A_c B_c^T; then stages 4 and 5 above on side D.
constexpr int kMeanChunk = 1024;
constexpr int kMaxSlabs = 8;

// rows of a set -> slabs of the covariance product: as many as keep the chip busy when the tiles are few, at most
// kMaxSlabs, none shorter than 512 rows; a function of (n, D) only
__host__ __device__ inline int cov_slabs(int n, int D) {
  const int nt = (D + 63) / 64, tiles = nt * (nt + 1) / 2;
  int s = 256 / tiles;
  if (s > kMaxSlabs) s = kMaxSlabs;
  if (s > (n + 511) / 512) s = (n + 511) / 512;
  return s < 1 ? 1 : s;
}

// rows per slab, a multiple of the 16-row stage
__host__ __device__ inline int cov_slab_rows(int n, int slabs) { return ((n + slabs - 1) / slabs + 15) / 16 * 16; }

// per-problem workspace (doubles) of the feature-space route, after the same head of P flags.  S shares C_A's place: the
// factors are dead once N is formed.
struct CovLayout {
  size_t head, per;
  size_t mean, csq, misc, psum, pcsq, C, N, S, slab, v, pv, e, tau, d, lam;
  int nc[2], ns[2];
  __host__ __device__ CovLayout(int P, int n_a, int n_b, int D) {
    head = flag_head_bytes(P);
    const size_t d1 = (size_t)D, d2 = d1 * d1;
    nc[0] = (n_a + kMeanChunk - 1) / kMeanChunk;
    nc[1] = (n_b + kMeanChunk - 1) / kMeanChunk;
    ns[0] = cov_slabs(n_a, D);
    ns[1] = cov_slabs(n_b, D);
    mean = 0;                                   // [2][D]
    csq = mean + 2 * d1;                        // [2][D]
    misc = csq + 2 * d1;
    psum = misc + MISC_COUNT;                   // [nc_a + nc_b][D]
    pcsq = psum + (size_t)(nc[0] + nc[1]) * d1;
    C = pcsq + (size_t)(nc[0] + nc[1]) * d1;    // [2][D][D]
    N = C + 2 * d2;
    S = C;
    slab = N + d2;                              // [ns_a if > 1][D][D], then [ns_b if > 1][D][D]
    v = slab + (size_t)((ns[0] > 1 ? ns[0] : 0) + (ns[1] > 1 ? ns[1] : 0)) * d2;
    pv = v + d1;
    e = pv + d1;
    tau = e + d1;
    d = tau + d1;
    lam = d + d1;
    per = lam + d1;
  }
  __host__ __device__ size_t slab_of(int set, int D) const {
    return slab + (set && ns[0] > 1 ? (size_t)ns[0] * D * D : 0);
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

// ---------------------------------------------------------------------------------------------- c1. means and traces
// grid (quad blocks * chunks, P, set): one thread per quad of columns and chunk of rows, rows in order
__global__ __launch_bounds__(kWave) void cov_colsum_kernel(Rows R, int D, CovLayout L, double *ws, int *flag, int nqb) {
  const int p = blockIdx.y, set = blockIdx.z;
  const int chunk = blockIdx.x / nqb, q = (blockIdx.x % nqb) * kWave + threadIdx.x;
  if (chunk >= L.nc[set] || 4 * q >= D) return;
  const RowSet S = row_set(R, set, p);
  const int r0 = chunk * kMeanChunk, r1 = r0 + kMeanChunk < S.n ? r0 + kMeanChunk : S.n;
  double s0 = 0.0, s1 = 0.0, s2 = 0.0, s3 = 0.0;
  bool bad = false;
  for (int i = r0; i < r1; ++i) {
    const float4 x = reinterpret_cast<const float4 *>(S.row0 + i * S.rs)[q];
    bad |= !(isfinite(x.x) && isfinite(x.y) && isfinite(x.z) && isfinite(x.w));
    s0 += x.x; s1 += x.y; s2 += x.z; s3 += x.w;
  }
  double *o = ws + (size_t)p * L.per + L.psum + (size_t)((set ? L.nc[0] : 0) + chunk) * D + 4 * (size_t)q;
  o[0] = s0; o[1] = s1; o[2] = s2; o[3] = s3;
  if (bad) atomicOr(flag + p, 1);
}

// the same grid: every chunk forms the means of its columns anew (chunk sums in chunk order, one division), chunk 0
// stores them; then its rows' squared deviations
__global__ __launch_bounds__(kWave) void cov_coldev_kernel(Rows R, int D, CovLayout L, double *ws, const int *flag,
                                                           int nqb) {
  const int p = blockIdx.y, set = blockIdx.z;
  const int chunk = blockIdx.x / nqb, q = (blockIdx.x % nqb) * kWave + threadIdx.x;
  if (flag[p] || chunk >= L.nc[set] || 4 * q >= D) return;
  const RowSet S = row_set(R, set, p);
  double *base = ws + (size_t)p * L.per;
  const size_t first = (size_t)(set ? L.nc[0] : 0) * D + 4 * (size_t)q;
  double m[4] = {0.0, 0.0, 0.0, 0.0};
  for (int c = 0; c < L.nc[set]; ++c) {
    const double *ps = base + L.psum + first + (size_t)c * D;
    m[0] += ps[0]; m[1] += ps[1]; m[2] += ps[2]; m[3] += ps[3];
  }
  const double nr = (double)S.n;
  m[0] /= nr; m[1] /= nr; m[2] /= nr; m[3] /= nr;
  const int r0 = chunk * kMeanChunk, r1 = r0 + kMeanChunk < S.n ? r0 + kMeanChunk : S.n;
  double c0 = 0.0, c1 = 0.0, c2 = 0.0, c3 = 0.0;
  for (int i = r0; i < r1; ++i) {
    const float4 x = reinterpret_cast<const float4 *>(S.row0 + i * S.rs)[q];
    const double d0 = (double)x.x - m[0], d1 = (double)x.y - m[1], d2 = (double)x.z - m[2], d3 = (double)x.w - m[3];
    c0 = fma(d0, d0, c0); c1 = fma(d1, d1, c1); c2 = fma(d2, d2, c2); c3 = fma(d3, d3, c3);
  }
  double *o = base + L.pcsq + first + (size_t)chunk * D;
  o[0] = c0; o[1] = c1; o[2] = c2; o[3] = c3;
  if (chunk == 0) {
    double *mo = base + L.mean + (size_t)set * D + 4 * (size_t)q;
    mo[0] = m[0]; mo[1] = m[1]; mo[2] = m[2]; mo[3] = m[3];
  }
}

__global__ __launch_bounds__(kThreads) void cov_stats_kernel(int n_a, int n_b, int D, CovLayout L, double *ws,
                                                             const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (flag[p]) return;
  double *base = ws + (size_t)p * L.per;
  const double *ma = base + L.mean, *mb = ma + D;
  double s = 0.0, ta = 0.0, tb = 0.0;
  for (int e = threadIdx.x; e < D; e += kThreads) {
    const double d = ma[e] - mb[e];
    s = fma(d, d, s);
    double ca = 0.0, cb = 0.0;
    for (int c = 0; c < L.nc[0]; ++c) ca += base[L.pcsq + (size_t)c * D + e];
    for (int c = 0; c < L.nc[1]; ++c) cb += base[L.pcsq + (size_t)(L.nc[0] + c) * D + e];
    ta += ca;
    tb += cb;
  }
  const double dmu2 = block_sum(s, red), sa = block_sum(ta, red), sb = block_sum(tb, red);
  if (threadIdx.x == 0) {
    double *misc = base + L.misc;
    misc[MISC_DMU2] = dmu2;
    misc[MISC_TRA] = sa / (double)(n_a - 1);
    misc[MISC_TRB] = sb / (double)(n_b - 1);
  }
}

// ---------------------------------------------------------------------------------------------- c2. C = A_c^T A_c
// grid (upper tiles * slabs, P, set).  The contraction runs over the rows: thread t stages the float4 of columns
// 4 (t % 16) .. + 3 of row t / 16 of the stage for both tile columns, centred, so a wave reads four rows of 256
// contiguous bytes.  Wave w owns output rows 16 w .. 16 w + 15 of the tile as four 16 x 16 blocks; per four rows of the
// stage lane l takes A[k = l / 16][row l % 16] and B[k = l / 16][col l % 16] and the instruction adds the four products
// of every output to its accumulator, which lies at column l % 16, rows l / 16 + 4 i of the block.  Every output of
// every tile runs through the same sequence of instructions on a_k,i a_k,j, and the product commutes, so C[i][j] and
// C[j][i] of a diagonal tile are the same bits.  The same tile on plain fp64 FMAs (the inner loop of tile_product) was
// measured beside this one and dropped: 1.5 times slower at D = 2048.  mfma_acc: dt_dense64.h.
__global__ __launch_bounds__(kThreads) void cov_gram_kernel(Rows R, int D, CovLayout L, double *ws, const int *flag,
                                                            int nt, int tiles) {
  __shared__ double As[16][64], Bs[16][64];
  const int p = blockIdx.y, set = blockIdx.z;
  const int slab = blockIdx.x / tiles, slabs = L.ns[set];
  if (flag[p] || slab >= slabs) return;
  int bi, bj;
  upper_tile(blockIdx.x % tiles, nt, bi, bj);
  const RowSet S = row_set(R, set, p);
  const int rows = cov_slab_rows(S.n, slabs);
  const int r0 = slab * rows, r1 = r0 + rows < S.n ? r0 + rows : S.n;
  double *base = ws + (size_t)p * L.per;
  const int t = threadIdx.x, kr = t / 16, cq = 4 * (t % 16);
  const int ca = bi * 64 + cq, cb = bj * 64 + cq;
  const double *mean = base + L.mean + (size_t)set * D;
  double ma[4] = {0.0, 0.0, 0.0, 0.0}, mb[4] = {0.0, 0.0, 0.0, 0.0};
  if (ca < D) { ma[0] = mean[ca]; ma[1] = mean[ca + 1]; ma[2] = mean[ca + 2]; ma[3] = mean[ca + 3]; }
  if (cb < D) { mb[0] = mean[cb]; mb[1] = mean[cb + 1]; mb[2] = mean[cb + 2]; mb[3] = mean[cb + 3]; }
  const int w = t / 64, lane = t % 64, lk = lane / 16, lc = lane % 16;
  mfma_acc acc[4] = {};
  for (int k0 = r0; k0 < r1; k0 += 16) {
    const int row = k0 + kr;
    double va[4] = {0.0, 0.0, 0.0, 0.0}, vb[4] = {0.0, 0.0, 0.0, 0.0};
    if (row < r1) {
      const float *src = S.row0 + row * S.rs;
      if (ca < D) {
        const float4 x = *reinterpret_cast<const float4 *>(src + ca);
        va[0] = (double)x.x - ma[0]; va[1] = (double)x.y - ma[1]; va[2] = (double)x.z - ma[2]; va[3] = (double)x.w - ma[3];
      }
      if (cb < D) {
        const float4 x = *reinterpret_cast<const float4 *>(src + cb);
        vb[0] = (double)x.x - mb[0]; vb[1] = (double)x.y - mb[1]; vb[2] = (double)x.z - mb[2]; vb[3] = (double)x.w - mb[3];
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { As[kr][cq + i] = va[i]; Bs[kr][cq + i] = vb[i]; }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {
      const double a = As[kk + lk][16 * w + lc];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(a, Bs[kk + lk][16 * j + lc], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
  double *C = base + (slabs > 1 ? L.slab_of(set, D) + (size_t)slab * D * D : L.C + (size_t)set * D * D);
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = bi * 64 + 16 * w + lk + 4 * i, c = bj * 64 + 16 * j + lc;
      if (r < D && c < D) {
        C[(size_t)r * D + c] = acc[j][i];
        if (bi != bj) C[(size_t)c * D + r] = acc[j][i];
      }
    }
}

// C = slab 0 + slab 1 + ... in that order; grid (blocks over D * D, P, set), sets with one slab were written in place
__global__ __launch_bounds__(kThreads) void cov_slab_sum_kernel(int D, CovLayout L, double *ws, const int *flag) {
  const int p = blockIdx.y, set = blockIdx.z;
  if (flag[p] || L.ns[set] < 2) return;
  const size_t d2 = (size_t)D * D, i = (size_t)blockIdx.x * kThreads + threadIdx.x;
  if (i >= d2) return;
  double *base = ws + (size_t)p * L.per;
  const double *sl = base + L.slab_of(set, D) + i;
  double s = sl[0];
  for (int k = 1; k < L.ns[set]; ++k) s += sl[(size_t)k * d2];
  base[L.C + (size_t)set * d2 + i] = s;
}

// ---------------------------------------------------------------------------------------------- c3. C = L L^T
// tol = D 2^-52 max_i C[i][i]; grid (P, set)
__global__ __launch_bounds__(kThreads) void cov_tol_kernel(int D, CovLayout L, double *ws, const int *flag) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x, set = blockIdx.y;
  if (flag[p]) return;
  double *base = ws + (size_t)p * L.per;
  const double *C = base + L.C + (size_t)set * D * D;
  double mx = 0.0;
  for (int i = threadIdx.x; i < D; i += kThreads) mx = fmax(mx, C[(size_t)i * D + i]);
  mx = block_max(mx, red);
  if (threadIdx.x == 0) base[L.misc + MISC_TOL + set] = (double)D * DBL_EPSILON * mx;
}

// The diagonal block of panel j0 (w columns), factored in LDS by one workgroup: column by column, a pivot that is not
// > tol leaves a zero column and divides nothing.  Written back lower-triangular with zeros above.  grid (1, P, set)
__global__ __launch_bounds__(kThreads) void cov_chol_diag_kernel(int D, CovLayout L, double *ws, const int *flag, int j0,
                                                                 int w) {
  __shared__ double T[64][65];
  const int p = blockIdx.y, set = blockIdx.z, t = threadIdx.x;
  if (flag[p]) return;
  double *base = ws + (size_t)p * L.per;
  double *C = base + L.C + (size_t)set * D * D;
  const double tol = base[L.misc + MISC_TOL + set];
  for (int q = t; q < 64 * 64; q += kThreads) {
    const int r = q / 64, c = q % 64;
    T[r][c] = r < w && c < w ? C[(size_t)(j0 + r) * D + j0 + c] : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < w; ++c) {
    const double piv = T[c][c];
    const bool ok = piv > tol;
    const double d = ok ? sqrt(piv) : 0.0;
    __syncthreads();
    if (t >= c && t < 64) T[t][c] = t == c ? d : (ok ? T[t][c] / d : 0.0);
    __syncthreads();
    if (ok)
      for (int q = t; q < 64 * 64; q += kThreads) {
        const int r = q / 64, cc = q % 64;
        if (cc > c && r >= cc && r < w) T[r][cc] = fma(-T[r][c], T[cc][c], T[r][cc]);
      }
    __syncthreads();
  }
  for (int q = t; q < 64 * 64; q += kThreads) {
    const int r = q / 64, c = q % 64;
    if (r < w && c < w) C[(size_t)(j0 + r) * D + j0 + c] = c <= r ? T[r][c] : 0.0;
  }
}

// The panel below the diagonal block: rows i of it solve x L_d^T = C[i][j0 .. j0 + w), 32 rows per workgroup in LDS,
// column by column: x_c takes its pivot's reciprocal (0 for a dropped pivot, so x_c = 0), then leaves the columns after
// it.  Writes L[i][j0 ..] and zeroes the mirror entries above the diagonal, which nothing reads again before N.
// grid (row blocks of 32, P, set)
__global__ __launch_bounds__(kThreads) void cov_chol_panel_kernel(int D, CovLayout L, double *ws, const int *flag, int j0,
                                                                  int w) {
  __shared__ double LT[64][64], X[32][64], dinv[64];
  const int p = blockIdx.y, set = blockIdx.z, t = threadIdx.x;
  if (flag[p]) return;
  double *C = ws + (size_t)p * L.per + L.C + (size_t)set * D * D;
  const int i0 = j0 + w + blockIdx.x * 32;
  for (int q = t; q < 64 * 64; q += kThreads) {
    const int r = q / 64, c = q % 64;
    LT[c][r] = r < w && c < r ? C[(size_t)(j0 + r) * D + j0 + c] : 0.0;
  }
  if (t < 64) {
    const double dd = t < w ? C[(size_t)(j0 + t) * D + j0 + t] : 0.0;
    dinv[t] = dd > 0.0 ? 1.0 / dd : 0.0;
  }
  for (int q = t; q < 32 * 64; q += kThreads) {
    const int r = q / 64, c = q % 64;
    X[r][c] = i0 + r < D && c < w ? C[(size_t)(i0 + r) * D + j0 + c] : 0.0;
  }
  __syncthreads();
  for (int c = 0; c < w; ++c) {
    if (t < 32) X[t][c] *= dinv[c];
    __syncthreads();
    for (int q = t; q < 32 * 64; q += kThreads) {
      const int r = q / 64, cc = q % 64;
      if (cc > c) X[r][cc] = fma(-X[r][c], LT[c][cc], X[r][cc]);
    }
    __syncthreads();
  }
  for (int q = t; q < 32 * 64; q += kThreads) {
    const int r = q / 64, c = q % 64;
    if (i0 + r < D && c < w) C[(size_t)(i0 + r) * D + j0 + c] = X[r][c];
  }
  for (int q = t; q < 32 * 64; q += kThreads) {
    const int c = q / 32, r = q % 32;
    if (i0 + r < D && c < w) C[(size_t)(j0 + c) * D + i0 + r] = 0.0;
  }
}

// Loader for tile_product: entries k .. k+3 of the 64 panel columns of one row of L (nullptr: no such row)
struct PanelRow {
  const double *row;
  static constexpr int W = 4;
  __device__ void operator()(int k, double (&v)[4]) const {
    v[0] = v[1] = v[2] = v[3] = 0.0;
    if (row && k < 64) { v[0] = row[k]; v[1] = row[k + 1]; v[2] = row[k + 2]; v[3] = row[k + 3]; }
  }
};

// C[i][j] -= sum_k L[i][j0 + k] L[j][j0 + k] on the tiles bi >= bj past a full panel: the lower triangle is what the
// later panels read, and a diagonal tile stays exactly symmetric.  grid (lower tiles, P, set)
__global__ __launch_bounds__(kThreads) void cov_chol_update_kernel(int D, CovLayout L, double *ws, const int *flag,
                                                                   int j0, int ntr) {
  const int p = blockIdx.y, set = blockIdx.z;
  if (flag[p]) return;
  int u, v;
  upper_tile(blockIdx.x, ntr, u, v);
  const int bi = j0 / 64 + 1 + v, bj = j0 / 64 + 1 + u;
  double *C = ws + (size_t)p * L.per + L.C + (size_t)set * D * D;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  double acc[4][4] = {};
  tile_product(64, lr, lq, PanelRow{ra < D ? C + (size_t)ra * D + j0 : nullptr},
               PanelRow{rb < D ? C + (size_t)rb * D + j0 : nullptr}, acc);
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
#pragma unroll
  for (int a = 0; a < 4; ++a)
#pragma unroll
    for (int b = 0; b < 4; ++b) {
      const int r = bi * 64 + ty + 16 * a, c = bj * 64 + tx + 16 * b;
      if (r < D && c < D) C[(size_t)r * D + c] -= acc[a][b];
    }
}

// ---------------------------------------------------------------------------------------------- c4. N and N N^T
// N[i][j] = sum_k L_A[k][i] L_B[k][j]: both factors are lower-triangular, so the k below the later tile's first row add
// exact zeros and are skipped.  grid (tiles, P)
__global__ __launch_bounds__(kThreads) void cov_cross_kernel(int D, CovLayout L, double *ws, const int *flag, int nt) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const int bi = blockIdx.x / nt, bj = blockIdx.x % nt;
  double *base = ws + (size_t)p * L.per;
  const int t = threadIdx.x, lr = t % 64, lq = t / 64;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  const int k0 = 64 * (bi > bj ? bi : bj);
  const double *LA = base + L.C + (size_t)k0 * D, *LB = LA + (size_t)D * D;
  double acc[4][4] = {};
  tile_product(D - k0, lr, lq, FactorRow<true>{LA, D, D - k0, ra, ra < D}, FactorRow<true>{LB, D, D - k0, rb, rb < D}, acc);
  store_tile<false>(base + L.N, D, D, bi, bj, acc);
}

__global__ __launch_bounds__(kThreads) void cov_square_kernel(int D, CovLayout L, double *ws, const int *flag, int nt) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  int bi, bj;
  upper_tile(blockIdx.x, nt, bi, bj);
  double *base = ws + (size_t)p * L.per;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  double acc[4][4] = {};
  tile_product(D, lr, lq, FactorRow<false>{base + L.N, D, D, ra, ra < D}, FactorRow<false>{base + L.N, D, D, rb, rb < D},
               acc);
  store_tile<true>(base + L.S, D, D, bi, bj, acc);
}

bool cov_shape_ok(int P, int n_a, int n_b, int D) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_b >= 2 && n_a <= DT_FID_COV_MAX_ROWS && n_b <= DT_FID_COV_MAX_ROWS &&
         D >= 4 && D % 4 == 0 && D <= DT_FID_COV_MAX_WIDTH;
}
static_assert(DT_FID_COV_MAX_WIDTH <= DT_FID_MAX_SIDE, "the LDS arrays of stages 4 and 5 hold DT_FID_MAX_SIDE entries");

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
  if (!shape_ok(P, n_a, n_b, D)) return DT_E_SHAPE;
  const Layout L(P, n_a, n_b, D);
  const auto [rc, R, flag, wd] = set_pair_open(a_dev, n_a, a_pstride, a_rstride, b_dev, n_b, b_pstride, b_rstride, ws,
                                               ws_bytes, L.bytes(P), L.head);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
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
  if (const int rc = eigen_tail(Tail{L.misc, L.S, L.d, L.e, L.lam, m, n_a, n_b}, P, wd, L.per, flag, fid_dev, parts_dev,
                                status_dev, s))
    return rc;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[4], s));
  return DT_OK;
}

extern "C" size_t dt_fid_cov_workspace_bytes(int P, int n_a, int n_b, int D) {
  if (!cov_shape_ok(P, n_a, n_b, D)) return 0;
  return CovLayout(P, n_a, n_b, D).bytes(P);   // < 2^47: 65535 problems of fewer than 2^28 doubles
}

extern "C" int dt_fid_cov_distance(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                                   const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P, int D,
                                   double *fid_dev, double *parts_dev, int *status_dev, void *ws, size_t ws_bytes,
                                   void *const *events, void *stream) {
  if (!a_dev || !b_dev || !fid_dev || !parts_dev || !status_dev || !ws) return DT_E_NULL;
  if (!cov_shape_ok(P, n_a, n_b, D)) return DT_E_SHAPE;
  const CovLayout L(P, n_a, n_b, D);
  const auto [rc, R, flag, wd] = set_pair_open(a_dev, n_a, a_pstride, a_rstride, b_dev, n_b, b_pstride, b_rstride, ws,
                                               ws_bytes, L.bytes(P), L.head);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  DT_HIP_TRY(hipMemsetAsync(ws, 0, L.head, s));
  const int nqb = (D / 4 + kWave - 1) / kWave, ncmax = L.nc[0] > L.nc[1] ? L.nc[0] : L.nc[1];
  cov_colsum_kernel<<<dim3(nqb * ncmax, P, 2), kWave, 0, s>>>(R, D, L, wd, flag, nqb);
  DT_LAUNCH_CHECK();
  cov_coldev_kernel<<<dim3(nqb * ncmax, P, 2), kWave, 0, s>>>(R, D, L, wd, flag, nqb);
  DT_LAUNCH_CHECK();
  cov_stats_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, D, L, wd, flag);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[1], s));
  const int nt = (D + 63) / 64, tiles = nt * (nt + 1) / 2, nsmax = L.ns[0] > L.ns[1] ? L.ns[0] : L.ns[1];
  cov_gram_kernel<<<dim3(tiles * nsmax, P, 2), kThreads, 0, s>>>(R, D, L, wd, flag, nt, tiles);
  DT_LAUNCH_CHECK();
  if (nsmax > 1) {
    cov_slab_sum_kernel<<<dim3((unsigned)(((size_t)D * D + kThreads - 1) / kThreads), P, 2), kThreads, 0, s>>>(D, L, wd, flag);
    DT_LAUNCH_CHECK();
  }
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[2], s));
  cov_tol_kernel<<<dim3(P, 2), kThreads, 0, s>>>(D, L, wd, flag);
  DT_LAUNCH_CHECK();
  for (int j0 = 0; j0 < D; j0 += 64) {
    const int w = D - j0 < 64 ? D - j0 : 64, below = D - j0 - w;
    cov_chol_diag_kernel<<<dim3(1, P, 2), kThreads, 0, s>>>(D, L, wd, flag, j0, w);
    DT_LAUNCH_CHECK();
    if (below > 0) {
      const int ntr = nt - (j0 / 64 + 1);
      cov_chol_panel_kernel<<<dim3((below + 31) / 32, P, 2), kThreads, 0, s>>>(D, L, wd, flag, j0, w);
      DT_LAUNCH_CHECK();
      cov_chol_update_kernel<<<dim3(ntr * (ntr + 1) / 2, P, 2), kThreads, 0, s>>>(D, L, wd, flag, j0, ntr);
      DT_LAUNCH_CHECK();
    }
  }
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[3], s));
  cov_cross_kernel<<<dim3(nt * nt, P), kThreads, 0, s>>>(D, L, wd, flag, nt);
  DT_LAUNCH_CHECK();
  cov_square_kernel<<<dim3(tiles, P), kThreads, 0, s>>>(D, L, wd, flag, nt);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[4], s));
  const Tri T{wd, L.per, L.S, L.v, L.pv, L.e, L.tau, flag, D};
  if (const int rc = tridiagonalise(T, P, s)) return rc;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[5], s));
  if (const int rc = eigen_tail(Tail{L.misc, L.S, L.d, L.e, L.lam, D, n_a, n_b}, P, wd, L.per, flag, fid_dev, parts_dev,
                                status_dev, s))
    return rc;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[6], s));
  return DT_OK;
}
