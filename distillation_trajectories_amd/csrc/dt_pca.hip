// Exact, deterministic PCA of a batch of independent problems (include/dt_hip_pca.h): the dimensionality analysis of
// analysis/dimensionality/ on the device.
//
// Stages, per problem (every output element summed in a fixed order, so a result does not depend on P or on the other
// problems of the launch):
//   1. column means in fp64 and the non-finite flag (pca_mean_kernel);
//   2. the centred Gram matrix G = Xc Xc^T in fp64, upper-triangle 64 x 64 tiles mirrored into full symmetric storage
//      (pca_gram_kernel); centring before the product keeps the large common component of a trajectory's states from
//      cancelling; trace(G) and the status word (pca_status_kernel);
//   3. Householder tridiagonalisation (unblocked, dsytd2-like, lower): one reflector, one matrix-vector product and one
//      symmetric rank-2 update per column, each a launch spread over the chip (the n x n fp64 matrix lives in the
//      workspace: it does not fit in LDS from n ~ 140 up); then, one workgroup per problem (pca_eigen_kernel), bisection
//      with Sturm counts for the k largest eigenvalues, inverse iteration for their vectors (dstein-like: clusters
//      re-orthogonalised) and the back-transformation through the stored reflectors; a lambda_j within n eps ||T|| of
//      zero is a null direction and is set to 0 there, which makes stage 4 write zeros for it;
//   4. components v = Xc^T u / s (pca_components_kernel), then the sign rule of sklearn's svd_flip(u_based_decision=False),
//      scores s * u and the variances (pca_finish_kernel).
#include <float.h>
#include <math.h>

#include "../../include/dt_hip_pca.h"
#include "dt_internal.h"
#include "dt_dense64.h"

namespace {

// per-problem workspace (doubles), after a head of 2 * P ints (non-finite flag, status) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t mean, G, v, pv, d, e, tau, lam, misc, Z, lu, V;
  __host__ __device__ Layout(int P, int n, int E, int k) {
    head = flag_head_bytes(2 * P);
    const size_t N = (size_t)n;
    mean = 0;
    G = mean + (size_t)E;
    v = G + N * N;
    pv = v + N;
    d = pv + N;
    e = d + N;
    tau = e + N;
    lam = tau + N;
    misc = lam + DT_PCA_MAX_K;
    Z = misc + 16;
    lu = Z + (size_t)k * N;
    V = lu + 5 * N;
    per = V + (size_t)k * E;
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

// ---------------------------------------------------------------------------------------------- 1. mean and check
__global__ __launch_bounds__(kThreads) void pca_mean_kernel(Rows R, int E, double *ws, size_t per, int *flag,
                                                            float *mean_out) {
  const int p = blockIdx.y;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (4 * q >= E) return;
  double m[4];
  const bool bad = quad_mean(R, p, 0, 1, q, m);
  double *out = ws + (size_t)p * per + 4 * (size_t)q;
  out[0] = m[0]; out[1] = m[1]; out[2] = m[2]; out[3] = m[3];
  reinterpret_cast<float4 *>(mean_out + (size_t)p * E)[q] = make_float4((float)m[0], (float)m[1], (float)m[2], (float)m[3]);
  if (bad) atomicOr(flag + p, 1);
}

// ---------------------------------------------------------------------------------------------- 2. centred Gram
// G = Xc Xc^T over the upper triangle of 64 x 64 tiles (tile_product, dt_dense64.h), rows centred as they are loaded
__global__ __launch_bounds__(kThreads) void pca_gram_kernel(Rows R, int E, double *ws, size_t per, const int *flag,
                                                            int nt) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  int bi, bj;
  upper_tile(blockIdx.x, nt, bi, bj);
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int n = R.n_a + R.n_b;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  const double *mean = ws + (size_t)p * per;
  double acc[4][4] = {};
  tile_product(E, lr, lq, CentredRow{ra < n ? row_ptr(R, p, ra) : nullptr, mean, E},
               CentredRow{rb < n ? row_ptr(R, p, rb) : nullptr, mean, E}, acc);
  store_tile<true>(ws + (size_t)p * per + E, n, n, bi, bj, acc);
}

// trace(G) and the status word: non-finite input, then zero total variance
__global__ __launch_bounds__(kThreads) void pca_status_kernel(int n, int E, int k, double *ws, size_t per,
                                                              const int *flag, int *st, int *status_out) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  const double *G = ws + (size_t)p * per + E;
  double s = 0.0;
  for (int i = threadIdx.x; i < n; i += kThreads) s += G[(size_t)i * n + i];
  const double tr = block_sum(s, red);
  if (threadIdx.x == 0) {
    const int code = (flag[p] || !isfinite(tr)) ? DT_PCA_NONFINITE : (tr == 0.0 ? DT_PCA_ZERO_VARIANCE : DT_PCA_OK);
    st[p] = code;
    status_out[p] = code;
    ws[(size_t)p * per + Layout(0, n, E, k).misc] = tr;
  }
}

// ---------------------------------------------------------------------------------------------- 3. eigen stage
// The tridiagonalisation kernels, the spectrum bounds and the bisection are in dt_dense64.h (shared with dt_fid.hip).

__device__ inline double start_entry(int i, int j) {
  unsigned h = (unsigned)i * 2654435761u ^ ((unsigned)j + 1u) * 40503u;
  h ^= h >> 15; h *= 2246822519u; h ^= h >> 13; h *= 3266489917u; h ^= h >> 16;
  return (double)(h & 0xffffffu) / 8388608.0 - 1.0;
}

// One workgroup per problem: bisection for the k largest eigenvalues of the tridiagonal, inverse iteration for their
// vectors, back-transformation through the reflectors.  Z [k][n] receives the eigenvectors u of G.
__global__ __launch_bounds__(kThreads) void pca_eigen_kernel(int n, int E, int k, double *ws, size_t per,
                                                             const int *st) {
  __shared__ double red[kThreads];
  const int p = blockIdx.x;
  if (st[p]) return;
  const Layout L(0, n, E, k);
  double *base = ws + (size_t)p * per;
  const double *A = base + L.G;
  double *d = base + L.d, *e = base + L.e, *lam = base + L.lam, *Z = base + L.Z;
  const int t = threadIdx.x;
  double onenrm;
  const Spectrum sp = tridiagonal_spectrum(A, n, d, e, red, &onenrm);
  const double tnorm = sp.tnorm;
  if (t < k) lam[t] = bisect_eigenvalue(d, e, n, n - 1 - t, sp);      // lambda_j is eigenvalue n-1-j in ascending order
  __syncthreads();

  // inverse iteration (dstein-like), one thread: LU with partial pivoting of T - x I, five solves per vector, each
  // followed by Gram-Schmidt against the earlier vectors of its cluster (eigenvalues within 1e-3 ||T||_1) and a
  // normalisation
  if (t == 0) {
    double *dd = base + L.lu, *du1 = dd + n, *du2 = du1 + n, *lm = du2 + n, *piv = lm + n;
    const double ortol = 1e-3 * onenrm, tiny = DBL_EPSILON * tnorm;
    int first = 0;
    double xprev = 0.0;
    for (int j = 0; j < k; ++j) {
      double x = lam[j];
      if (j > 0) {
        if (xprev - x > ortol) {
          first = j;
        } else {
          const double pertol = 10.0 * DBL_EPSILON * fmax(fabs(x), tnorm * DBL_EPSILON);
          if (xprev - x < pertol) x = xprev - pertol;
        }
      }
      for (int i = 0; i < n; ++i) {
        dd[i] = d[i] - x;
        du1[i] = i < n - 1 ? e[i] : 0.0;
        du2[i] = 0.0;
      }
      for (int i = 0; i < n - 1; ++i) {
        const double b = e[i];
        if (fabs(dd[i]) >= fabs(b)) {
          piv[i] = 0.0;
          if (dd[i] == 0.0) dd[i] = tiny;
          lm[i] = b / dd[i];
          dd[i + 1] -= lm[i] * du1[i];
        } else {
          piv[i] = 1.0;
          lm[i] = dd[i] / b;
          dd[i] = b;
          const double u = du1[i];
          du1[i] = dd[i + 1];
          dd[i + 1] = u - lm[i] * dd[i + 1];
          if (i + 1 < n - 1) {
            du2[i] = du1[i + 1];
            du1[i + 1] = -lm[i] * du2[i];
          }
        }
      }
      for (int i = 0; i < n; ++i)
        if (fabs(dd[i]) < tiny) dd[i] = dd[i] < 0.0 ? -tiny : tiny;
      double *z = Z + (size_t)j * n;
      for (int i = 0; i < n; ++i) z[i] = start_entry(i, j);
      for (int it = 0; it < 5; ++it) {
        for (int i = 0; i < n - 1; ++i) {
          if (piv[i] != 0.0) { const double u = z[i]; z[i] = z[i + 1]; z[i + 1] = u; }
          z[i + 1] -= lm[i] * z[i];
        }
        z[n - 1] /= dd[n - 1];
        z[n - 2] = (z[n - 2] - du1[n - 2] * z[n - 1]) / dd[n - 2];
        for (int i = n - 3; i >= 0; --i) z[i] = (z[i] - du1[i] * z[i + 1] - du2[i] * z[i + 2]) / dd[i];
        for (int jj = first; jj < j; ++jj) {
          const double *y = Z + (size_t)jj * n;
          double s = 0.0;
          for (int i = 0; i < n; ++i) s = fma(z[i], y[i], s);
          for (int i = 0; i < n; ++i) z[i] -= s * y[i];
        }
        double s = 0.0, amax = 0.0;
        for (int i = 0; i < n; ++i) amax = fmax(amax, fabs(z[i]));
        if (amax == 0.0) {                       // annihilated by the re-orthogonalisation: start again elsewhere
          for (int i = 0; i < n; ++i) z[i] = start_entry(i, j + 7919 * (it + 1));
          continue;
        }
        for (int i = 0; i < n; ++i) { z[i] /= amax; s = fma(z[i], z[i], s); }
        s = 1.0 / sqrt(s);
        for (int i = 0; i < n; ++i) z[i] *= s;
      }
      xprev = x;
    }
  }
  __syncthreads();

  // Null directions.  This stage resolves lambda no finer than the n eps ||T|| it widens its own Gershgorin interval by: a
  // lambda_j at or below that is rounding noise of either sign, and its sign must not decide the output.  lambda_j = 0
  // makes the components and the finish kernel write zeros for the direction (singular value, variance, ratio, component,
  // score column), as DT_PCA_ZERO_VARIANCE does for a whole problem.
  if (t < k && lam[t] <= n * DBL_EPSILON * tnorm) lam[t] = 0.0;

  // back-transformation u = H_0 ... H_{n-3} z: one wave per vector; lane l owns rows r = l (mod 64) throughout
  const int w = t / 64, lane = t % 64;
  const double *tau = base + L.tau;
  for (int j = w; j < k; j += kThreads / 64) {
    double *z = Z + (size_t)j * n;
    for (int i = n - 3; i >= 0; --i) {
      const double ti = tau[i];
      if (ti == 0.0) continue;
      const double *vr = A + (size_t)i * n;
      double s = 0.0;
      for (int r = lane; r < n; r += 64)
        if (r > i) s = fma(r == i + 1 ? 1.0 : vr[r], z[r], s);
      const double f = ti * wave_sum(s);
      for (int r = lane; r < n; r += 64)
        if (r > i) z[r] -= f * (r == i + 1 ? 1.0 : vr[r]);
    }
  }
}

// ---------------------------------------------------------------------------------------------- 4. components, signs
// V[j][e] = sum_i (x_i[e] - mean[e]) u_j[i] / s_j, one thread per column, rows in order
__global__ __launch_bounds__(kThreads) void pca_components_kernel(Rows R, int E, int k, double *ws, size_t per,
                                                                  const int *st) {
  __shared__ double Us[DT_PCA_MAX_K][64];
  const int p = blockIdx.y;
  if (st[p]) return;
  const int n = R.n_a + R.n_b;
  const Layout L(0, n, E, k);
  double *base = ws + (size_t)p * per;
  const int e = blockIdx.x * kThreads + threadIdx.x;
  const double mu = e < E ? base[L.mean + e] : 0.0;
  double acc[DT_PCA_MAX_K];
#pragma unroll
  for (int j = 0; j < DT_PCA_MAX_K; ++j) acc[j] = 0.0;
  for (int i0 = 0; i0 < n; i0 += 64) {
    for (int q = threadIdx.x; q < k * 64; q += kThreads) {
      const int j = q / 64, ii = i0 + q % 64;
      Us[j][q % 64] = ii < n ? base[L.Z + (size_t)j * n + ii] : 0.0;
    }
    __syncthreads();
    if (e < E) {
      const int cnt = min(64, n - i0);
      for (int ii = 0; ii < cnt; ++ii) {
        const double x = (double)row_ptr(R, p, i0 + ii)[e] - mu;
#pragma unroll
        for (int j = 0; j < DT_PCA_MAX_K; ++j)
          if (j < k) acc[j] = fma(x, Us[j][ii], acc[j]);
      }
    }
    __syncthreads();
  }
  if (e < E) {
#pragma unroll
    for (int j = 0; j < DT_PCA_MAX_K; ++j)
      if (j < k) {
        const double s = sqrt(fmax(base[L.lam + j], 0.0));
        base[L.V + (size_t)j * E + e] = s > 0.0 ? acc[j] / s : 0.0;
      }
  }
}

// signs (largest |entry| of each component made positive, first index on ties), fp32 components and scores, variances
__global__ __launch_bounds__(kThreads) void pca_finish_kernel(int n, int E, int k, double *ws, size_t per, const int *st,
                                                              float *mean_out, float *comp_out, float *scores_out,
                                                              double *sv_out, double *var_out, double *ratio_out) {
  __shared__ double rv[kThreads];
  __shared__ int ri[kThreads];
  const int p = blockIdx.x, t = threadIdx.x;
  const Layout L(0, n, E, k);
  const double *base = ws + (size_t)p * per;
  float *comp = comp_out + (size_t)p * k * E, *scores = scores_out + (size_t)p * n * k;
  const int code = st[p];
  if (code != DT_PCA_OK) {
    const float fill = code == DT_PCA_NONFINITE ? NAN : 0.0f;
    if (code == DT_PCA_NONFINITE)
      for (int e = t; e < E; e += kThreads) mean_out[(size_t)p * E + e] = NAN;
    for (size_t q = t; q < (size_t)k * E; q += kThreads) comp[q] = fill;
    for (size_t q = t; q < (size_t)n * k; q += kThreads) scores[q] = fill;
    if (t < k) {
      sv_out[(size_t)p * k + t] = code == DT_PCA_NONFINITE ? NAN : 0.0;
      var_out[(size_t)p * k + t] = code == DT_PCA_NONFINITE ? NAN : 0.0;
      ratio_out[(size_t)p * k + t] = NAN;
    }
    return;
  }
  const double trace = base[L.misc];
  for (int j = 0; j < k; ++j) {
    const double *V = base + L.V + (size_t)j * E;
    double best = -1.0;
    int bi = 0;
    for (int e = t; e < E; e += kThreads) {
      const double a = fabs(V[e]);
      if (a > best) { best = a; bi = e; }
    }
    rv[t] = best;
    ri[t] = bi;
    __syncthreads();
    for (int h = kThreads / 2; h >= 1; h >>= 1) {
      if (t < h && (rv[t + h] > rv[t] || (rv[t + h] == rv[t] && ri[t + h] < ri[t]))) {
        rv[t] = rv[t + h];
        ri[t] = ri[t + h];
      }
      __syncthreads();
    }
    const double sign = V[ri[0]] < 0.0 ? -1.0 : 1.0;
    __syncthreads();
    for (int e = t; e < E; e += kThreads) comp[(size_t)j * E + e] = (float)(sign * V[e]);
    const double lj = fmax(base[L.lam + j], 0.0), s = sqrt(lj);
    const double *u = base + L.Z + (size_t)j * n;
    for (int i = t; i < n; i += kThreads) scores[(size_t)i * k + j] = s > 0.0 ? (float)(sign * s * u[i]) : 0.0f;
    if (t == 0) {
      sv_out[(size_t)p * k + j] = s;
      var_out[(size_t)p * k + j] = lj / (n - 1);
      ratio_out[(size_t)p * k + j] = lj / trace;
    }
  }
}

// ---------------------------------------------------------------------------------------------- projection
// one wave per row: lanes over float4 quads in order, then a butterfly per component
__global__ __launch_bounds__(kThreads) void pca_project_kernel(Rows R, int E, int k, const float *mean,
                                                               long long mean_ps, const float *comp, long long comp_ps,
                                                               float *scores) {
  const int p = blockIdx.y, w = threadIdx.x / 64, lane = threadIdx.x % 64;
  const int r = blockIdx.x * (kThreads / 64) + w;
  if (r >= R.n_a + R.n_b) return;
  const float4 *x = reinterpret_cast<const float4 *>(row_ptr(R, p, r));
  const float4 *m = reinterpret_cast<const float4 *>(mean + p * mean_ps);
  const float *cb = comp + p * comp_ps;
  const int E4 = E / 4;
  double acc[DT_PCA_MAX_K];
#pragma unroll
  for (int j = 0; j < DT_PCA_MAX_K; ++j) acc[j] = 0.0;
  for (int q = lane; q < E4; q += 64) {
    const float4 xv = x[q], mv = m[q];
    const double d0 = (double)xv.x - mv.x, d1 = (double)xv.y - mv.y, d2 = (double)xv.z - mv.z, d3 = (double)xv.w - mv.w;
#pragma unroll
    for (int j = 0; j < DT_PCA_MAX_K; ++j)
      if (j < k) {
        const float4 c = reinterpret_cast<const float4 *>(cb + (size_t)j * E)[q];
        acc[j] = fma(d3, (double)c.w, fma(d2, (double)c.z, fma(d1, (double)c.y, fma(d0, (double)c.x, acc[j]))));
      }
  }
#pragma unroll
  for (int j = 0; j < DT_PCA_MAX_K; ++j)
    if (j < k) {
      const double s = wave_sum(acc[j]);
      if (lane == 0) scores[((size_t)p * (R.n_a + R.n_b) + r) * k + j] = (float)s;
    }
}

bool fit_shape_ok(int P, int n, int E, int k) {
  return P >= 1 && P <= 65535 && n >= 2 && n <= 32768 && E >= 4 && E % 4 == 0 && E <= (1 << 28) && k >= 1 &&
         k <= DT_PCA_MAX_K && k <= n - 1 && k <= E;
}

}  // namespace

extern "C" size_t dt_pca_workspace_bytes(int P, int n, int E, int k) {
  if (!fit_shape_ok(P, n, E, k)) return 0;
  return Layout(P, n, E, k).bytes(P);
}

extern "C" int dt_pca_fit(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev,
                          int n_b, long long b_pstride, long long b_rstride, int P, int E, int k, float *mean_dev,
                          float *components_dev, float *scores_dev, double *singular_dev, double *variance_dev,
                          double *ratio_dev, int *status_dev, void *ws, size_t ws_bytes, void *const *events,
                          void *stream) {
  if (!a_dev || (n_b > 0 && !b_dev) || !mean_dev || !components_dev || !scores_dev || !singular_dev || !variance_dev ||
      !ratio_dev || !status_dev || !ws)
    return DT_E_NULL;
  if (n_a < 1 || n_b < 0 || n_a > 32768 || n_b > 32768 || !fit_shape_ok(P, n_a + n_b, E, k)) return DT_E_SHAPE;
  if (!aligned16(a_dev, a_pstride, a_rstride) || (n_b > 0 && !aligned16(b_dev, b_pstride, b_rstride)) ||
      ((uintptr_t)mean_dev & 15) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const int n = n_a + n_b;
  const Layout L(P, n, E, k);
  if (ws_bytes < L.bytes(P)) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  const Rows R{a_dev, n_b > 0 ? b_dev : a_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
  int *flag = (int *)ws, *st = flag + P;
  double *wd = (double *)((char *)ws + L.head);
  DT_HIP_TRY(hipMemsetAsync(ws, 0, L.head, s));
  pca_mean_kernel<<<dim3((E / 4 + kThreads - 1) / kThreads, P), kThreads, 0, s>>>(R, E, wd, L.per, flag, mean_dev);
  DT_LAUNCH_CHECK();
  const int nt = (n + 63) / 64;
  pca_gram_kernel<<<dim3(nt * (nt + 1) / 2, P), kThreads, 0, s>>>(R, E, wd, L.per, flag, nt);
  DT_LAUNCH_CHECK();
  pca_status_kernel<<<P, kThreads, 0, s>>>(n, E, k, wd, L.per, flag, st, status_dev);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[1], s));
  const Tri T{wd, L.per, L.G, L.v, L.pv, L.e, L.tau, st, n};
  if (const int rc = tridiagonalise(T, P, s)) return rc;
  pca_eigen_kernel<<<P, kThreads, 0, s>>>(n, E, k, wd, L.per, st);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[2], s));
  pca_components_kernel<<<dim3((E + kThreads - 1) / kThreads, P), kThreads, 0, s>>>(R, E, k, wd, L.per, st);
  DT_LAUNCH_CHECK();
  pca_finish_kernel<<<P, kThreads, 0, s>>>(n, E, k, wd, L.per, st, mean_dev, components_dev, scores_dev, singular_dev,
                                           variance_dev, ratio_dev);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[3], s));
  return DT_OK;
}

extern "C" int dt_pca_project(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                              const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P, int E,
                              int k, const float *mean_dev, long long mean_pstride, const float *components_dev,
                              long long comp_pstride, float *scores_dev, void *stream) {
  if (!a_dev || (n_b > 0 && !b_dev) || !mean_dev || !components_dev || !scores_dev) return DT_E_NULL;
  if (n_a < 0 || n_b < 0 || (long long)n_a + n_b < 1 || (long long)n_a + n_b > (1 << 30) || P < 1 || P > 65535 ||
      E < 4 || E % 4 || k < 1 || k > DT_PCA_MAX_K || mean_pstride < 0 || comp_pstride < 0)
    return DT_E_SHAPE;
  if ((n_a > 0 && !aligned16(a_dev, a_pstride, a_rstride)) || (n_b > 0 && !aligned16(b_dev, b_pstride, b_rstride)) ||
      !aligned16(mean_dev, mean_pstride, 0) || !aligned16(components_dev, comp_pstride, 0))
    return DT_E_ARG;
  const int n = n_a + n_b;
  const Rows R{n_a > 0 ? a_dev : b_dev, n_b > 0 ? b_dev : a_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
  const int per_block = kThreads / 64;
  pca_project_kernel<<<dim3((n + per_block - 1) / per_block, P), kThreads, 0, (hipStream_t)stream>>>(
      R, E, k, mean_dev, mean_pstride, components_dev, comp_pstride, scores_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
