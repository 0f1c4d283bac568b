// Exact t-SNE of a batch of independent problems (include/dt_hip_tsne.h): sklearn's method="exact" with 2 components, the
// t-SNE of analysis/dimensionality/ on the device.
//
// Affinities, per problem (the mean, the Gram tile product and the block sums are those of dt_dense64.h):
//   1. column means in fp64 and the non-finite flag (tsne_mean_kernel);
//   2. the centred Gram matrix G = Xc Xc^T in fp64 (tsne_gram_kernel); D_ij = G_ii + G_jj - 2 G_ij, clamped at 0;
//   3. one wave per row (tsne_row_kernel): the row's distances stay in registers through sklearn's binary search for the
//      precision; the conditional row C_i and its sum go to the workspace;
//   4. P = (C + C^T) / sum floored at DBL_EPSILON, diagonal 0, and the status word (tsne_joint_kernel).
// Descent (tsne_descend_kernel): one workgroup per problem runs a whole range of iterations in one launch; y, update and
// gains stay in LDS, P is read from memory (row i is column i, so a group's lanes read it coalesced; copying P into LDS
// first, which fits up to n = 128, was measured at 3 % and not kept: DESIGN.md §9n).
//
// Every sum has a fixed order that depends only on n: a lane's chain over its columns ascending, one butterfly over the
// group's lanes, then one wave's chain and butterfly over the rows.  A problem's bits do not depend on P, on the other
// problems of the launch, or on how a range of iterations is cut into calls.
#include <float.h>
#include <math.h>

#include "../../include/dt_hip_tsne.h"
#include "dt_internal.h"
#include "dt_dense64.h"

namespace {

// ---------------------------------------------------------------------------------------------- affinities
// per-problem workspace (doubles), after a head of P ints (non-finite flag) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t mean, G, C, rowsum;
  __host__ __device__ Layout(int P, int n, int E) {
    head = flag_head_bytes(P);
    const size_t N = (size_t)n;
    mean = 0;
    G = mean + (size_t)E;
    C = G + N * N;
    rowsum = C + N * N;
    per = rowsum + N;
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

__global__ __launch_bounds__(kThreads) void tsne_mean_kernel(Rows R, int E, double *ws, size_t per, int *flag) {
  const int p = blockIdx.y;
  const int q = blockIdx.x * kThreads + threadIdx.x;
  if (4 * q >= E) return;
  double m[4];
  const bool bad = quad_mean(R, p, 0, 1, q, m);
  double *out = ws + (size_t)p * per + 4 * (size_t)q;
  out[0] = m[0]; out[1] = m[1]; out[2] = m[2]; out[3] = m[3];
  if (bad) atomicOr(flag + p, 1);
}

// G = Xc Xc^T over the upper triangle of 64 x 64 tiles (tile_product, dt_dense64.h), rows centred as they are loaded
__global__ __launch_bounds__(kThreads) void tsne_gram_kernel(Rows R, int E, double *ws, size_t per, const int *flag,
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

constexpr int kRowSlots = DT_TSNE_MAX_N / 64;   // columns lane, lane + 64, ... of a row: 8 per lane at n = 512

// One wave per row i: sklearn's _binary_search_perplexity on D_i. (column i left out), then C_i. = exp(-beta D_i.) / sum
// of the last step evaluated and the row's sum.
__global__ __launch_bounds__(kThreads) void tsne_row_kernel(int n, int E, double log_perplexity, double *ws, size_t per,
                                                            const int *flag) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const int lane = threadIdx.x % 64;
  const int i = blockIdx.x * (kThreads / 64) + threadIdx.x / 64;
  if (i >= n) return;                                      // whole waves leave; no block barrier below
  const Layout L(0, n, E);
  double *base = ws + (size_t)p * per;
  const double *G = base + L.G;
  const double gii = G[(size_t)i * n + i];
  double d[kRowSlots], c[kRowSlots];
  bool on[kRowSlots];
#pragma unroll
  for (int m = 0; m < kRowSlots; ++m) {
    const int j = lane + 64 * m;
    on[m] = j < n && j != i;
    d[m] = on[m] ? fmax(gii + G[(size_t)j * n + j] - 2.0 * G[(size_t)i * n + j], 0.0) : 0.0;
    c[m] = 0.0;
  }
  double beta = 1.0, beta_min = -INFINITY, beta_max = INFINITY;
  for (int step = 0; step < 100; ++step) {
    double s = 0.0;
#pragma unroll
    for (int m = 0; m < kRowSlots; ++m) {
      c[m] = on[m] ? exp(-d[m] * beta) : 0.0;
      s += c[m];
    }
    double sum = wave_sum(s);
    if (sum == 0.0) sum = 1e-8;
    double sd = 0.0;
#pragma unroll
    for (int m = 0; m < kRowSlots; ++m) {
      c[m] /= sum;
      sd = fma(d[m], c[m], sd);
    }
    const double diff = log(sum) + beta * wave_sum(sd) - log_perplexity;
    if (fabs(diff) <= 1e-5) break;
    if (diff > 0.0) {
      beta_min = beta;
      beta = beta_max == INFINITY ? beta * 2.0 : (beta + beta_max) / 2.0;
    } else {
      beta_max = beta;
      beta = beta_min == -INFINITY ? beta / 2.0 : (beta + beta_min) / 2.0;
    }
  }
  double s = 0.0;
#pragma unroll
  for (int m = 0; m < kRowSlots; ++m) {
    const int j = lane + 64 * m;
    if (j < n) base[L.C + (size_t)i * n + j] = c[m];
    s += c[m];
  }
  s = wave_sum(s);
  if (lane == 0) base[L.rowsum + i] = s;
}

// row i of P = max((C + C^T) / sum, DBL_EPSILON), diagonal 0; NaN and status 1 for a problem with a non-finite row
__global__ __launch_bounds__(kThreads) void tsne_joint_kernel(int n, int E, const double *ws, size_t per,
                                                              const int *flag, double *p_out, int *status_out) {
  __shared__ double red[kThreads];
  const int p = blockIdx.y, i = blockIdx.x, t = threadIdx.x;
  double *out = p_out + ((size_t)p * n + i) * n;
  if (flag[p]) {
    for (int j = t; j < n; j += kThreads) out[j] = NAN;
    if (i == 0 && t == 0) status_out[p] = DT_TSNE_NONFINITE;
    return;
  }
  const Layout L(0, n, E);
  const double *base = ws + (size_t)p * per;
  double s = 0.0;
  for (int r = t; r < n; r += kThreads) s += base[L.rowsum + r];
  const double total = fmax(2.0 * block_sum(s, red), DBL_EPSILON);
  const double *C = base + L.C;
  for (int j = t; j < n; j += kThreads)
    out[j] = j == i ? 0.0 : fmax((C[(size_t)i * n + j] + C[(size_t)j * n + i]) / total, DBL_EPSILON);
  if (i == 0 && t == 0) status_out[p] = DT_TSNE_OK;
}

// ---------------------------------------------------------------------------------------------- descent
constexpr int kDescendThreads = 512;

// lanes of a row's group: 16 up to n = 128 (32 rows in flight), a whole wave above
__host__ __device__ inline int group_lanes(int n) { return n <= 128 ? 16 : 64; }

__device__ inline double group_sum(double s, int lanes) {
  for (int m = lanes / 2; m >= 1; m >>= 1) s += __shfl_xor(s, m, 64);
  return s;
}

// sum of v[0 .. count-1] in LDS by the first wave (a lane's chain over its entries ascending, then a butterfly); every
// thread gets the result
__device__ double lds_sum(const double *v, int count, double *slot) {
  __syncthreads();
  if (threadIdx.x < 64) {
    double s = 0.0;
    for (int q = threadIdx.x; q < count; q += 64) s += v[q];
    s = wave_sum(s);
    if (threadIdx.x == 0) *slot = s;
  }
  __syncthreads();
  const double r = *slot;
  return r;
}

// One pass over all pairs (i, j != i), a group of `lanes` lanes per row, w = 1 / (1 + |y_i - y_j|^2):
//   neither  : rowv[i] = sum_j w                                              (the row's part of Z)
//   FORCE    : grad[i] = 4 sum_j (alpha P_ij - max(w / Z, eps)) w (y_i - y_j)
//   KL       : rowv[i] = sum_j alpha P_ij log(max(alpha P_ij, eps) / max(w / Z, eps))
template <bool FORCE, bool KL>
__device__ void pair_pass(const double *Pm, int n, int lanes, const double *y, double alpha, double Z, double *grad,
                          double *rowv) {
  const int g = threadIdx.x / lanes, l = threadIdx.x % lanes, groups = kDescendThreads / lanes;
  for (int r0 = 0; r0 < n; r0 += groups) {
    const int r = r0 + g;
    double fx = 0.0, fy = 0.0, acc = 0.0;
    if (r < n) {
      const double yx = y[2 * r], yy = y[2 * r + 1];
      const double *Pr = Pm + (size_t)r * n;
      for (int j = l; j < n; j += lanes) {
        if (j == r) continue;
        const double dx = yx - y[2 * j], dy = yy - y[2 * j + 1];
        const double w = 1.0 / (1.0 + (dx * dx + dy * dy));
        if (!FORCE && !KL) {
          acc += w;
        } else {
          const double pij = alpha * Pr[j];
          const double q = fmax(w / Z, DBL_EPSILON);
          if (FORCE) {
            const double m = (pij - q) * w;
            fx = fma(m, dx, fx);
            fy = fma(m, dy, fy);
          }
          if (KL) acc += pij * log(fmax(pij, DBL_EPSILON) / q);
        }
      }
    }
    if (FORCE) {
      fx = group_sum(fx, lanes);
      fy = group_sum(fy, lanes);
    }
    if (KL || !FORCE) acc = group_sum(acc, lanes);
    if (l == 0 && r < n) {
      if (FORCE) {
        grad[2 * r] = 4.0 * fx;
        grad[2 * r + 1] = 4.0 * fy;
      }
      if (KL || !FORCE) rowv[r] = acc;
    }
  }
}

__global__ __launch_bounds__(kDescendThreads) void tsne_descend_kernel(const double *p_in, int n, double *state,
                                                                        int it_begin, int it_end, dt_tsne_params prm,
                                                                        float *embedding, double *kl_out) {
  __shared__ double y[2 * DT_TSNE_MAX_N], upd[2 * DT_TSNE_MAX_N], gain[2 * DT_TSNE_MAX_N], grad[2 * DT_TSNE_MAX_N];
  __shared__ double rowv[DT_TSNE_MAX_N];
  __shared__ double slot;
  const int p = blockIdx.x, t = threadIdx.x, n2 = 2 * n;
  const double *Pm = p_in + (size_t)p * n * n;
  double *st = state + (size_t)p * DT_TSNE_STATE_DOUBLES(n);
  float *emb = embedding + (size_t)p * n2;
  if (isnan(Pm[1])) {                                       // a problem dt_tsne_affinities gave up on: NaN out, state kept
    for (int q = t; q < n2; q += kDescendThreads) emb[q] = NAN;
    if (t == 0) kl_out[p] = NAN;
    return;
  }
  for (int q = t; q < n2; q += kDescendThreads) {
    y[q] = st[q];
    upd[q] = st[n2 + q];
    gain[q] = st[2 * n2 + q];
  }
  double best_error = st[3 * n2], best_iter = st[3 * n2 + 1], done = st[3 * n2 + 2];
  int stop = (int)st[3 * n2 + 3];
  const int lanes = group_lanes(n);
  __syncthreads();

  for (int it = it_begin; it < it_end && stop == DT_TSNE_RUNNING; ++it) {
    if (it == prm.exaggeration_iters) {                    // sklearn's second _gradient_descent call starts afresh
      for (int q = t; q < n2; q += kDescendThreads) {
        upd[q] = 0.0;
        gain[q] = 1.0;
      }
      best_error = DBL_MAX;
      best_iter = (double)it;
    }
    const int stage = it < prm.exaggeration_iters ? 0 : 1;
    const double alpha = stage == 0 ? prm.early_exaggeration : 1.0;
    const bool check = (it + 1) % prm.n_iter_check == 0;
    pair_pass<false, false>(Pm, n, lanes, y, alpha, 0.0, grad, rowv);
    const double Z = lds_sum(rowv, n, &slot);
    if (check)
      pair_pass<true, true>(Pm, n, lanes, y, alpha, Z, grad, rowv);
    else
      pair_pass<true, false>(Pm, n, lanes, y, alpha, Z, grad, rowv);
    __syncthreads();
    for (int q = t; q < n2; q += kDescendThreads) {
      const double gq = grad[q], u = upd[q];
      double gn = u * gq < 0.0 ? gain[q] + 0.2 : gain[q] * 0.8;
      gn = fmax(gn, prm.min_gain);
      const double scaled = gq * gn;
      const double un = prm.momentum[stage] * u - prm.learning_rate * scaled;
      gain[q] = gn;
      upd[q] = un;
      y[q] += un;
      grad[q] = scaled * scaled;
    }
    done = (double)(it + 1);
    if (check) {                                           // the error is that of y before this iteration's step
      const double error = lds_sum(rowv, n, &slot);
      const double grad_norm = sqrt(lds_sum(grad, n2, &slot));
      if (error < best_error) {
        best_error = error;
        best_iter = (double)it;
      } else if ((double)it - best_iter > (double)prm.n_iter_without_progress[stage]) {
        stop = DT_TSNE_NO_PROGRESS;
      }
      if (stop == DT_TSNE_RUNNING && grad_norm <= prm.min_grad_norm) stop = DT_TSNE_GRAD_NORM;
    }
    __syncthreads();
  }

  // the plain KL of the current y
  pair_pass<false, false>(Pm, n, lanes, y, 1.0, 0.0, grad, rowv);
  const double Z = lds_sum(rowv, n, &slot);
  pair_pass<false, true>(Pm, n, lanes, y, 1.0, Z, grad, rowv);
  const double kl = lds_sum(rowv, n, &slot);
  for (int q = t; q < n2; q += kDescendThreads) {
    st[q] = y[q];
    st[n2 + q] = upd[q];
    st[2 * n2 + q] = gain[q];
    emb[q] = (float)y[q];
  }
  if (t == 0) {
    st[3 * n2] = best_error;
    st[3 * n2 + 1] = best_iter;
    st[3 * n2 + 2] = done;
    st[3 * n2 + 3] = (double)stop;
    kl_out[p] = kl;
  }
}

bool shape_ok(int P, int n, int E) {
  return P >= 1 && P <= 65535 && n >= 4 && n <= DT_TSNE_MAX_N && E >= 4 && E % 4 == 0 && E <= (1 << 28);
}

}  // namespace

extern "C" size_t dt_tsne_workspace_bytes(int P, int n, int E) {
  if (!shape_ok(P, n, E)) return 0;
  return Layout(P, n, E).bytes(P);
}

extern "C" int dt_tsne_affinities(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                                  const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P, int E,
                                  double perplexity, double *p_dev, int *status_dev, void *ws, size_t ws_bytes,
                                  void *stream) {
  if (!a_dev || (n_b > 0 && !b_dev) || !p_dev || !status_dev || !ws) return DT_E_NULL;
  if (n_a < 1 || n_b < 0 || n_a > DT_TSNE_MAX_N || n_b > DT_TSNE_MAX_N || !shape_ok(P, n_a + n_b, E)) return DT_E_SHAPE;
  const int n = n_a + n_b;
  if (!(perplexity > 0.0 && perplexity < (double)n)) return DT_E_ARG;
  if (!aligned16(a_dev, a_pstride, a_rstride) || (n_b > 0 && !aligned16(b_dev, b_pstride, b_rstride)) ||
      ((uintptr_t)ws & 15) || ((uintptr_t)p_dev & 7))
    return DT_E_ARG;
  const Layout L(P, n, E);
  if (ws_bytes < L.bytes(P)) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Rows R{a_dev, n_b > 0 ? b_dev : a_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
  int *flag = (int *)ws;
  double *wd = (double *)((char *)ws + L.head);
  DT_HIP_TRY(hipMemsetAsync(ws, 0, L.head, s));
  tsne_mean_kernel<<<dim3((E / 4 + kThreads - 1) / kThreads, P), kThreads, 0, s>>>(R, E, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  const int nt = (n + 63) / 64;
  tsne_gram_kernel<<<dim3(nt * (nt + 1) / 2, P), kThreads, 0, s>>>(R, E, wd, L.per, flag, nt);
  DT_LAUNCH_CHECK();
  const int per_block = kThreads / 64;
  tsne_row_kernel<<<dim3((n + per_block - 1) / per_block, P), kThreads, 0, s>>>(n, E, log(perplexity), wd, L.per, flag);
  DT_LAUNCH_CHECK();
  tsne_joint_kernel<<<dim3(n, P), kThreads, 0, s>>>(n, E, wd, L.per, flag, p_dev, status_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_tsne_descend(const double *p_dev, int P, int n, double *state_dev, int it_begin, int it_end,
                               const dt_tsne_params *params, float *embedding_dev, double *kl_dev, void *stream) {
  if (!p_dev || !state_dev || !params || !embedding_dev || !kl_dev) return DT_E_NULL;
  if (P < 1 || P > 65535 || n < 4 || n > DT_TSNE_MAX_N) return DT_E_SHAPE;
  const dt_tsne_params prm = *params;
  if (it_begin < 0 || it_end < it_begin || prm.n_iter_check < 1 || prm.exaggeration_iters < 0 ||
      prm.n_iter_without_progress[0] < 0 || prm.n_iter_without_progress[1] < 0 || !(prm.early_exaggeration > 0.0) ||
      !(prm.learning_rate > 0.0) || !(prm.min_gain >= 0.0) || !(prm.min_grad_norm >= 0.0) ||
      !isfinite(prm.momentum[0]) || !isfinite(prm.momentum[1]) || ((uintptr_t)p_dev & 7) || ((uintptr_t)state_dev & 7))
    return DT_E_ARG;
  tsne_descend_kernel<<<P, kDescendThreads, 0, (hipStream_t)stream>>>(p_dev, n, state_dev, it_begin, it_end, prm,
                                                                       embedding_dev, kl_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
