// Entropic optimal-transport cost between two sets of states (include/dt_hip_sinkhorn.h): the fp64 cost matrix from fp32
// rows read in place, Sinkhorn iterations on the dual potentials in the log domain, the marginal error of every step and a
// per-problem freeze, all on the device.
//
// sinkhorn_scan_kernel    NaN / Inf in a problem's rows (-> status[q]): kScanSlices workgroups per problem, each its share
//                         of the rows; a hit is an atomicOr of a flag (order-free).
// sinkhorn_init_kernel    eps of the problem -> status[q]; the problem's state words in the workspace; g = 0.
// sinkhorn_cost_kernel    one 64 x 64 tile of C per workgroup, staged through LDS like tile_product (dt_dense64.h) with the
//                         inner operation d = a - b, acc = fma(d, d, acc): one chain per cell over e ascending.
// sinkhorn_rowsum_kernel  r_i = sum_j C_ij, one wave per row (dt_sinkhorn_mean_cost).
// sinkhorn_mean_kernel    one workgroup per problem: the tree over the r_i and the division.
// sinkhorn_row_kernel     half-step 1 of step k: every workgroup first adds up the e_j of step k - 1 (the same tree in all of
//                         them) and leaves when the problem is frozen (from the step after, the recorded flag says so
//                         without the sum); then one wave per row, lanes along j: maximum, sum of exponentials, f_i.
// sinkhorn_col_kernel     half-step 2: one workgroup of kColWaves waves per strip of 64 columns, lanes along j, the waves
//                         take the rows in turn; maxima and partial sums meet in LDS in wave order; g'_j, e_j, g = g'.
//                         Both half-steps read the one row-major C with consecutive lanes on consecutive doubles.
// sinkhorn_finish_kernel  one workgroup per problem: err, iters, the NOT_CONVERGED bit, ot, and f, g where asked for.
// Two launches per step; the host enqueues max_iter steps and never waits.
#include <math.h>

#include "../../include/dt_hip_sinkhorn.h"
#include "dt_dense64.h"

#pragma clang fp contract(off)   // every operation below is rounded on its own; the cost chain names its fma

using namespace dt;

namespace {

constexpr int kMaxN = DT_SINKHORN_MAX_N;
constexpr int kScanSlices = 16;
constexpr int kRowsPerWave = 4;                                  // sinkhorn_row_kernel: 4 waves x 4 rows per workgroup
constexpr int kRowsPerBlock = (kThreads / 64) * kRowsPerWave;
constexpr int kColWaves = 16;                                    // sinkhorn_col_kernel: waves that share the rows of a strip
constexpr int kColThreads = kColWaves * 64;

__host__ __device__ inline int pow2_above(int n) {   // the least power of two >= n (n >= 1)
  int m = 1;
  while (m < n) m <<= 1;
  return m;
}

// one set of rows for a batch of problems
struct Set {
  const float *x;
  long long ps, rs;
  int n;
};

// A chunk's workspace: problem qc works in ws + qc * per (doubles): C [n_a][n_b] at 0, then f [n_a], g [n_b], e [n_b] and
// two ints of state: state[0] != 0: flagged (nothing runs); state[1] = k: frozen after step k.
struct Work {
  double *ws;
  size_t per, f, g, e, state;
  int n_a, n_b;
};

__host__ __device__ inline size_t per_problem_doubles(int n_a, int n_b) {
  return (size_t)n_a * n_b + (size_t)n_a + 2 * (size_t)n_b + 2;
}

Work work_of(void *ws, int n_a, int n_b) {
  const size_t c = (size_t)n_a * n_b;
  return Work{(double *)ws, per_problem_doubles(n_a, n_b), c, c + n_a, c + n_a + n_b, c + n_a + 2 * (size_t)n_b, n_a, n_b};
}

__device__ inline double wave_max(double s) {
  for (int m = 32; m >= 1; m >>= 1) s = fmax(s, __shfl_xor(s, m, 64));
  return s;
}

// The sum of src[0 .. n-1] (n <= kMaxN), padded with 0.0 to the next power of two N, in the tree part[i] += part[i + h],
// h = N/2 .. 1; every thread of the workgroup gets it.  part: kMaxN doubles of LDS.  Begins and ends with a barrier.
__device__ inline double tree_sum(const double *src, int n, double *part) {
  const int n2 = pow2_above(n), nt = blockDim.x;
  __syncthreads();
  for (int i = threadIdx.x; i < n2; i += nt) part[i] = i < n ? src[i] : 0.0;
  __syncthreads();
  for (int h = n2 / 2; h >= 1; h >>= 1) {
    for (int i = threadIdx.x; i < h; i += nt) part[i] += part[i + h];
    __syncthreads();
  }
  const double r = part[0];
  __syncthreads();
  return r;
}

__global__ __launch_bounds__(kThreads) void sinkhorn_scan_kernel(Set S, int E, int *__restrict__ status) {
  const int q = blockIdx.x / kScanSlices, slice = blockIdx.x % kScanSlices;
  const float *base = S.x + q * S.ps;
  int bad = 0;
  for (int i = slice; i < S.n; i += kScanSlices) {
    const float *row = base + i * S.rs;
    for (int e = threadIdx.x; e < E; e += kThreads) bad |= !isfinite(row[e]);
  }
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicOr(status + q, DT_SINKHORN_NONFINITE);
}

// block qc -> problem q0 + qc; eps == nullptr: dt_sinkhorn_mean_cost, which has none
__global__ __launch_bounds__(kThreads) void sinkhorn_init_kernel(Work W, int q0, const double *__restrict__ eps,
                                                                 int *__restrict__ status) {
  const int q = q0 + blockIdx.x;
  double *base = W.ws + (size_t)blockIdx.x * W.per;
  int st = status[q];
  if (eps) {
    const double e = eps[q];
    if (!(isfinite(e) && e > 0.0)) st |= DT_SINKHORN_BAD_EPS;
  }
  for (int j = threadIdx.x; j < W.n_b; j += kThreads) base[W.g + j] = 0.0;
  if (threadIdx.x == 0) {
    int *state = (int *)(base + W.state);
    state[0] = st;
    state[1] = 0;
    status[q] = st;
  }
}

// element k of an fp32 row of len columns (nullptr: no such row), as it is
__device__ inline double element(const float *row, int k, int len) { return row && k < len ? (double)row[k] : 0.0; }

// problems q0 .. q0 + chunk - 1: grid = chunk * tiles, tiles = tiles_i * tiles_j
__global__ __launch_bounds__(kThreads) void sinkhorn_cost_kernel(Set A, Set B, int E, int q0, int tiles_j, int tiles, int pw,
                                                                 Work W) {
  __shared__ double As[16][64], Bs[16][64];
  const int qc = blockIdx.x / tiles, tile = blockIdx.x % tiles, q = q0 + qc;
  double *base = W.ws + (size_t)qc * W.per;
  if (((const int *)(base + W.state))[0]) return;   // uniform
  const int bi = tile / tiles_j, bj = tile % tiles_j;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
  const int i = bi * 64 + lr, j = bj * 64 + lr;
  const float *ra = i < A.n ? A.x + q * A.ps + i * A.rs : nullptr;
  const float *rb = j < B.n ? B.x + q * B.ps + j * B.rs : nullptr;
  double acc[4][4] = {};
  for (int k0 = 0; k0 < E; k0 += 16) {
#pragma unroll
    for (int c = 0; c < 4; ++c) {
      const int k = k0 + 4 * lq + c;
      As[4 * lq + c][lr] = element(ra, k, E);
      Bs[4 * lq + c][lr] = element(rb, k, E);
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
        for (int w = 0; w < 4; ++w) {
          const double d = a[u] - b[w];
          acc[u][w] = fma(d, d, acc[u][w]);
        }
    }
    __syncthreads();
  }
  if (pw == 1) {
#pragma unroll
    for (int u = 0; u < 4; ++u)
#pragma unroll
      for (int w = 0; w < 4; ++w) acc[u][w] = sqrt(acc[u][w]);
  }
  store_tile<false>(base, A.n, B.n, bi, bj, acc);
}

// grid = chunk * blocks, blocks = ceil(n_a / kRowsPerBlock); r_i into the f slot
__global__ __launch_bounds__(kThreads) void sinkhorn_rowsum_kernel(Work W, int blocks) {
  const int qc = blockIdx.x / blocks, blk = blockIdx.x % blocks;
  double *base = W.ws + (size_t)qc * W.per;
  if (((const int *)(base + W.state))[0]) return;   // uniform
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, n_b = W.n_b;
  for (int rr = 0; rr < kRowsPerWave; ++rr) {
    const int i = (blk * (kThreads / 64) + w) * kRowsPerWave + rr;
    if (i >= W.n_a) break;   // uniform in the wave
    const double *Ci = base + (size_t)i * n_b;
    double s = 0.0;
    for (int j = lane; j < n_b; j += 64) s += Ci[j];
    s = wave_sum(s);
    if (lane == 0) base[W.f + i] = s;
  }
}

// block qc -> problem q0 + qc
__global__ __launch_bounds__(kThreads) void sinkhorn_mean_kernel(Work W, int q0, double *__restrict__ mean_cost) {
  __shared__ double part[kMaxN];
  const double *base = W.ws + (size_t)blockIdx.x * W.per;
  if (((const int *)(base + W.state))[0]) {   // uniform
    if (threadIdx.x == 0) mean_cost[q0 + blockIdx.x] = __builtin_nan("");
    return;
  }
  const double s = tree_sum(base + W.f, W.n_a, part);
  if (threadIdx.x == 0) mean_cost[q0 + blockIdx.x] = s / (double)(W.n_a * W.n_b);
}

// half-step 1 of step k (from 1); grid = chunk * blocks, blocks = ceil(n_a / kRowsPerBlock)
__global__ __launch_bounds__(kThreads) void sinkhorn_row_kernel(Work W, int q0, int blocks, int k, double tol,
                                                                const double *__restrict__ eps) {
  __shared__ double part[kMaxN];
  const int qc = blockIdx.x / blocks, blk = blockIdx.x % blocks;
  double *base = W.ws + (size_t)qc * W.per;
  int *state = (int *)(base + W.state);
  if (state[0]) return;   // uniform: set before the first step, never afterwards
  const int n_b = W.n_b;
  if (tol > 0.0 && k > 1) {
    // A problem frozen two or more steps ago has state[1] settled by an earlier launch: leave without the sum.  Thread 0
    // reads it for the workgroup; workgroup 0 of this very launch may be storing k - 1 there, and whichever of the two
    // values is seen, the verdict below is the same (both accesses are atomic, the read decides nothing else).
    __shared__ int frozen;
    if (threadIdx.x == 0) frozen = k > 2 ? __atomic_load_n(state + 1, __ATOMIC_RELAXED) : 0;
    __syncthreads();
    if (frozen) return;   // uniform
    // The e_j of step k - 1 (of the step that froze the problem, if one did: nothing has written them since), by every
    // workgroup in the same order.
    const double err = tree_sum(base + W.e, n_b, part) / (double)n_b;
    if (err <= tol) {   // uniform
      if (blk == 0 && threadIdx.x == 0) __atomic_store_n(state + 1, k - 1, __ATOMIC_RELAXED);
      return;
    }
  }
  const double e = eps[q0 + qc], r = 1.0 / e, logn = log((double)n_b);
  const double *g = base + W.g;
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64;
  for (int rr = 0; rr < kRowsPerWave; ++rr) {
    const int i = (blk * (kThreads / 64) + w) * kRowsPerWave + rr;
    if (i >= W.n_a) break;   // uniform in the wave
    const double *Ci = base + (size_t)i * n_b;
    double m = -INFINITY;
    for (int j = lane; j < n_b; j += 64) m = fmax(m, (g[j] - Ci[j]) * r);
    m = wave_max(m);
    double s = 0.0;
    for (int j = lane; j < n_b; j += 64) s += exp((g[j] - Ci[j]) * r - m);
    s = wave_sum(s);
    if (lane == 0) base[W.f + i] = -e * ((m + log(s)) - logn);
  }
}

// half-step 2; grid = chunk * strips, strips = ceil(n_b / 64)
__global__ __launch_bounds__(kColThreads) void sinkhorn_col_kernel(Work W, int q0, int strips, const double *__restrict__ eps) {
  __shared__ double red[kColWaves][64];
  const int qc = blockIdx.x / strips, strip = blockIdx.x % strips;
  double *base = W.ws + (size_t)qc * W.per;
  const int *state = (const int *)(base + W.state);
  if (state[0] | state[1]) return;   // uniform: both were settled by earlier launches
  const int n_a = W.n_a, n_b = W.n_b;
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, j = strip * 64 + lane;
  const bool valid = j < n_b;
  const double e = eps[q0 + qc], r = 1.0 / e;
  const double *f = base + W.f, *Cj = base + j;
  double m = -INFINITY;
  if (valid)
    for (int i = w; i < n_a; i += kColWaves) m = fmax(m, (f[i] - Cj[(size_t)i * n_b]) * r);
  red[w][lane] = m;
  __syncthreads();
  m = red[0][lane];
#pragma unroll
  for (int v = 1; v < kColWaves; ++v) m = fmax(m, red[v][lane]);
  __syncthreads();
  double s = 0.0;
  if (valid)
    for (int i = w; i < n_a; i += kColWaves) s += exp((f[i] - Cj[(size_t)i * n_b]) * r - m);
  red[w][lane] = s;
  __syncthreads();
  if (w == 0 && valid) {
    s = red[0][lane];
#pragma unroll
    for (int v = 1; v < kColWaves; ++v) s += red[v][lane];
    const double gn = -e * ((m + log(s)) - log((double)n_a));
    base[W.e + j] = fabs(expm1((base[W.g + j] - gn) * r));
    base[W.g + j] = gn;
  }
}

struct Outputs {
  double *ot, *err, *f, *g;
  int *iters, *status;
};

// block qc -> problem q0 + qc
__global__ __launch_bounds__(kThreads) void sinkhorn_finish_kernel(Work W, int q0, int max_iter, double tol, Outputs O) {
  __shared__ double part[kMaxN];
  const int q = q0 + blockIdx.x, n_a = W.n_a, n_b = W.n_b, t = threadIdx.x;
  const double *base = W.ws + (size_t)blockIdx.x * W.per;
  const int *state = (const int *)(base + W.state);
  if (state[0]) {   // uniform; status[q] holds the bits already
    const double nan = __builtin_nan("");
    if (O.f)
      for (int i = t; i < n_a; i += kThreads) O.f[(size_t)q * n_a + i] = nan;
    if (O.g)
      for (int j = t; j < n_b; j += kThreads) O.g[(size_t)q * n_b + j] = nan;
    if (t == 0) { O.ot[q] = nan; O.err[q] = nan; O.iters[q] = 0; }
    return;
  }
  const double err = tree_sum(base + W.e, n_b, part) / (double)n_b;
  const double sf = tree_sum(base + W.f, n_a, part), sg = tree_sum(base + W.g, n_b, part);
  if (O.f)
    for (int i = t; i < n_a; i += kThreads) O.f[(size_t)q * n_a + i] = base[W.f + i];
  if (O.g)
    for (int j = t; j < n_b; j += kThreads) O.g[(size_t)q * n_b + j] = base[W.g + j];
  if (t == 0) {
    const int frozen = state[1];
    O.ot[q] = sf / (double)n_a + sg / (double)n_b;
    O.err[q] = err;
    O.iters[q] = frozen ? frozen : max_iter;
    O.status[q] = !frozen && tol > 0.0 && !(err <= tol) ? DT_SINKHORN_NOT_CONVERGED : DT_SINKHORN_OK;
  }
}

// ---------------------------------------------------------------------------------------------- host
bool set_ok(int n) { return n >= 1 && n <= kMaxN; }
bool batch_ok(int P) { return P >= 1 && P <= DT_SINKHORN_MAX_P; }
bool width_ok(int E) { return E >= 1 && E <= DT_SINKHORN_MAX_E; }

int check_rows(const float *x, long long ps, long long rs) {
  if (ps < 0 || rs < 0) return DT_E_SHAPE;
  return (uintptr_t)x & 3 ? DT_E_ARG : DT_OK;
}

// the common prefix of both entries: flags, state and the cost matrices of problems q0 .. q0 + c - 1
int launch_costs(const Set &A, const Set &B, int E, int q0, int c, int pw, const double *eps, int *status, const Work &W,
                 hipStream_t s) {
  {
    ProfileScope prof(KC_SINKHORN_SCAN, 0.0, 4.0 * E * c * ((double)A.n + B.n), s);
    const Set Aq{A.x + q0 * A.ps, A.ps, A.rs, A.n}, Bq{B.x + q0 * B.ps, B.ps, B.rs, B.n};
    sinkhorn_scan_kernel<<<c * kScanSlices, kThreads, 0, s>>>(Aq, E, status + q0);
    DT_LAUNCH_CHECK();
    sinkhorn_scan_kernel<<<c * kScanSlices, kThreads, 0, s>>>(Bq, E, status + q0);
    DT_LAUNCH_CHECK();
  }
  {
    ProfileScope prof(KC_SINKHORN_INIT, 0.0, 8.0 * c * (B.n + 2.0), s);
    sinkhorn_init_kernel<<<c, kThreads, 0, s>>>(W, q0, eps, status);
    DT_LAUNCH_CHECK();
  }
  const int tiles_j = (B.n + 63) / 64, tiles = tiles_j * ((A.n + 63) / 64);
  ProfileScope prof(KC_SINKHORN_COST, 3.0 * c * A.n * B.n * E, (double)c * (4.0 * E * (A.n + B.n) + 8.0 * A.n * B.n), s);
  sinkhorn_cost_kernel<<<c * tiles, kThreads, 0, s>>>(A, B, E, q0, tiles_j, tiles, pw, W);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace

extern "C" size_t dt_sinkhorn_workspace_bytes(int P, int n_a, int n_b) {
  return set_ok(n_a) && set_ok(n_b) && batch_ok(P) ? sizeof(double) * (size_t)P * per_problem_doubles(n_a, n_b) : 0;
}

extern "C" int dt_sinkhorn_mean_cost(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev,
                                     long long b_ps, long long b_rs, int n_b, int E, int P, int p, double *mean_cost_dev,
                                     int *status_dev, void *ws, size_t ws_bytes, void *stream) {
  if (!a_dev || !b_dev || !mean_cost_dev || !status_dev || !ws) return DT_E_NULL;
  if (!set_ok(n_a) || !set_ok(n_b) || !width_ok(E) || !batch_ok(P)) return DT_E_SHAPE;
  int rc;
  if ((rc = check_rows(a_dev, a_ps, a_rs)) != DT_OK) return rc;
  if ((rc = check_rows(b_dev, b_ps, b_rs)) != DT_OK) return rc;
  if (p != 1 && p != 2) return DT_E_ARG;
  if (((uintptr_t)mean_cost_dev & 7) || ((uintptr_t)status_dev & 3) || ((uintptr_t)ws & 15)) return DT_E_ARG;
  const size_t per = sizeof(double) * per_problem_doubles(n_a, n_b);
  if (ws_bytes < per) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t fit = ws_bytes / per;
  const int chunk = fit < (size_t)P ? (int)fit : P;
  const Set A{a_dev, a_ps, a_rs, n_a}, B{b_dev, b_ps, b_rs, n_b};
  const Work W = work_of(ws, n_a, n_b);
  const int blocks = (n_a + kRowsPerBlock - 1) / kRowsPerBlock;
  DT_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int) * (size_t)P, s));
  for (int q0 = 0; q0 < P; q0 += chunk) {
    const int c = P - q0 < chunk ? P - q0 : chunk;
    if ((rc = launch_costs(A, B, E, q0, c, p, nullptr, status_dev, W, s)) != DT_OK) return rc;
    {
      ProfileScope prof(KC_SINKHORN_ROWSUM, (double)c * n_a * n_b, 8.0 * c * n_a * n_b, s);
      sinkhorn_rowsum_kernel<<<c * blocks, kThreads, 0, s>>>(W, blocks);
      DT_LAUNCH_CHECK();
    }
    ProfileScope prof(KC_SINKHORN_MEAN, (double)c * n_a, 8.0 * c * n_a, s);
    sinkhorn_mean_kernel<<<c, kThreads, 0, s>>>(W, q0, mean_cost_dev);
    DT_LAUNCH_CHECK();
  }
  return DT_OK;
}

extern "C" int dt_sinkhorn_ot(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev, long long b_ps,
                              long long b_rs, int n_b, int E, int P, int p, const double *eps_dev, int max_iter, double tol,
                              double *ot_dev, double *err_dev, int *iters_dev, int *status_dev, double *f_dev, double *g_dev,
                              void *ws, size_t ws_bytes, void *stream) {
  if (!a_dev || !b_dev || !eps_dev || !ot_dev || !err_dev || !iters_dev || !status_dev || !ws) return DT_E_NULL;
  if (!set_ok(n_a) || !set_ok(n_b) || !width_ok(E) || !batch_ok(P) || max_iter < 1 || max_iter > DT_SINKHORN_MAX_ITER)
    return DT_E_SHAPE;
  int rc;
  if ((rc = check_rows(a_dev, a_ps, a_rs)) != DT_OK) return rc;
  if ((rc = check_rows(b_dev, b_ps, b_rs)) != DT_OK) return rc;
  if ((p != 1 && p != 2) || !(tol >= 0.0) || !(tol <= DBL_MAX)) return DT_E_ARG;
  if (((uintptr_t)eps_dev & 7) || ((uintptr_t)ot_dev & 7) || ((uintptr_t)err_dev & 7) || ((uintptr_t)f_dev & 7) ||
      ((uintptr_t)g_dev & 7) || ((uintptr_t)iters_dev & 3) || ((uintptr_t)status_dev & 3) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const size_t per = sizeof(double) * per_problem_doubles(n_a, n_b);
  if (ws_bytes < per) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t fit = ws_bytes / per;
  const int chunk = fit < (size_t)P ? (int)fit : P;
  const Set A{a_dev, a_ps, a_rs, n_a}, B{b_dev, b_ps, b_rs, n_b};
  const Work W = work_of(ws, n_a, n_b);
  const Outputs O{ot_dev, err_dev, f_dev, g_dev, iters_dev, status_dev};
  const int blocks = (n_a + kRowsPerBlock - 1) / kRowsPerBlock, strips = (n_b + 63) / 64;
  DT_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int) * (size_t)P, s));
  for (int q0 = 0; q0 < P; q0 += chunk) {
    const int c = P - q0 < chunk ? P - q0 : chunk;
    if ((rc = launch_costs(A, B, E, q0, c, p, eps_dev, status_dev, W, s)) != DT_OK) return rc;
    const double cells = (double)c * n_a * n_b;
    for (int k = 1; k <= max_iter; ++k) {
      {
        ProfileScope prof(KC_SINKHORN_ROW, 6.0 * cells, 16.0 * cells, s);
        sinkhorn_row_kernel<<<c * blocks, kThreads, 0, s>>>(W, q0, blocks, k, tol, eps_dev);
        DT_LAUNCH_CHECK();
      }
      ProfileScope prof(KC_SINKHORN_COL, 6.0 * cells, 16.0 * cells, s);
      sinkhorn_col_kernel<<<c * strips, kColThreads, 0, s>>>(W, q0, strips, eps_dev);
      DT_LAUNCH_CHECK();
    }
    ProfileScope prof(KC_SINKHORN_FINISH, 0.0, 8.0 * c * (2.0 * n_a + 3.0 * n_b), s);
    sinkhorn_finish_kernel<<<c, kThreads, 0, s>>>(W, q0, max_iter, tol, O);
    DT_LAUNCH_CHECK();
  }
  return DT_OK;
}
