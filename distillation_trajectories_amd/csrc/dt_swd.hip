// Sliced Wasserstein distance between two sets of states (include/dt_hip_swd.h): projection of both sets onto the caller's
// directions, a sort of every projection, the exact 1-D W_p^p per direction, its mean and maximum over the directions; all
// fp64 from fp32 rows read in place.
//
// swd_scan_kernel      NaN / Inf in a problem's rows (-> status[q]) and in theta (-> a flag in the workspace): kScanSlices
//                      workgroups per problem, each its share of the rows; a hit is an atomicOr of 1 (order-free).
// swd_status_kernel    status[q] = (status[q] | theta flag) != 0.
// swd_project_kernel   one 64 (directions) x 64 (rows) tile per workgroup on tile_product (dt_dense64.h) with a loader that
//                      reads one float at a time and does not centre: one FMA chain per cell over e ascending.  Writes
//                      proj [chunk][L][n], a column per (problem, direction).
// swd_sort_kernel      one workgroup per (problem, direction): the column to LDS, bitonic sort, back in place.
// swd_pair_kernel      one workgroup per (problem, direction): both columns to LDS, sorted there unless they come sorted,
//                      one thread per element of the larger set adds its overlaps, the partial sums meet in a tree fixed by
//                      the larger size.  Writes the total T_l.
// swd_reduce_kernel    one workgroup per problem: w = T / (nB nS), the tree over the T_l, the maximum and its first index,
//                      or NaN and -1 for a flagged problem.
// dt_swd, dt_swd_sorted + dt_swd_distance run the same device functions on the same values, so they agree bit for bit.
#include <math.h>

#include "../../include/dt_hip_swd.h"
#include "dt_dense64.h"

using namespace dt;

namespace {

constexpr int kMaxN = DT_SWD_MAX_N;
constexpr int kMaxL = DT_SWD_MAX_L;
constexpr int kScanSlices = 16;
constexpr size_t kHeadBytes = DT_SWD_SORTED_WORKSPACE_BYTES;   // the theta flag lives in its first int

__host__ __device__ inline int pow2_above(int n) {   // the least power of two >= n (n >= 1)
  int m = 1;
  while (m < n) m <<= 1;
  return m;
}

// loader for tile_product: element k of an fp32 row of len columns (nullptr: no such row), as it is
struct PlainRow {
  const float *row;
  int len;
  static constexpr int W = 1;
  __device__ void operator()(int k, double (&v)[1]) const { v[0] = row && k < len ? (double)row[k] : 0.0; }
};

// one set of rows for a batch of problems, or theta (P = 1 problem of L rows)
struct Set {
  const float *x;
  long long ps, rs;
  int n;
};

__global__ __launch_bounds__(kThreads) void swd_scan_kernel(Set S, int E, int P, Set T, int *__restrict__ status,
                                                            int *__restrict__ theta_flag) {
  const int q = blockIdx.x / kScanSlices, slice = blockIdx.x % kScanSlices;
  const bool is_theta = q == P;   // (only launched with T.n > 0)
  const float *base = is_theta ? T.x : S.x + q * S.ps;
  const long long rs = is_theta ? T.rs : S.rs;
  const int n = is_theta ? T.n : S.n;
  int bad = 0;
  for (int i = slice; i < n; i += kScanSlices) {
    const float *row = base + i * rs;
    for (int e = threadIdx.x; e < E; e += kThreads) bad |= !isfinite(row[e]);
  }
  bad = __syncthreads_or(bad);
  if (bad && threadIdx.x == 0) atomicOr(is_theta ? theta_flag : status + q, 1);
}

__global__ __launch_bounds__(kThreads) void swd_status_kernel(int *__restrict__ status, int P, const int *__restrict__ theta_flag) {
  const int bad = *theta_flag;
  for (int q = blockIdx.x * kThreads + threadIdx.x; q < P; q += gridDim.x * kThreads)
    status[q] = (status[q] | bad) ? DT_SWD_NONFINITE : DT_SWD_OK;
}

// problems q0 .. q0 + chunk - 1: grid = chunk * tiles, tiles = tiles_l * tiles_i
__global__ __launch_bounds__(kThreads) void swd_project_kernel(Set S, int E, Set T, int q0, int tiles_i, int tiles,
                                                               const int *__restrict__ status, double *__restrict__ proj) {
  const int qc = blockIdx.x / tiles, tile = blockIdx.x % tiles, q = q0 + qc;
  if (status[q]) return;   // uniform
  const int bl = tile / tiles_i, bi = tile % tiles_i;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int l = bl * 64 + lr, i = bi * 64 + lr;
  double acc[4][4] = {};
  tile_product(E, lr, lq, PlainRow{l < T.n ? T.x + l * T.rs : nullptr, E},
               PlainRow{i < S.n ? S.x + q * S.ps + i * S.rs : nullptr, E}, acc);
  store_tile<false>(proj + (size_t)qc * T.n * S.n, T.n, S.n, bl, bi, acc);
}

// ascending, in LDS: v[0 .. n2-1], n2 a power of two, the tail beyond the data padded with +Inf by the caller.  Begins and
// ends with a barrier.
__device__ inline void sort_lds(double *v, int n2) {
  __syncthreads();
  for (int k = 2; k <= n2; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int h = threadIdx.x; h < n2 / 2; h += kThreads) {
        const int i = ((h & ~(j - 1)) << 1) | (h & (j - 1)), ij = i | j;
        const bool up = (i & k) == 0;
        const double a = v[i], b = v[ij];
        if ((a > b) == up) { v[i] = b; v[ij] = a; }
      }
      __syncthreads();
    }
}

__device__ inline void load_column(double *v, const double *g, int n, int n2) {
  for (int i = threadIdx.x; i < n2; i += kThreads) v[i] = i < n ? g[i] : INFINITY;
}

// T of include/dt_hip_swd.h from two sorted columns in LDS, nB >= nS; every thread gets it.  Begins with a barrier.
__device__ inline double distance_lds(const double *big, int nB, const double *small, int nS, int pw, double *part) {
  const int n2 = pow2_above(nB);
  __syncthreads();
  for (int i = threadIdx.x; i < n2; i += kThreads) {
    double acc = 0.0;
    if (i < nB) {
      const int lo = i * nS, hi = lo + nS;   // <= 2^22
      const double x = big[i];
      for (int j = lo / nB; j * nB < hi; ++j) {   // j < nS
        const int wt = min(hi, (j + 1) * nB) - max(lo, j * nB);
        const double d = fabs(x - small[j]);
        acc = fma((double)wt, pw == 2 ? d * d : d, acc);
      }
    }
    part[i] = acc;
  }
  __syncthreads();
  for (int h = n2 / 2; h >= 1; h >>= 1) {
    for (int i = threadIdx.x; i < h; i += kThreads) part[i] += part[i + h];
    __syncthreads();
  }
  return part[0];
}

__global__ __launch_bounds__(kThreads) void swd_sort_kernel(double *__restrict__ sorted, int n, int L,
                                                            const int *__restrict__ status) {
  __shared__ double v[kMaxN];
  const int q = blockIdx.x / L;
  double *g = sorted + (size_t)blockIdx.x * n;
  if (status[q]) {   // uniform
    for (int i = threadIdx.x; i < n; i += kThreads) g[i] = __builtin_nan("");
    return;
  }
  const int n2 = pow2_above(n);
  load_column(v, g, n, n2);
  sort_lds(v, n2);
  for (int i = threadIdx.x; i < n; i += kThreads) g[i] = v[i];
}

// Columns of problem q0 + qc, direction l: ca + qc*a_ps + l*n_a and cb likewise (a_ps == 0: shared).  SORT: they hold raw
// projections.  Flags: fa[q*fa_s] | fb[q*fb_s].  total [chunk][L].
struct Columns {
  const double *ca, *cb;
  long long a_ps, b_ps;
  const int *fa, *fb;
  int fa_s, fb_s, n_a, n_b;
};

template <bool SORT>
__global__ __launch_bounds__(kThreads) void swd_pair_kernel(Columns C, int L, int q0, int pw, double *__restrict__ total) {
  __shared__ double va[kMaxN], vb[kMaxN], part[kMaxN];
  const int qc = blockIdx.x / L, l = blockIdx.x % L, q = q0 + qc;
  if (C.fa[(size_t)q * C.fa_s] | C.fb[(size_t)q * C.fb_s]) return;   // uniform; swd_reduce_kernel does not read the totals then
  const int a2 = pow2_above(C.n_a), b2 = pow2_above(C.n_b);
  load_column(va, C.ca + qc * C.a_ps + (size_t)l * C.n_a, C.n_a, a2);
  load_column(vb, C.cb + qc * C.b_ps + (size_t)l * C.n_b, C.n_b, b2);
  if constexpr (SORT) {
    sort_lds(va, a2);
    sort_lds(vb, b2);
  }
  const bool a_big = C.n_a >= C.n_b;
  const double t = a_big ? distance_lds(va, C.n_a, vb, C.n_b, pw, part) : distance_lds(vb, C.n_b, va, C.n_a, pw, part);
  if (threadIdx.x == 0) total[blockIdx.x] = t;
}

struct Outputs {
  double *w, *mean_w, *max_w;
  int *argmax, *status;
};

// block qc -> problem q0 + qc
__global__ __launch_bounds__(kThreads) void swd_reduce_kernel(const double *__restrict__ total, int L, int q0, double denom,
                                                              const int *fa, int fa_s, const int *fb, int fb_s, Outputs O) {
  __shared__ double part[kMaxL];
  __shared__ double best_v[kThreads];
  __shared__ int best_i[kThreads];
  const int t = threadIdx.x, q = q0 + blockIdx.x;
  // (dt_swd: O.status is fa and fb, stride 1 -- word q is read here by every thread of this workgroup alone, and thread 0
  // writes the value it already has)
  const int bad = fa[(size_t)q * fa_s] | fb[(size_t)q * fb_s];
  if (bad) {   // uniform
    const double nan = __builtin_nan("");
    if (O.w)
      for (int l = t; l < L; l += kThreads) O.w[(size_t)q * L + l] = nan;
    if (t == 0) { O.mean_w[q] = nan; O.max_w[q] = nan; O.argmax[q] = -1; O.status[q] = DT_SWD_NONFINITE; }
    return;
  }
  const double *T = total + (size_t)blockIdx.x * L;
  const int l2 = pow2_above(L);
  double bv = -1.0;   // every w is >= 0
  int bi = 0;
  for (int l = t; l < l2; l += kThreads) {
    const double v = l < L ? T[l] : 0.0;
    part[l] = v;
    if (l < L) {
      const double w = v / denom;
      if (O.w) O.w[(size_t)q * L + l] = w;
      if (w > bv) { bv = w; bi = l; }   // l ascending: the first index of this thread's maximum
    }
  }
  best_v[t] = bv;
  best_i[t] = bi;
  __syncthreads();
  for (int h = l2 / 2; h >= 1; h >>= 1) {
    for (int l = t; l < h; l += kThreads) part[l] += part[l + h];
    __syncthreads();
  }
  for (int h = kThreads / 2; h >= 1; h >>= 1) {
    if (t < h) {
      const double ov = best_v[t + h];
      const int oi = best_i[t + h];
      if (ov > best_v[t] || (ov == best_v[t] && oi < best_i[t])) { best_v[t] = ov; best_i[t] = oi; }
    }
    __syncthreads();
  }
  if (t == 0) {
    O.mean_w[q] = part[0] / (denom * (double)L);
    O.max_w[q] = best_v[0];
    O.argmax[q] = best_i[0];
    O.status[q] = DT_SWD_OK;
  }
}

// ---------------------------------------------------------------------------------------------- host
bool set_ok(int n) { return n >= 1 && n <= kMaxN; }
bool batch_ok(int L, int P) { return L >= 1 && L <= kMaxL && P >= 1 && P <= DT_SWD_MAX_P; }
bool width_ok(int E) { return E >= 1 && E <= DT_SWD_MAX_E; }

size_t per_problem_bytes(int n_a, int n_b, int L) { return sizeof(double) * (size_t)L * (1 + (size_t)n_a + n_b); }

int check_rows(const float *x, long long ps, long long rs) {
  if (ps < 0 || rs < 0) return DT_E_SHAPE;
  return (uintptr_t)x & 3 ? DT_E_ARG : DT_OK;
}

int check_outputs(const double *w, const double *mean_w, const double *max_w, const int *argmax, const int *status, int p) {
  if (((uintptr_t)w & 7) || ((uintptr_t)mean_w & 7) || ((uintptr_t)max_w & 7) || ((uintptr_t)argmax & 3) || ((uintptr_t)status & 3))
    return DT_E_ARG;
  return p == 1 || p == 2 ? DT_OK : DT_E_ARG;
}

// non-finite rows of S into status (which the caller has zeroed, or which holds another set's flags); theta as well when T.n > 0
int launch_scan(const Set &S, int E, int P, const Set &T, int *status, int *theta_flag, hipStream_t s) {
  ProfileScope prof(KC_SWD_SCAN, 0.0, 4.0 * E * ((double)P * S.n + T.n), s);
  swd_scan_kernel<<<(P + (T.n > 0 ? 1 : 0)) * kScanSlices, kThreads, 0, s>>>(S, E, P, T, status, theta_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int launch_status(int *status, int P, const int *theta_flag, hipStream_t s) {
  ProfileScope prof(KC_SWD_SCAN, 0.0, 8.0 * P, s);
  swd_status_kernel<<<grid_blocks(P, 256), kThreads, 0, s>>>(status, P, theta_flag);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int launch_project(const Set &S, int E, const Set &T, int q0, int chunk, const int *status, double *proj, hipStream_t s) {
  const int tiles_i = (S.n + 63) / 64, tiles = tiles_i * ((T.n + 63) / 64);
  ProfileScope prof(KC_SWD_PROJECT, 2.0 * chunk * T.n * S.n * E, (double)chunk * (4.0 * E * (S.n + T.n) + 8.0 * T.n * S.n), s);
  swd_project_kernel<<<chunk * tiles, kThreads, 0, s>>>(S, E, T, q0, tiles_i, tiles, status, proj);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

template <bool SORT>
int launch_pair(const Columns &C, int L, int q0, int chunk, int pw, double *total, hipStream_t s) {
  ProfileScope prof(SORT ? KC_SWD_SORT_PAIR : KC_SWD_PAIR, 0.0, 8.0 * chunk * L * (C.n_a + C.n_b + 1.0), s);
  swd_pair_kernel<SORT><<<chunk * L, kThreads, 0, s>>>(C, L, q0, pw, total);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int launch_reduce(const double *total, int L, int q0, int chunk, const Columns &C, const Outputs &O, hipStream_t s) {
  const int nB = C.n_a >= C.n_b ? C.n_a : C.n_b, nS = C.n_a >= C.n_b ? C.n_b : C.n_a;
  ProfileScope prof(KC_SWD_REDUCE, 0.0, 8.0 * chunk * L * (O.w ? 2.0 : 1.0), s);
  swd_reduce_kernel<<<chunk, kThreads, 0, s>>>(total, L, q0, (double)(nB * nS), C.fa, C.fa_s, C.fb, C.fb_s, O);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace

extern "C" size_t dt_swd_sorted_bytes(int P, int n, int L) {
  return set_ok(n) && batch_ok(L, P) ? sizeof(double) * (size_t)P * L * n : 0;
}

extern "C" size_t dt_swd_workspace_bytes(int P, int n_a, int n_b, int L) {
  return set_ok(n_a) && set_ok(n_b) && batch_ok(L, P) ? kHeadBytes + (size_t)P * per_problem_bytes(n_a, n_b, L) : 0;
}

extern "C" size_t dt_swd_distance_workspace_bytes(int P, int L) {
  return batch_ok(L, P) ? sizeof(double) * (size_t)P * L : 0;
}

extern "C" int dt_swd_sorted(const float *x_dev, long long x_ps, long long x_rs, int n, int E, const float *theta_dev,
                             long long theta_rs, int L, int P, double *sorted_dev, int *status_dev, void *ws, size_t ws_bytes,
                             void *stream) {
  if (!x_dev || !theta_dev || !sorted_dev || !status_dev || !ws) return DT_E_NULL;
  if (!set_ok(n) || !width_ok(E) || !batch_ok(L, P)) return DT_E_SHAPE;
  int rc;
  if ((rc = check_rows(x_dev, x_ps, x_rs)) != DT_OK) return rc;
  if ((rc = check_rows(theta_dev, 0, theta_rs)) != DT_OK) return rc;
  if (((uintptr_t)sorted_dev & 7) || ((uintptr_t)status_dev & 3) || ((uintptr_t)ws & 15)) return DT_E_ARG;
  if (ws_bytes < kHeadBytes) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const Set S{x_dev, x_ps, x_rs, n}, T{theta_dev, 0, theta_rs, L};
  int *theta_flag = (int *)ws;
  DT_HIP_TRY(hipMemsetAsync(theta_flag, 0, sizeof(int), s));
  DT_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int) * (size_t)P, s));
  if ((rc = launch_scan(S, E, P, T, status_dev, theta_flag, s)) != DT_OK) return rc;
  if ((rc = launch_status(status_dev, P, theta_flag, s)) != DT_OK) return rc;
  if ((rc = launch_project(S, E, T, 0, P, status_dev, sorted_dev, s)) != DT_OK) return rc;
  ProfileScope prof(KC_SWD_SORT, 0.0, 16.0 * P * L * n, s);
  swd_sort_kernel<<<P * L, kThreads, 0, s>>>(sorted_dev, n, L, status_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

extern "C" int dt_swd_distance(const double *sa_dev, long long sa_ps, const int *status_a_dev, int n_a, const double *sb_dev,
                               long long sb_ps, const int *status_b_dev, int n_b, int L, int P, int p, double *w_dev,
                               double *mean_w_dev, double *max_w_dev, int *argmax_dev, int *status_dev, void *ws,
                               size_t ws_bytes, void *stream) {
  if (!sa_dev || !sb_dev || !status_a_dev || !status_b_dev || !mean_w_dev || !max_w_dev || !argmax_dev || !status_dev || !ws)
    return DT_E_NULL;
  if (!set_ok(n_a) || !set_ok(n_b) || !batch_ok(L, P)) return DT_E_SHAPE;
  if ((sa_ps != 0 && sa_ps < (long long)L * n_a) || (sb_ps != 0 && sb_ps < (long long)L * n_b)) return DT_E_SHAPE;
  int rc;
  if ((rc = check_outputs(w_dev, mean_w_dev, max_w_dev, argmax_dev, status_dev, p)) != DT_OK) return rc;
  if (((uintptr_t)sa_dev & 7) || ((uintptr_t)sb_dev & 7) || ((uintptr_t)status_a_dev & 3) || ((uintptr_t)status_b_dev & 3) ||
      ((uintptr_t)ws & 15))
    return DT_E_ARG;
  if (ws_bytes < sizeof(double) * (size_t)L) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t fit = ws_bytes / (sizeof(double) * (size_t)L);
  const int chunk = fit < (size_t)P ? (int)fit : P;
  double *total = (double *)ws;
  const Outputs O{w_dev, mean_w_dev, max_w_dev, argmax_dev, status_dev};
  for (int q0 = 0; q0 < P; q0 += chunk) {
    const int c = P - q0 < chunk ? P - q0 : chunk;
    // (the kernels address a chunk's columns from its first problem)
    const Columns C{sa_dev + q0 * sa_ps, sb_dev + q0 * sb_ps, sa_ps, sb_ps, status_a_dev, status_b_dev, sa_ps ? 1 : 0,
                    sb_ps ? 1 : 0, n_a, n_b};
    if ((rc = launch_pair<false>(C, L, q0, c, p, total, s)) != DT_OK) return rc;
    if ((rc = launch_reduce(total, L, q0, c, C, O, s)) != DT_OK) return rc;
  }
  return DT_OK;
}

extern "C" int dt_swd(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev, long long b_ps,
                      long long b_rs, int n_b, int E, const float *theta_dev, long long theta_rs, int L, int P, int p,
                      double *w_dev, double *mean_w_dev, double *max_w_dev, int *argmax_dev, int *status_dev, void *ws,
                      size_t ws_bytes, void *stream) {
  if (!a_dev || !b_dev || !theta_dev || !mean_w_dev || !max_w_dev || !argmax_dev || !status_dev || !ws) return DT_E_NULL;
  if (!set_ok(n_a) || !set_ok(n_b) || !width_ok(E) || !batch_ok(L, P)) return DT_E_SHAPE;
  int rc;
  if ((rc = check_rows(a_dev, a_ps, a_rs)) != DT_OK) return rc;
  if ((rc = check_rows(b_dev, b_ps, b_rs)) != DT_OK) return rc;
  if ((rc = check_rows(theta_dev, 0, theta_rs)) != DT_OK) return rc;
  if ((rc = check_outputs(w_dev, mean_w_dev, max_w_dev, argmax_dev, status_dev, p)) != DT_OK) return rc;
  if ((uintptr_t)ws & 15) return DT_E_ARG;
  const size_t per = per_problem_bytes(n_a, n_b, L);
  if (ws_bytes < kHeadBytes + per) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  const size_t fit = (ws_bytes - kHeadBytes) / per;
  const int chunk = fit < (size_t)P ? (int)fit : P;
  const Set A{a_dev, a_ps, a_rs, n_a}, B{b_dev, b_ps, b_rs, n_b}, T{theta_dev, 0, theta_rs, L}, none{nullptr, 0, 0, 0};
  int *theta_flag = (int *)ws;
  double *total = (double *)((char *)ws + kHeadBytes);
  double *pa = total + (size_t)chunk * L, *pb = pa + (size_t)chunk * L * n_a;
  DT_HIP_TRY(hipMemsetAsync(theta_flag, 0, sizeof(int), s));
  DT_HIP_TRY(hipMemsetAsync(status_dev, 0, sizeof(int) * (size_t)P, s));
  if ((rc = launch_scan(A, E, P, T, status_dev, theta_flag, s)) != DT_OK) return rc;
  if ((rc = launch_scan(B, E, P, none, status_dev, theta_flag, s)) != DT_OK) return rc;
  if ((rc = launch_status(status_dev, P, theta_flag, s)) != DT_OK) return rc;
  const Columns C{pa, pb, (long long)L * n_a, (long long)L * n_b, status_dev, status_dev, 1, 1, n_a, n_b};
  const Outputs O{w_dev, mean_w_dev, max_w_dev, argmax_dev, status_dev};
  for (int q0 = 0; q0 < P; q0 += chunk) {
    const int c = P - q0 < chunk ? P - q0 : chunk;
    if ((rc = launch_project(A, E, T, q0, c, status_dev, pa, s)) != DT_OK) return rc;
    if ((rc = launch_project(B, E, T, q0, c, status_dev, pb, s)) != DT_OK) return rc;
    if ((rc = launch_pair<true>(C, L, q0, c, p, total, s)) != DT_OK) return rc;
    if ((rc = launch_reduce(total, L, q0, c, C, O, s)) != DT_OK) return rc;
  }
  return DT_OK;
}
