// KID, improved precision / recall and density / coverage of two feature sets for a batch of independent problems
// (include/dt_hip_quality.h): k-nearest-neighbour statistics and polynomial-kernel sums of the three Gram matrices.
//
// Stages, per problem, all in fp64 (every floating-point sum in a fixed order, the counts are integers, so a result does
// not depend on P, on the other problems of the launch, on the strides or on what the workspace held):
//   1. G_AA, G_BB (upper-triangle tiles, mirrored) and G_AB, 64 x 64 tiles of the shared tile_product over the un-centred
//      rows (quality_gram_kernel); their diagonals, and the non-finite flag read off them: a row's G(x, x) is finite
//      exactly when the row is (quality_diag_kernel);
//   2. the squared radii: one wave per row of d2(A, A) / d2(B, B), the row's distances as 63-bit keys in LDS and the
//      (k+1)-th smallest of them (select_key, dt_quality_math.h) (quality_radius_kernel);
//   3. the counts: one wave per row of d2(A, B) (recall, density, coverage) and one per column (precision), per-row
//      integers without atomics (quality_count_kernel);
//   4. the row sums of kappa, one wave per row of each matrix (quality_kappa_kernel), the subsets' sums gathered from
//      the same matrices (quality_subset_kernel), and the fixed trees, KID, counts, radii and status
//      (quality_finish_kernel).
// The work of a wave on a Gram row and the finish are those of dt_quality_math.h, shared with dt_quality_stream.hip.
#include <math.h>

#include "../../include/dt_hip_quality.h"
#include "dt_internal.h"
#include "dt_quality_math.h"

namespace {

// per-problem workspace (doubles), after a head of P ints (the non-finite flag) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t GAA, GBB, GAB;
  ScoreTail tail;
  __host__ __device__ Layout(int P, int n_a, int n_b) {
    head = flag_head_bytes(P);
    const size_t na = (size_t)n_a, nb = (size_t)n_b;
    GAA = 0;                          // [n_a][n_a]
    GBB = GAA + na * na;              // [n_b][n_b]
    GAB = GBB + nb * nb;              // [n_a][n_b]
    per = tail.place(GAB + na * nb, na, nb);
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

// ---------------------------------------------------------------------------------------------- 1. Gram matrices
// blockIdx.x: the upper-triangle tiles of G_AA, then those of G_BB, then all tiles of G_AB
__global__ __launch_bounds__(kThreads) void quality_gram_kernel(Rows R, int D, double *ws, size_t per, int nta, int ntb) {
  const int p = blockIdx.y;
  const int ua = nta * (nta + 1) / 2, ub = ntb * (ntb + 1) / 2;
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const Layout L(0, R.n_a, R.n_b);
  double *base = ws + (size_t)p * per;
  int tile = blockIdx.x, bi, bj;
  const bool cross = tile >= ua + ub, second = !cross && tile >= ua;
  if (cross) {
    tile -= ua + ub;
    bi = tile / ntb;
    bj = tile % ntb;
  } else {
    upper_tile(second ? tile - ua : tile, second ? ntb : nta, bi, bj);
  }
  // the tile's rows come from set x (first row x0 of the problem's rows, nx of them), its columns from set y
  const int nx = second ? R.n_b : R.n_a, x0 = second ? R.n_a : 0;
  const int ny = cross || second ? R.n_b : R.n_a, y0 = cross || second ? R.n_a : 0;
  const int rx = bi * 64 + lr, ry = bj * 64 + lr;
  double acc[4][4] = {};
  tile_product(D, lr, lq, PlainRow{rx < nx ? row_ptr(R, p, x0 + rx) : nullptr, D},
               PlainRow{ry < ny ? row_ptr(R, p, y0 + ry) : nullptr, D}, acc);
  if (cross)
    store_tile<false>(base + L.GAB, nx, ny, bi, bj, acc);
  else
    store_tile<true>(base + (second ? L.GBB : L.GAA), nx, ny, bi, bj, acc);
}

// the diagonals of G_AA and G_BB side by side, and the flag: a sum of squares of fp32 values cannot overflow in fp64, so
// it is finite exactly when every entry of the row is
__global__ __launch_bounds__(kThreads) void quality_diag_kernel(int n_a, int n_b, double *ws, size_t per, int *flag) {
  __shared__ int bad_s;
  const int p = blockIdx.x;
  const Layout L(0, n_a, n_b);
  double *base = ws + (size_t)p * per;
  if (threadIdx.x == 0) bad_s = 0;
  __syncthreads();
  bool bad = false;
  for (int i = threadIdx.x; i < n_a + n_b; i += kThreads) {
    const double g = i < n_a ? base[L.GAA + (size_t)i * n_a + i] : base[L.GBB + (size_t)(i - n_a) * n_b + (i - n_a)];
    base[L.tail.diag + i] = g;
    bad |= !isfinite(g);
  }
  if (bad) atomicOr(&bad_s, 1);
  __syncthreads();
  if (threadIdx.x == 0) flag[p] = bad_s;
}

// ---------------------------------------------------------------------------------------------- 2. radii
// blockIdx.x: rows of A, then rows of B; one wave each
__global__ __launch_bounds__(kWave) void quality_radius_kernel(int n_a, int n_b, int k, double *ws, size_t per,
                                                               const int *flag) {
  __shared__ unsigned long long key[DT_QUALITY_MAX_ROWS];
  const int p = blockIdx.y;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b);
  double *base = ws + (size_t)p * per;
  const bool second = (int)blockIdx.x >= n_a;
  const int i = second ? blockIdx.x - n_a : blockIdx.x, n = second ? n_b : n_a;
  const double *G = base + (second ? L.GBB : L.GAA) + (size_t)i * n;
  const double *dg = base + L.tail.diag + (second ? n_a : 0);
  const double gi = dg[i];
  for (int j = threadIdx.x; j < n; j += kWave) key[j] = dist2_key(gi, dg[j], G[j]);
  __syncthreads();
  const unsigned long long r = select_key(key, n, k);
  if (threadIdx.x == 0) base[L.tail.r2 + blockIdx.x] = __longlong_as_double((long long)r);
}

// ---------------------------------------------------------------------------------------------- 3. counts
// blockIdx.x < n_a: row i of d2(A, B) -> whether some b_j has a_i within its radius (recall) and how many b_j lie within
// a_i's (density; coverage is whether any does).  Otherwise column j -> whether b_j lies within some a_i's radius
// (precision).  One wave each.
__global__ __launch_bounds__(kWave) void quality_count_kernel(int n_a, int n_b, double *ws, size_t per, const int *flag) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b);
  double *base = ws + (size_t)p * per;
  const double *ga = base + L.tail.diag, *gb = ga + n_a, *ra = base + L.tail.r2, *rb = ra + n_a, *G = base + L.GAB;
  int *hits = reinterpret_cast<int *>(base + L.tail.hits);
  if ((int)blockIdx.x < n_a) {
    const int i = blockIdx.x;
    count_row(G + (size_t)i * n_b, n_b, ga[i], ra[i], gb, rb, hits + i, hits + n_a + i);
  } else {
    const int j = blockIdx.x - n_a;
    const double gj = gb[j];
    int reached = 0;
    for (int i = threadIdx.x; i < n_a; i += kWave) reached |= dist2(ga[i], gj, G[(size_t)i * n_b + j]) < ra[i];
    reached = wave_sum_int(reached) != 0;
    if (threadIdx.x == 0) hits[2 * n_a + j] = reached;
  }
}

// ---------------------------------------------------------------------------------------------- 4. kernel sums
// blockIdx.x: rows of G_AA, rows of G_BB (both without their diagonal entry), rows of G_AB (kappa_row_sum)
__global__ __launch_bounds__(kWave) void quality_kappa_kernel(int n_a, int n_b, int D, double *ws, size_t per,
                                                              const int *flag) {
  const int p = blockIdx.y;
  if (flag[p]) return;
  const Layout L(0, n_a, n_b);
  double *base = ws + (size_t)p * per;
  const int x = blockIdx.x;
  const double *G;
  int n, skip = -1;
  if (x < n_a) { n = n_a; G = base + L.GAA + (size_t)x * n_a; skip = x; }
  else if (x < n_a + n_b) { n = n_b; G = base + L.GBB + (size_t)(x - n_a) * n_b; skip = x - n_a; }
  else { n = n_b; G = base + L.GAB + (size_t)(x - n_a - n_b) * n_b; }
  const double s = kappa_row_sum(G, n, skip, (double)D);
  if (threadIdx.x == 0) base[L.tail.rs + x] = s;
}

// One workgroup per (subset, problem): wave w takes the subset's rows w, w + 4, ..., lanes over its columns, and adds
// the rows' sums in that order; the four waves' sums are then added in one order.
__global__ __launch_bounds__(kThreads) void quality_subset_kernel(int n_a, int n_b, int D, const int *sub_a,
                                                                  const int *sub_b, int S, int m, const double *ws,
                                                                  size_t per, const int *flag, double *kid_out) {
  __shared__ int ia[DT_QUALITY_MAX_ROWS], ib[DT_QUALITY_MAX_ROWS];
  __shared__ double part[3][kThreads / kWave];
  const int s = blockIdx.x, p = blockIdx.y, t = threadIdx.x;
  double *out = kid_out + (size_t)p * (1 + S) + 1 + s;
  if (flag[p]) {
    if (t == 0) *out = NAN;
    return;
  }
  for (int u = t; u < m; u += kThreads) {
    ia[u] = min(max(sub_a[(size_t)s * m + u], 0), n_a - 1);
    ib[u] = min(max(sub_b[(size_t)s * m + u], 0), n_b - 1);
  }
  __syncthreads();
  const Layout L(0, n_a, n_b);
  const double *base = ws + (size_t)p * per;
  const double dd = (double)D;
  const int w = t / kWave, lane = t % kWave;
  double saa = 0.0, sbb = 0.0, sab = 0.0;
  for (int u = w; u < m; u += kThreads / kWave) {
    const double *Ga = base + L.GAA + (size_t)ia[u] * n_a, *Gb = base + L.GBB + (size_t)ib[u] * n_b,
                 *Gx = base + L.GAB + (size_t)ia[u] * n_b;
    double r1 = 0.0, r2 = 0.0, r3 = 0.0;
    for (int v = lane; v < m; v += kWave) {
      if (v != u) {
        r1 += kappa(Ga[ia[v]], dd);
        r2 += kappa(Gb[ib[v]], dd);
      }
      r3 += kappa(Gx[ib[v]], dd);
    }
    saa += wave_sum(r1);
    sbb += wave_sum(r2);
    sab += wave_sum(r3);
  }
  if (lane == 0) { part[0][w] = saa; part[1][w] = sbb; part[2][w] = sab; }
  __syncthreads();
  if (t == 0) {
    double tot[3];
    for (int c = 0; c < 3; ++c) tot[c] = (part[c][0] + part[c][1]) + (part[c][2] + part[c][3]);
    *out = kid_value(tot[0], tot[1], tot[2], m, m);
  }
}

__global__ __launch_bounds__(kThreads) void quality_finish_kernel(int n_a, int n_b, int S, const double *ws, size_t per,
                                                                  const int *flag, double *kid_out, long long *counts_out,
                                                                  double *radii_out, int *status_out) {
  const Layout L(0, n_a, n_b);
  const double *base = ws + (size_t)blockIdx.x * per;
  score_finish(flag[blockIdx.x] != 0, n_a, n_b, L.tail, base, base, kid_out, 1 + S, counts_out, radii_out, status_out);
}

bool shape_ok(int P, int n_a, int n_b, int D) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_b >= 2 && n_a <= DT_QUALITY_MAX_ROWS && n_b <= DT_QUALITY_MAX_ROWS &&
         D >= 4 && D % 4 == 0 && D <= (1 << 20);
}

}  // namespace

extern "C" size_t dt_quality_workspace_bytes(int P, int n_a, int n_b, int D) {
  if (!shape_ok(P, n_a, n_b, D)) return 0;
  return Layout(P, n_a, n_b).bytes(P);
}

extern "C" int dt_quality_scores(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                                 const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P, int D, int k,
                                 const int *sub_a_dev, const int *sub_b_dev, int S, int m, double *kid_dev,
                                 long long *counts_dev, double *radii_dev, int *status_dev, void *ws, size_t ws_bytes,
                                 void *const *events, void *stream) {
  if (!a_dev || !b_dev || !kid_dev || !counts_dev || !status_dev || !ws) return DT_E_NULL;
  if (S > 0 && (!sub_a_dev || !sub_b_dev)) return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b, D)) return DT_E_SHAPE;
  const int n_min = n_a < n_b ? n_a : n_b;
  if (k < 1 || k > n_min - 1) return DT_E_SHAPE;
  if (S < 0 || S > DT_QUALITY_MAX_SUBSETS || (S > 0 && (m < 2 || m > n_min))) return DT_E_SHAPE;
  const Layout L(P, n_a, n_b);
  const auto [rc, R, flag, wd] = set_pair_open(a_dev, n_a, a_pstride, a_rstride, b_dev, n_b, b_pstride, b_rstride, ws,
                                               ws_bytes, L.bytes(P), L.head);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  const int nta = (n_a + 63) / 64, ntb = (n_b + 63) / 64;
  quality_gram_kernel<<<dim3(nta * (nta + 1) / 2 + ntb * (ntb + 1) / 2 + nta * ntb, P), kThreads, 0, s>>>(R, D, wd, L.per,
                                                                                                        nta, ntb);
  DT_LAUNCH_CHECK();
  quality_diag_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[1], s));
  quality_radius_kernel<<<dim3(n_a + n_b, P), kWave, 0, s>>>(n_a, n_b, k, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[2], s));
  quality_count_kernel<<<dim3(n_a + n_b, P), kWave, 0, s>>>(n_a, n_b, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[3], s));
  quality_kappa_kernel<<<dim3(2 * n_a + n_b, P), kWave, 0, s>>>(n_a, n_b, D, wd, L.per, flag);
  DT_LAUNCH_CHECK();
  if (S > 0) {
    quality_subset_kernel<<<dim3(S, P), kThreads, 0, s>>>(n_a, n_b, D, sub_a_dev, sub_b_dev, S, m, wd, L.per, flag,
                                                          kid_dev);
    DT_LAUNCH_CHECK();
  }
  quality_finish_kernel<<<P, kThreads, 0, s>>>(n_a, n_b, S, wd, L.per, flag, kid_dev, counts_dev, radii_dev, status_dev);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[4], s));
  return DT_OK;
}
