// KID, improved precision / recall and density / coverage for sets of up to 131072 rows (include/dt_hip_quality_stream.h):
// the scores of dt_quality.hip without ever holding an n x n matrix.  Per problem the workspace holds one panel of
// panel_rows rows of a Gram matrix; the host loops over the row panels of A x A, B x B and A x B, and each panel is
// consumed before the next overwrites it.
//
// Launches, all in fp64 (every floating-point sum in a fixed order, the radii exact order statistics, the counts
// integers, so a result does not depend on P, on the other problems of the launch, on the strides, on what the workspace
// held or on panel_rows):
//   0. the diagonals G(x, x) from the diagonal tiles (qstream_diag_kernel) and the non-finite flags read off them
//      (qstream_flag_kernel);
//   1. a panel of X Y^T, 64 x 64 tiles on v_mfma_f64_16x16x4_f64 (qstream_gram_kernel);
//   2. on panels of A x A and B x B: the squared radii, one wave per row streaming the row's 63-bit keys through a
//      threshold and a 2048-key LDS buffer (qstream_select_kernel);
//   3. on every panel: the row sums of kappa (qstream_kappa_kernel);
//   4. on panels of A x B: per row the recall flag and the density count (qstream_count_rows_kernel), per column the
//      precision flag OR-ed into its word (qstream_count_cols_kernel);
//   5. the fixed trees, KID, counts, radii and status (qstream_finish_kernel).
// With a shared teacher (a_pstride == 0, P > 1) the A side lives in problem 0's part of the workspace and is formed once.
#include <math.h>

#include "../../include/dt_hip_quality_stream.h"
#include "dt_internal.h"
#include "dt_quality_math.h"

namespace {

constexpr int kBuf = 2048;      // keys of the selection's LDS buffer
constexpr int kStep = 4 * kWave;   // keys a wave takes per step of the stream

// per-problem workspace (doubles), after a head of 2 P ints (the non-finite flags of A and of B) rounded to 256 bytes
struct Layout {
  size_t head, per;
  size_t panel, diag, r2, rs, hits;
  __host__ __device__ Layout(int P, int n_a, int n_b, int panel_rows) {
    head = flag_head_bytes(2 * P);
    const size_t na = (size_t)n_a, nb = (size_t)n_b;
    panel = 0;                                         // [panel_rows][columns of the matrix the panel is of]
    diag = panel + (size_t)panel_rows * (na > nb ? na : nb);   // G(a_i, a_i), then G(b_j, b_j)
    r2 = diag + na + nb;                               // squared radii, A's then B's
    rs = r2 + na + nb;                                 // kappa row sums: A x A, B x B, A x B
    hits = rs + 2 * na + nb;                           // ints: recall flag [n_a], density count [n_a], precision flag [n_b]
    per = hits + (2 * na + nb + 1) / 2;
  }
  __host__ __device__ size_t bytes(int P) const { return head + (size_t)P * per * sizeof(double); }
};

// what every kernel reads of the call; ash: A is shared, its vectors live in problem 0's part of the workspace
struct Job {
  Rows R;
  Layout L;
  double *ws;
  int *flag;   // [P][2]: A's rows, B's rows
  int D, k, ash;
};

__device__ inline double *part_of(const Job &J, int p) { return J.ws + (size_t)p * J.L.per; }
__device__ inline double *a_part_of(const Job &J, int p) { return part_of(J, J.ash ? 0 : p); }
__device__ inline bool bad_problem(const Job &J, int p) { return (J.flag[2 * p] | J.flag[2 * p + 1]) != 0; }

// ---------------------------------------------------------------------------------------------- Gram tiles
// One 64 x 64 tile of X Y^T per workgroup of kThreads; the contraction runs over the D columns, 16 per LDS stage.  Thread
// t stages the float4 of columns 4 (t % 4) .. + 3 of tile row t / 4 of both factors, as tile_product does.  Wave w owns
// output rows 16 w .. 16 w + 15 as four 16 x 16 blocks; per four columns of the stage lane l takes X[row l % 16][k = l / 16]
// and Y[col l % 16][k = l / 16], and the instruction adds the four products of every output to its accumulator, which
// lies at column l % 16, rows l / 16 + 4 i of the block (the inner loop of cov_gram_kernel in dt_fid.hip).
//
// The bit argument.  Every output of every tile, wherever the tile lies and whichever launch forms it, runs through this
// one sequence of instructions on the products x_k y_k, k ascending (columns past D are staged as zeros and add nothing),
// and the product commutes.  So two rows give the same bits wherever they meet: G(x, y) == G(y, x), and G(x, x) of the
// diagonals (qstream_diag_kernel calls this function on the diagonal tiles) has the bits of the entry (x, x) of a panel
// of A x A.  Hence the self-distance, and the distance of two bitwise-equal rows, is exactly 0.
typedef double mfma_acc __attribute__((ext_vector_type(4)));

__device__ inline void gram_tile(int D, const float *xrow, const float *yrow, mfma_acc (&acc)[4]) {
  __shared__ double Xs[16][64], Ys[16][64];
  const int t = threadIdx.x, lr = t / 4, kq = 4 * (t % 4);
  const int w = t / 64, lane = t % 64, lk = lane / 16, lc = lane % 16;
  for (int k0 = 0; k0 < D; k0 += 16) {
    double vx[4] = {0.0, 0.0, 0.0, 0.0}, vy[4] = {0.0, 0.0, 0.0, 0.0};
    if (k0 + kq < D) {
      if (xrow) {
        const float4 x = *reinterpret_cast<const float4 *>(xrow + k0 + kq);
        vx[0] = (double)x.x; vx[1] = (double)x.y; vx[2] = (double)x.z; vx[3] = (double)x.w;
      }
      if (yrow) {
        const float4 y = *reinterpret_cast<const float4 *>(yrow + k0 + kq);
        vy[0] = (double)y.x; vy[1] = (double)y.y; vy[2] = (double)y.z; vy[3] = (double)y.w;
      }
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) { Xs[kq + i][lr] = vx[i]; Ys[kq + i][lr] = vy[i]; }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < 16; kk += 4) {
      const double x = Xs[kk + lk][16 * w + lc];
#pragma unroll
      for (int j = 0; j < 4; ++j)
        acc[j] = __builtin_amdgcn_mfma_f64_16x16x4f64(x, Ys[kk + lk][16 * j + lc], acc[j], 0, 0, 0);
    }
    __syncthreads();
  }
}

// the rows of set `set` (0: A, 1: B) of problem p
__device__ inline const float *set_row(const Rows &R, int set, int p, int i) {
  return set == 0 ? R.a + p * R.a_ps + i * R.a_rs : R.b + p * R.b_ps + i * R.b_rs;
}

// ---------------------------------------------------------------------------------------------- 0. diagonals, flags
// blockIdx.x: the diagonal tiles of A x A, then those of B x B.  A shared A is done by problem 0 alone.
__global__ __launch_bounds__(kThreads) void qstream_diag_kernel(Job J, int nta) {
  const int p = blockIdx.y;
  const bool second = (int)blockIdx.x >= nta;
  if (!second && J.ash && p > 0) return;
  const int set = second ? 1 : 0, tile = second ? blockIdx.x - nta : blockIdx.x;
  const int n = second ? J.R.n_b : J.R.n_a;
  const int row = tile * 64 + threadIdx.x / 4;
  const float *src = row < n ? set_row(J.R, set, p, row) : nullptr;
  mfma_acc acc[4] = {};
  gram_tile(J.D, src, src, acc);
  double *diag = part_of(J, p) + J.L.diag + (second ? J.R.n_a : 0);
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, lk = lane / 16, lc = lane % 16;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = 16 * w + lk + 4 * i, c = 16 * j + lc;
      if (r == c && tile * 64 + r < n) diag[tile * 64 + r] = acc[j][i];
    }
}

// flag[p] = (a row of A is not finite, a row of B is not finite): a sum of squares of fp32 values cannot overflow in
// fp64, so G(x, x) is finite exactly when every entry of the row is
__global__ __launch_bounds__(kThreads) void qstream_flag_kernel(Job J) {
  __shared__ int bad_s[2];
  const int p = blockIdx.x, n_a = J.R.n_a, n_b = J.R.n_b;
  if (threadIdx.x < 2) bad_s[threadIdx.x] = 0;
  __syncthreads();
  const double *da = a_part_of(J, p) + J.L.diag, *db = part_of(J, p) + J.L.diag + n_a;
  bool bad_a = false, bad_b = false;
  for (int i = threadIdx.x; i < n_a; i += kThreads) bad_a |= !isfinite(da[i]);
  for (int j = threadIdx.x; j < n_b; j += kThreads) bad_b |= !isfinite(db[j]);
  if (bad_a) atomicOr(&bad_s[0], 1);
  if (bad_b) atomicOr(&bad_s[1], 1);
  __syncthreads();
  if (threadIdx.x < 2) J.flag[2 * p + threadIdx.x] = bad_s[threadIdx.x];
}

// ---------------------------------------------------------------------------------------------- 1. Gram panel
// rows r0 .. r0 + rows - 1 of set xs against all rows of set ys -> panel [rows][n of ys]; blockIdx.x: tile row * ntc +
// tile column.  A panel of A x A with A shared is launched for problem 0 alone.
__global__ __launch_bounds__(kThreads) void qstream_gram_kernel(Job J, int xs, int ys, int r0, int rows, int ntc) {
  const int p = blockIdx.y;
  if (J.flag[2 * p] | (xs + ys > 0 ? J.flag[2 * p + 1] : 0)) return;
  const int bi = blockIdx.x / ntc, bj = blockIdx.x % ntc;
  const int nx = xs ? J.R.n_b : J.R.n_a, ny = ys ? J.R.n_b : J.R.n_a;
  const int lr = threadIdx.x / 4;
  const int rx = r0 + bi * 64 + lr, ry = bj * 64 + lr;
  mfma_acc acc[4] = {};
  gram_tile(J.D, bi * 64 + lr < rows && rx < nx ? set_row(J.R, xs, p, rx) : nullptr,
            ry < ny ? set_row(J.R, ys, p, ry) : nullptr, acc);
  double *G = part_of(J, p) + J.L.panel;
  const int w = threadIdx.x / 64, lane = threadIdx.x % 64, lk = lane / 16, lc = lane % 16;
#pragma unroll
  for (int j = 0; j < 4; ++j)
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int r = bi * 64 + 16 * w + lk + 4 * i, c = bj * 64 + 16 * j + lc;
      if (r < rows && r0 + r < nx && c < ny) G[(size_t)r * ny + c] = acc[j][i];
    }
}

// ---------------------------------------------------------------------------------------------- 2. radii
// The (k+1)-th smallest of buf[0 .. count), count > k: the largest r with fewer than k + 1 keys below it, built bit by bit
// from the top, each bit one count over the buffer (the selection of quality_radius_kernel).  One wave.
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

// One wave per row of the panel of d2(A, A) (set 0) or d2(B, B) (set 1); a key is the 63-bit pattern of dist2 (a
// non-negative double orders as its bit pattern).  The wave keeps a threshold T, at first above every key, and appends
// a key to the LDS buffer only if it is < T.  When the buffer cannot take another step's keys, t = the (k+1)-th smallest
// of the buffer becomes T and the buffer shrinks to its keys < t (at most k) plus as many copies of t as make k + 1
// entries.  A dropped key is >= T, and at least k + 1 entries <= T stay in the buffer, so the (k+1)-th smallest of the
// buffer is always that of the keys seen so far, duplicates counted: the result is exact and depends on nothing but the
// row's keys.  k + 1 <= 1024 entries leave room for a step after every refill.
__global__ __launch_bounds__(kWave) void qstream_select_kernel(Job J, int set, int r0) {
  __shared__ unsigned long long buf[kBuf];
  const int p = blockIdx.y;
  if (J.flag[2 * p] | (set ? J.flag[2 * p + 1] : 0)) return;
  const int n = set ? J.R.n_b : J.R.n_a, off = set ? J.R.n_a : 0, k = J.k;
  double *base = part_of(J, p);
  const int i = r0 + blockIdx.x, lane = threadIdx.x;
  const double *G = base + J.L.panel + (size_t)blockIdx.x * n;
  const double *dg = base + J.L.diag + off;
  const double gi = dg[i];
  const unsigned long long none = ~0ull, below_me = (1ull << lane) - 1;
  unsigned long long T = none;
  int count = 0;
  for (int j0 = 0; j0 < n; j0 += kStep) {
    if (count > kBuf - kStep) {
      __syncthreads();
      const unsigned long long t = select_key(buf, count, k);
      int kept = 0;
      for (int c0 = 0; c0 < count; c0 += kWave) {      // in place: a chunk is read before anything at or above it is written
        const unsigned long long v = c0 + lane < count ? buf[c0 + lane] : none;
        const bool keep = v < t;
        const unsigned long long m = __ballot(keep);
        if (keep) buf[kept + __popcll(m & below_me)] = v;
        kept += __popcll(m);
      }
      __syncthreads();
      for (int c = kept + lane; c < k + 1; c += kWave) buf[c] = t;
      count = k + 1;
      T = t;
    }
    unsigned long long key[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int j = j0 + kWave * u + lane;
      key[u] = j < n ? (unsigned long long)__double_as_longlong(dist2(gi, dg[j], G[j])) & 0x7fffffffffffffffull : none;
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const bool take = key[u] < T;
      const unsigned long long m = __ballot(take);
      if (take) buf[count + __popcll(m & below_me)] = key[u];
      count += __popcll(m);
    }
  }
  __syncthreads();
  const unsigned long long r = select_key(buf, count, k);
  if (lane == 0) base[J.L.r2 + off + i] = __longlong_as_double((long long)r);
}

// ---------------------------------------------------------------------------------------------- 3. kernel sums
// One wave per row of the panel; kind 0: A x A, 1: B x B (both without the diagonal entry, skipped by index), 2: A x B.
// Lanes over the columns in ascending order, then the butterfly: a row's sum does not depend on the panel it fell into.
__global__ __launch_bounds__(kWave) void qstream_kappa_kernel(Job J, int kind, int r0) {
  const int p = blockIdx.y;
  if (J.flag[2 * p] | (kind ? J.flag[2 * p + 1] : 0)) return;
  const int n_a = J.R.n_a, n_b = J.R.n_b, n = kind ? n_b : n_a;
  double *base = part_of(J, p);
  const int i = r0 + blockIdx.x, skip = kind < 2 ? i : -1;
  const double *G = base + J.L.panel + (size_t)blockIdx.x * n;
  const double dd = (double)J.D;
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kWave)
    if (j != skip) s += kappa(G[j], dd);
  s = wave_sum(s);
  if (threadIdx.x == 0) base[J.L.rs + (kind == 0 ? 0 : kind == 1 ? n_a : n_a + n_b) + i] = s;
}

// ---------------------------------------------------------------------------------------------- 4. counts
// One wave per row i of the panel of A x B: whether some b_j has a_i within its radius (recall) and how many b_j lie
// within a_i's (density; coverage is whether any does).
__global__ __launch_bounds__(kWave) void qstream_count_rows_kernel(Job J, int r0) {
  const int p = blockIdx.y;
  if (bad_problem(J, p)) return;
  const int n_a = J.R.n_a, n_b = J.R.n_b;
  double *base = part_of(J, p);
  const double *abase = a_part_of(J, p);
  const int i = r0 + blockIdx.x;
  const double *G = base + J.L.panel + (size_t)blockIdx.x * n_b;
  const double *gb = base + J.L.diag + n_a, *rb = base + J.L.r2 + n_a;
  const double gi = abase[J.L.diag + i], ri = abase[J.L.r2 + i];
  int *hits = reinterpret_cast<int *>(base + J.L.hits);
  int within = 0, reached = 0;
  for (int j = threadIdx.x; j < n_b; j += kWave) {
    const double d = dist2(gi, gb[j], G[j]);
    within += d < ri;
    reached |= d < rb[j];
  }
  within = wave_sum_int(within);
  reached = wave_sum_int(reached) != 0;
  if (threadIdx.x == 0) {
    hits[i] = reached;
    hits[n_a + i] = within;
  }
}

// 64 columns of the panel of A x B per workgroup: wave w takes the panel's rows w, w + 4, ... (a wave reads 64
// neighbouring columns of one row), lane l column l of the 64; whether b_j lies within some a_i's radius (precision),
// OR-ed over the four waves and then into the column's word.  The panels of a problem are successive launches on one
// stream and a column has one owner per launch, so no atomics; the first panel's launch (r0 == 0) sets the word.
__global__ __launch_bounds__(kThreads) void qstream_count_cols_kernel(Job J, int r0, int rows) {
  __shared__ int part[kThreads / kWave][kWave];
  const int p = blockIdx.y;
  if (bad_problem(J, p)) return;
  const int n_a = J.R.n_a, n_b = J.R.n_b;
  double *base = part_of(J, p);
  const double *abase = a_part_of(J, p);
  const double *ga = abase + J.L.diag, *ra = abase + J.L.r2, *G = base + J.L.panel;
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave, j = blockIdx.x * kWave + lane;
  int reached = 0;
  if (j < n_b) {
    const double gj = base[J.L.diag + n_a + j];
    for (int r = w; r < rows; r += kThreads / kWave)
      reached |= dist2(ga[r0 + r], gj, G[(size_t)r * n_b + j]) < ra[r0 + r];
  }
  part[w][lane] = reached;
  __syncthreads();
  if (w == 0 && j < n_b) {
    int *word = reinterpret_cast<int *>(base + J.L.hits) + 2 * n_a + j;
    const int all = part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
    *word = r0 == 0 ? all : (*word | all);
  }
}

// ---------------------------------------------------------------------------------------------- 5. finish
// the order of quality_finish_kernel
__global__ __launch_bounds__(kThreads) void qstream_finish_kernel(Job J, double *kid_out, long long *counts_out,
                                                                  double *radii_out, int *status_out) {
  __shared__ double red[kThreads];
  __shared__ long long redi[kThreads];
  const int p = blockIdx.x, t = threadIdx.x, n_a = J.R.n_a, n_b = J.R.n_b;
  long long *counts = counts_out + 4 * (size_t)p;
  double *radii = radii_out ? radii_out + (size_t)p * (n_a + n_b) : nullptr;
  if (bad_problem(J, p)) {
    if (radii)
      for (int i = t; i < n_a + n_b; i += kThreads) radii[i] = NAN;
    if (t == 0) {
      kid_out[p] = NAN;
      counts[0] = counts[1] = counts[2] = counts[3] = -1;
      status_out[p] = DT_QUALITY_NONFINITE;
    }
    return;
  }
  const double *base = part_of(J, p), *abase = a_part_of(J, p);
  const double *rs = base + J.L.rs, *rsa = abase + J.L.rs;
  const int *hits = reinterpret_cast<const int *>(base + J.L.hits);
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
    for (int i = t; i < n_a + n_b; i += kThreads) radii[i] = (i < n_a ? abase : base)[J.L.r2 + i];
  if (t == 0) {
    kid_out[p] = kid_value(saa, sbb, sab, n_a, n_b);
    counts[0] = precision;
    counts[1] = recall;
    counts[2] = density;
    counts[3] = coverage;
    status_out[p] = DT_QUALITY_OK;
  }
}

bool shape_ok(int P, int n_a, int n_b, int D, int panel_rows) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_b >= 2 && n_a <= DT_QUALITY_STREAM_MAX_ROWS &&
         n_b <= DT_QUALITY_STREAM_MAX_ROWS && D >= 4 && D % 4 == 0 && D <= (1 << 20) && panel_rows >= 64 &&
         panel_rows <= 4096 && panel_rows % 64 == 0;
}

}  // namespace

extern "C" size_t dt_quality_stream_workspace_bytes(int P, int n_a, int n_b, int D, int panel_rows) {
  if (!shape_ok(P, n_a, n_b, D, panel_rows)) return 0;
  return Layout(P, n_a, n_b, panel_rows).bytes(P);
}

extern "C" int dt_quality_stream_scores(const float *a_dev, int n_a, long long a_pstride, long long a_rstride,
                                        const float *b_dev, int n_b, long long b_pstride, long long b_rstride, int P,
                                        int D, int k, int panel_rows, double *kid_dev, long long *counts_dev,
                                        double *radii_dev, int *status_dev, void *ws, size_t ws_bytes,
                                        void *const *events, void *stream) {
  if (!a_dev || !b_dev || !kid_dev || !counts_dev || !status_dev || !ws) return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b, D, panel_rows) || a_pstride < 0 || b_pstride < 0 || a_rstride < 0 || b_rstride < 0)
    return DT_E_SHAPE;
  const int n_min = n_a < n_b ? n_a : n_b;
  if (k < 1 || k > n_min - 1 || k > DT_QUALITY_STREAM_MAX_K) return DT_E_SHAPE;
  if (!aligned16(a_dev, a_pstride, a_rstride) || !aligned16(b_dev, b_pstride, b_rstride) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const Layout L(P, n_a, n_b, panel_rows);
  if (ws_bytes < L.bytes(P)) return DT_E_WORKSPACE;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  const int ash = a_pstride == 0 && P > 1;
  const Job J{Rows{a_dev, b_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b}, L, (double *)((char *)ws + L.head),
              (int *)ws, D, k, ash};
  const int nta = (n_a + 63) / 64, ntb = (n_b + 63) / 64;
  qstream_diag_kernel<<<dim3(nta + ntb, P), kThreads, 0, s>>>(J, nta);
  DT_LAUNCH_CHECK();
  qstream_flag_kernel<<<P, kThreads, 0, s>>>(J);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[1], s));
  // the two sides: A x A (one problem if A is shared), then B x B
  for (int set = 0; set < 2; ++set) {
    const int n = set ? n_b : n_a, nt = set ? ntb : nta, Ps = set == 0 && ash ? 1 : P;
    for (int r0 = 0; r0 < n; r0 += panel_rows) {
      const int rows = n - r0 < panel_rows ? n - r0 : panel_rows;
      qstream_gram_kernel<<<dim3((rows + 63) / 64 * nt, Ps), kThreads, 0, s>>>(J, set, set, r0, rows, nt);
      DT_LAUNCH_CHECK();
      qstream_select_kernel<<<dim3(rows, Ps), kWave, 0, s>>>(J, set, r0);
      DT_LAUNCH_CHECK();
      qstream_kappa_kernel<<<dim3(rows, Ps), kWave, 0, s>>>(J, set, r0);
      DT_LAUNCH_CHECK();
    }
    if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[2 + set], s));
  }
  for (int r0 = 0; r0 < n_a; r0 += panel_rows) {
    const int rows = n_a - r0 < panel_rows ? n_a - r0 : panel_rows;
    qstream_gram_kernel<<<dim3((rows + 63) / 64 * ntb, P), kThreads, 0, s>>>(J, 0, 1, r0, rows, ntb);
    DT_LAUNCH_CHECK();
    qstream_count_rows_kernel<<<dim3(rows, P), kWave, 0, s>>>(J, r0);
    DT_LAUNCH_CHECK();
    qstream_count_cols_kernel<<<dim3(ntb, P), kThreads, 0, s>>>(J, r0, rows);
    DT_LAUNCH_CHECK();
    qstream_kappa_kernel<<<dim3(rows, P), kWave, 0, s>>>(J, 2, r0);
    DT_LAUNCH_CHECK();
  }
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[4], s));
  qstream_finish_kernel<<<P, kThreads, 0, s>>>(J, kid_dev, counts_dev, radii_dev, status_dev);
  DT_LAUNCH_CHECK();
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[5], s));
  return DT_OK;
}
