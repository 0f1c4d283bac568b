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
// The work of a wave on a Gram row and the finish are those of dt_quality_math.h, shared with dt_quality.hip: the same
// definitions and the same orders of summation because they are the same functions.
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
  size_t panel;
  ScoreTail tail;
  __host__ __device__ Layout(int P, int n_a, int n_b, int panel_rows) {
    head = flag_head_bytes(2 * P);
    const size_t na = (size_t)n_a, nb = (size_t)n_b;
    panel = 0;                        // [panel_rows][columns of the matrix the panel is of]
    per = tail.place(panel + (size_t)panel_rows * (na > nb ? na : nb), na, nb);
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
  double *diag = part_of(J, p) + J.L.tail.diag + (second ? J.R.n_a : 0);
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
  const double *da = a_part_of(J, p) + J.L.tail.diag, *db = part_of(J, p) + J.L.tail.diag + n_a;
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
// One wave per row of the panel of d2(A, A) (set 0) or d2(B, B) (set 1); a key is dist2_key (dt_quality_math.h).  The
// wave keeps a threshold T, at first above every key, and appends a key to the LDS buffer only if it is < T.  When the
// buffer cannot take another step's keys, t = the (k+1)-th smallest of the buffer (select_key) becomes T and the buffer
// shrinks to its keys < t (at most k) plus as many copies of t as make k + 1 entries.  A dropped key is >= T, and at
// least k + 1 entries <= T stay in the buffer, so the (k+1)-th smallest of the buffer is always that of the keys seen so
// far, duplicates counted: the result is exact and depends on nothing but the row's keys.  k + 1 <= 1024 entries leave
// room for a step after every refill.
__global__ __launch_bounds__(kWave) void qstream_select_kernel(Job J, int set, int r0) {
  __shared__ unsigned long long buf[kBuf];
  const int p = blockIdx.y;
  if (J.flag[2 * p] | (set ? J.flag[2 * p + 1] : 0)) return;
  const int n = set ? J.R.n_b : J.R.n_a, off = set ? J.R.n_a : 0, k = J.k;
  double *base = part_of(J, p);
  const int i = r0 + blockIdx.x, lane = threadIdx.x;
  const double *G = base + J.L.panel + (size_t)blockIdx.x * n;
  const double *dg = base + J.L.tail.diag + off;
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
      key[u] = j < n ? dist2_key(gi, dg[j], G[j]) : none;
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
  if (lane == 0) base[J.L.tail.r2 + off + i] = __longlong_as_double((long long)r);
}

// ---------------------------------------------------------------------------------------------- 3. kernel sums
// One wave per row of the panel; kind 0: A x A, 1: B x B (both without the diagonal entry, skipped by index), 2: A x B
// (kappa_row_sum: a row's sum does not depend on the panel it fell into).
__global__ __launch_bounds__(kWave) void qstream_kappa_kernel(Job J, int kind, int r0) {
  const int p = blockIdx.y;
  if (J.flag[2 * p] | (kind ? J.flag[2 * p + 1] : 0)) return;
  const int n_a = J.R.n_a, n_b = J.R.n_b, n = kind ? n_b : n_a;
  double *base = part_of(J, p);
  const int i = r0 + blockIdx.x, skip = kind < 2 ? i : -1;
  const double s = kappa_row_sum(base + J.L.panel + (size_t)blockIdx.x * n, n, skip, (double)J.D);
  if (threadIdx.x == 0) base[J.L.tail.rs + (kind == 0 ? 0 : kind == 1 ? n_a : n_a + n_b) + i] = s;
}

// ---------------------------------------------------------------------------------------------- 4. counts
// One wave per row i of the panel of A x B: the recall flag and the density count (count_row).
__global__ __launch_bounds__(kWave) void qstream_count_rows_kernel(Job J, int r0) {
  const int p = blockIdx.y;
  if (bad_problem(J, p)) return;
  const int n_a = J.R.n_a, n_b = J.R.n_b;
  double *base = part_of(J, p);
  const double *abase = a_part_of(J, p);
  const int i = r0 + blockIdx.x;
  int *hits = reinterpret_cast<int *>(base + J.L.tail.hits);
  count_row(base + J.L.panel + (size_t)blockIdx.x * n_b, n_b, abase[J.L.tail.diag + i], abase[J.L.tail.r2 + i],
            base + J.L.tail.diag + n_a, base + J.L.tail.r2 + n_a, hits + i, hits + n_a + i);
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
  const double *ga = abase + J.L.tail.diag, *ra = abase + J.L.tail.r2, *G = base + J.L.panel;
  const int w = threadIdx.x / kWave, lane = threadIdx.x % kWave, j = blockIdx.x * kWave + lane;
  int reached = 0;
  if (j < n_b) {
    const double gj = base[J.L.tail.diag + n_a + j];
    for (int r = w; r < rows; r += kThreads / kWave)
      reached |= dist2(ga[r0 + r], gj, G[(size_t)r * n_b + j]) < ra[r0 + r];
  }
  part[w][lane] = reached;
  __syncthreads();
  if (w == 0 && j < n_b) {
    int *word = reinterpret_cast<int *>(base + J.L.tail.hits) + 2 * n_a + j;
    const int all = part[0][lane] | part[1][lane] | part[2][lane] | part[3][lane];
    *word = r0 == 0 ? all : (*word | all);
  }
}

// ---------------------------------------------------------------------------------------------- 5. finish
__global__ __launch_bounds__(kThreads) void qstream_finish_kernel(Job J, double *kid_out, long long *counts_out,
                                                                  double *radii_out, int *status_out) {
  const int p = blockIdx.x;
  score_finish(bad_problem(J, p), J.R.n_a, J.R.n_b, J.L.tail, a_part_of(J, p), part_of(J, p), kid_out, 1, counts_out,
               radii_out, status_out);
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
  if (!shape_ok(P, n_a, n_b, D, panel_rows)) return DT_E_SHAPE;
  const int n_min = n_a < n_b ? n_a : n_b;
  if (k < 1 || k > n_min - 1 || k > DT_QUALITY_STREAM_MAX_K) return DT_E_SHAPE;
  const Layout L(P, n_a, n_b, panel_rows);
  const auto [rc, R, flag, wd] = set_pair_open(a_dev, n_a, a_pstride, a_rstride, b_dev, n_b, b_pstride, b_rstride, ws,
                                               ws_bytes, L.bytes(P), L.head);
  if (rc) return rc;
  hipStream_t s = (hipStream_t)stream;
  if (events) DT_HIP_TRY(hipEventRecord((hipEvent_t)events[0], s));
  const int ash = a_pstride == 0 && P > 1;
  const Job J{R, L, wd, flag, D, k, ash};
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
