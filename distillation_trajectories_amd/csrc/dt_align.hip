// Trajectory alignment (include/dt_hip_align.h): the fp64 matrix of Euclidean distances between the states of two
// trajectories, and DTW / discrete Frechet over it, for P independent problems.
//
// align_cost_kernel   one 64 x 64 tile of one problem's matrix per 256-thread workgroup; 4 x 4 cells per thread.  The rows
//                     of a and b are staged through LDS 32 elements at a time, already widened to fp64; every cell then
//                     takes acc = fma(d, d, acc), d = a_e - b_e, in the order e = 0 .. E-1.  The tail of E is staged as
//                     zeros on both sides: fma(0, 0, acc) is acc.  Plain fp64 VALU work (the part's fp64 MFMA rate is no
//                     higher), LDS-fed: per e a thread reads 8 doubles for 32 fp64 instructions.
// align_dp_kernel     one workgroup per problem, thread i owns row i and walks it one cell per anti-diagonal.  A thread reads
//                     its row of D eight cells ahead into registers (the only global reads of the walk, 64 contiguous bytes
//                     per thread and block of eight diagonals), the last three diagonals of C live in LDS, one barrier per
//                     diagonal.  The predecessor bytes of eight diagonals go out as one 8-byte word per thread.  Wave 0 then
//                     walks back, fetching the words of the rows it can reach in a block of eight diagonals at once.
#include <math.h>

#include "../../include/dt_hip_align.h"
#include "dt_internal.h"

namespace {

constexpr int kTile = 64;          // cells of a cost tile per side
constexpr int kChunk = 32;         // elements of E staged per step
constexpr int kLd = kTile + 2;     // doubles per staged element: keeps 16-byte alignment, spreads the banks
constexpr int kCostThreads = 256;
constexpr int kDiagBlock = 8;      // diagonals per predecessor word and per register panel of D
constexpr int kMaxE = 1 << 28;

struct Rows {
  const float *a, *b;
  long long a_ps, a_rs, b_ps, b_rs;
  int n_a, n_b;
};

__global__ __launch_bounds__(kCostThreads) void align_cost_kernel(Rows R, int E, double *__restrict__ cost,
                                                                  int *__restrict__ status) {
  __shared__ __attribute__((aligned(16))) double sa[kChunk][kLd];
  __shared__ __attribute__((aligned(16))) double sb[kChunk][kLd];
  const int t = threadIdx.x, p = blockIdx.z;
  const int i0 = blockIdx.y * kTile, j0 = blockIdx.x * kTile;
  const int tx = t & 15, ty = t >> 4;
  const int el = t & (kChunk - 1), r0 = t >> 5;             // staging: element el of rows r0, r0 + 8, ...
  const float *ap = R.a + (long long)p * R.a_ps, *bp = R.b + (long long)p * R.b_ps;
  float ra[8], rb[8];
  bool bad = false;
  auto fetch = [&](int e0) {
    const int e = e0 + el;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int r = r0 + 8 * k;
      ra[k] = (e < E && i0 + r < R.n_a) ? ap[(long long)(i0 + r) * R.a_rs + e] : 0.f;
      rb[k] = (e < E && j0 + r < R.n_b) ? bp[(long long)(j0 + r) * R.b_rs + e] : 0.f;
      bad |= !isfinite(ra[k]) || !isfinite(rb[k]);
    }
  };
  double acc[4][4] = {};
  fetch(0);
  for (int e0 = 0; e0 < E; e0 += kChunk) {
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      sa[el][r0 + 8 * k] = (double)ra[k];
      sb[el][r0 + 8 * k] = (double)rb[k];
    }
    __syncthreads();
    if (e0 + kChunk < E) fetch(e0 + kChunk);                // lands under the arithmetic below
#pragma unroll 4
    for (int e = 0; e < kChunk; ++e) {
      double av[4], bv[4];
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        av[q] = sa[e][ty * 4 + q];
        bv[q] = sb[e][tx * 4 + q];
      }
#pragma unroll
      for (int y = 0; y < 4; ++y)
#pragma unroll
        for (int x = 0; x < 4; ++x) {
          const double d = av[y] - bv[x];
          acc[y][x] = fma(d, d, acc[y][x]);
        }
    }
    __syncthreads();
  }
  double *cp = cost + (size_t)p * R.n_a * R.n_b;
#pragma unroll
  for (int y = 0; y < 4; ++y) {
    const int i = i0 + ty * 4 + y;
    if (i >= R.n_a) continue;
#pragma unroll
    for (int x = 0; x < 4; ++x) {
      const int j = j0 + tx * 4 + x;
      if (j < R.n_b) cp[(size_t)i * R.n_b + j] = sqrt(acc[y][x]);
    }
  }
  if (bad) status[p] = DT_ALIGN_NONFINITE;                  // every writer stores the same word
}

__device__ inline bool in_band(int i, int j, int n_a, int n_b, long long reach) {
  const long long q = (long long)i * (n_b - 1) - (long long)j * (n_a - 1);
  return (q < 0 ? -q : q) <= reach;
}

// dirs: [P] problems of dir_stride bytes, each [blocks of eight diagonals][n_a] 8-byte words, byte d & 7 of word
// (d >> 3, i) the predecessor of cell (i, d - i): 0 (i-1, j-1), 1 (i-1, j), 2 (i, j-1), 3 none.  nullptr: no path.
__global__ __launch_bounds__(1024) void align_dp_kernel(const double *__restrict__ cost, int n_a, int n_b, int kind, int band,
                                                        double *__restrict__ value, int *__restrict__ path,
                                                        int *__restrict__ path_len, int *__restrict__ status,
                                                        unsigned long long *__restrict__ dirs, size_t dir_stride) {
  __shared__ double diag[3][DT_ALIGN_MAX_N];
  __shared__ unsigned int rev[2 * DT_ALIGN_MAX_N];          // the path backwards, (i << 16) | j
  __shared__ double s_end;
  __shared__ int s_len;
  const int i = threadIdx.x, p = blockIdx.x;
  const int nd = n_a + n_b - 1, n_blocks = (nd + kDiagBlock - 1) / kDiagBlock;
  const double *D = cost + (size_t)p * n_a * n_b;
  unsigned long long *dir = dirs ? (unsigned long long *)((char *)dirs + (size_t)p * dir_stride) : nullptr;
  const bool row = i < n_a;
  const long long reach = (long long)band * (n_a > n_b ? n_a - 1 : n_b - 1);
  const double inf = __builtin_huge_val();

  double cur[kDiagBlock], nxt[kDiagBlock];
  auto fetch = [&](int g) {
#pragma unroll
    for (int k = 0; k < kDiagBlock; ++k) {
      const int j = g * kDiagBlock + k - i;
      nxt[k] = (row && j >= 0 && j < n_b) ? D[(size_t)i * n_b + j] : 0.0;
    }
  };
  bool bad = false;
  double left = 0.0;                                         // C[i][j-1]
  fetch(0);
  for (int g = 0; g < n_blocks; ++g) {
#pragma unroll
    for (int k = 0; k < kDiagBlock; ++k) cur[k] = nxt[k];
    if (g + 1 < n_blocks) fetch(g + 1);
    unsigned long long word = 0;
#pragma unroll
    for (int k = 0; k < kDiagBlock; ++k) {
      const int d = g * kDiagBlock + k;
      if (d < nd) {                                          // uniform
        const int j = d - i;
        if (row && j >= 0 && j < n_b) {
          const double c = cur[k];
          bad |= !isfinite(c);
          double *now = diag[d % 3];
          const double *prev1 = diag[(d + 2) % 3], *prev2 = diag[(d + 1) % 3];
          unsigned long long code = 3;
          double v;
          if (band > 0 && !in_band(i, j, n_a, n_b, reach)) {
            v = inf;
          } else if (d == 0) {
            v = c;
          } else {
            double m = 0.0;
            if (i > 0 && j > 0) { m = prev2[i - 1]; code = 0; }
            if (i > 0) { const double up = prev1[i - 1]; if (code == 3 || up < m) { m = up; code = 1; } }
            if (j > 0 && (code == 3 || left < m)) { m = left; code = 2; }
            v = kind == DT_ALIGN_DTW ? m + c : (c > m ? c : m);
          }
          now[i] = v;
          left = v;
          word |= code << (8 * k);
        }
        __syncthreads();
      }
    }
    if (dir && row) dir[(size_t)g * n_a + i] = word;
  }
  if (i == n_a - 1) s_end = left;
  if (i == 0) s_len = 0;
  const int any_bad = __syncthreads_or(bad ? 1 : 0);
  const double end = s_end;
  const int st = any_bad ? DT_ALIGN_NONFINITE : (isinf(end) ? DT_ALIGN_NO_PATH : DT_ALIGN_OK);
  if (i == 0) {
    value[p] = any_bad ? __builtin_nan("") : end;
    status[p] = st;
  }
  if (!path) return;                                         // uniform
  if (st == DT_ALIGN_OK && i < 64) {                         // wave 0, every lane with the same (ci, cj, len)
    int ci = n_a - 1, cj = n_b - 1, len = 0;
    bool done = false;
    while (!done) {
      const int g = (ci + cj) / kDiagBlock, top = ci;
      const int r = top - i;                                 // lane l holds row top - l of block g (a walk inside a block
      unsigned long long w = 0;                              // drops fewer than eight rows)
      if (i < kDiagBlock && r >= 0) w = dir[(size_t)g * n_a + r];
      const unsigned int lo = (unsigned int)w, hi = (unsigned int)(w >> 32);
      while (true) {
        const int d = ci + cj;
        if (i == 0) rev[len] = ((unsigned int)ci << 16) | (unsigned int)cj;
        ++len;
        if (d == 0) { done = true; break; }
        const int k = d & (kDiagBlock - 1);
        const unsigned int half = k < 4 ? __shfl(lo, top - ci) : __shfl(hi, top - ci);
        const unsigned int code = (half >> (8 * (k & 3))) & 3u;
        if (code == 3 || len >= nd) { done = true; len = 0; break; }   // (not reached: a finite end has a chain to (0, 0))
        if (code == 0) { --ci; --cj; } else if (code == 1) { --ci; } else { --cj; }
        if ((ci + cj) / kDiagBlock != g) break;
      }
    }
    if (i == 0) s_len = len;
  }
  __syncthreads();
  const int len = s_len;
  int *pp = path + (size_t)p * nd * 2;
  for (int k = i; k < nd; k += blockDim.x) {
    int pi = -1, pj = -1;
    if (k < len) {
      const unsigned int v = rev[len - 1 - k];
      pi = (int)(v >> 16);
      pj = (int)(v & 0xffffu);
    }
    pp[2 * k] = pi;
    pp[2 * k + 1] = pj;
  }
  if (i == 0) path_len[p] = len;
}

bool shape_ok(int P, int n_a, int n_b) {
  return P >= 1 && P <= 65535 && n_a >= 2 && n_a <= DT_ALIGN_MAX_N && n_b >= 2 && n_b <= DT_ALIGN_MAX_N;
}

// one problem's share of a workspace: [cost matrix unless the caller has it][predecessor words if a path is wanted]
struct Layout {
  size_t cost, dir, per;
  Layout(int n_a, int n_b, bool want_path, bool cost_given) {
    const size_t blocks = (size_t)(n_a + n_b - 1 + kDiagBlock - 1) / kDiagBlock;
    cost = cost_given ? 0 : (size_t)n_a * n_b * sizeof(double);
    dir = want_path ? blocks * n_a * sizeof(unsigned long long) : 0;
    per = cost + dir ? (cost + dir + 15) / 16 * 16 : 16;
  }
};

int launch_cost(const Rows &R, int P, int E, double *cost, int *status, hipStream_t s) {
  DT_HIP_TRY(hipMemsetAsync(status, 0, (size_t)P * sizeof(int), s));
  const dim3 grid((R.n_b + kTile - 1) / kTile, (R.n_a + kTile - 1) / kTile, P);
  align_cost_kernel<<<grid, kCostThreads, 0, s>>>(R, E, cost, status);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int launch_dp(const double *cost, int P, int n_a, int n_b, int kind, int band, double *value, int *path, int *path_len,
              int *status, void *dirs, size_t dir_stride, hipStream_t s) {
  const int threads = (n_a + 63) / 64 * 64;
  align_dp_kernel<<<P, threads, 0, s>>>(cost, n_a, n_b, kind, band, value, path, path_len, status,
                                         path ? (unsigned long long *)dirs : nullptr, dir_stride);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace

extern "C" size_t dt_align_workspace_bytes(int P, int n_a, int n_b, int want_path, int cost_given) {
  if (!shape_ok(P, n_a, n_b)) return 0;
  return (size_t)P * Layout(n_a, n_b, want_path != 0, cost_given != 0).per;
}

extern "C" size_t dt_align_min_workspace_bytes(int n_a, int n_b, int want_path, int cost_given) {
  return dt_align_workspace_bytes(1, n_a, n_b, want_path, cost_given);
}

extern "C" int dt_align_cost(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev,
                             int n_b, long long b_pstride, long long b_rstride, int P, int E, double *cost_dev,
                             int *status_dev, void *stream) {
  if (!a_dev || !b_dev || !cost_dev || !status_dev) return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b) || E < 1 || E > kMaxE) return DT_E_SHAPE;
  if (((uintptr_t)a_dev & 3) || ((uintptr_t)b_dev & 3) || ((uintptr_t)cost_dev & 7) || ((uintptr_t)status_dev & 3))
    return DT_E_ARG;
  const Rows R{a_dev, b_dev, a_pstride, a_rstride, b_pstride, b_rstride, n_a, n_b};
  return launch_cost(R, P, E, cost_dev, status_dev, (hipStream_t)stream);
}

extern "C" int dt_align_dp(const double *cost_dev, int P, int n_a, int n_b, int kind, int band, double *value_dev,
                           int *path_dev, int *path_len_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream) {
  if (!cost_dev || !value_dev || !status_dev || !ws) return DT_E_NULL;
  if ((path_dev == nullptr) != (path_len_dev == nullptr)) return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b)) return DT_E_SHAPE;
  if ((kind != DT_ALIGN_DTW && kind != DT_ALIGN_FRECHET) || band < 0 || band > DT_ALIGN_MAX_BAND ||
      ((uintptr_t)cost_dev & 7) || ((uintptr_t)value_dev & 7) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const Layout L(n_a, n_b, path_dev != nullptr, true);
  if (ws_bytes < (size_t)P * L.per) return DT_E_WORKSPACE;
  return launch_dp(cost_dev, P, n_a, n_b, kind, band, value_dev, path_dev, path_len_dev, status_dev, ws, L.per,
                   (hipStream_t)stream);
}

extern "C" int dt_align(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
                        long long b_pstride, long long b_rstride, int P, int E, int kind_mask, int band,
                        double *cost_out_dev, double *dtw_dev, double *frechet_dev, int *dtw_path_dev,
                        int *dtw_path_len_dev, int *frechet_path_dev, int *frechet_path_len_dev, int *status_dev, void *ws,
                        size_t ws_bytes, void *stream) {
  const bool want_dtw = kind_mask & DT_ALIGN_MASK_DTW, want_fr = kind_mask & DT_ALIGN_MASK_FRECHET;
  if (!a_dev || !b_dev || !status_dev || !ws || (want_dtw && !dtw_dev) || (want_fr && !frechet_dev)) return DT_E_NULL;
  if ((dtw_path_dev == nullptr) != (dtw_path_len_dev == nullptr) ||
      (frechet_path_dev == nullptr) != (frechet_path_len_dev == nullptr))
    return DT_E_NULL;
  if (!shape_ok(P, n_a, n_b) || E < 1 || E > kMaxE) return DT_E_SHAPE;
  if (kind_mask < 1 || kind_mask > (DT_ALIGN_MASK_DTW | DT_ALIGN_MASK_FRECHET) || band < 0 || band > DT_ALIGN_MAX_BAND ||
      (dtw_path_dev && !want_dtw) || (frechet_path_dev && !want_fr) || ((uintptr_t)a_dev & 3) || ((uintptr_t)b_dev & 3) ||
      ((uintptr_t)cost_out_dev & 7) || ((uintptr_t)dtw_dev & 7) || ((uintptr_t)frechet_dev & 7) || ((uintptr_t)ws & 15))
    return DT_E_ARG;
  const bool want_path = dtw_path_dev || frechet_path_dev;
  const Layout L(n_a, n_b, want_path, cost_out_dev != nullptr);
  if (ws_bytes < L.per) return DT_E_WORKSPACE;
  const size_t fit = ws_bytes / L.per;
  const int chunk = fit < (size_t)P ? (int)fit : P;
  hipStream_t s = (hipStream_t)stream;
  const size_t cells = (size_t)n_a * n_b, path_ints = (size_t)(n_a + n_b - 1) * 2;
  for (int p0 = 0; p0 < P; p0 += chunk) {
    const int c = P - p0 < chunk ? P - p0 : chunk;
    // the chunk's share of the workspace: [c cost matrices][c predecessor tables]; the kinds run one after the other on the
    // stream and take turns with the tables
    double *cost = cost_out_dev ? cost_out_dev + (size_t)p0 * cells : (double *)ws;
    void *dirs = (char *)ws + (size_t)c * L.cost;
    const Rows R{a_dev + (long long)p0 * a_pstride, b_dev + (long long)p0 * b_pstride, a_pstride, a_rstride, b_pstride,
                 b_rstride, n_a, n_b};
    int rc = launch_cost(R, c, E, cost, status_dev + p0, s);
    if (rc != DT_OK) return rc;
    if (want_dtw) {
      rc = launch_dp(cost, c, n_a, n_b, DT_ALIGN_DTW, band, dtw_dev + p0,
                     dtw_path_dev ? dtw_path_dev + (size_t)p0 * path_ints : nullptr,
                     dtw_path_dev ? dtw_path_len_dev + p0 : nullptr, status_dev + p0, dirs, L.dir, s);
      if (rc != DT_OK) return rc;
    }
    if (want_fr) {
      rc = launch_dp(cost, c, n_a, n_b, DT_ALIGN_FRECHET, band, frechet_dev + p0,
                     frechet_path_dev ? frechet_path_dev + (size_t)p0 * path_ints : nullptr,
                     frechet_path_dev ? frechet_path_len_dev + p0 : nullptr, status_dev + p0, dirs, L.dir, s);
      if (rc != DT_OK) return rc;
    }
  }
  return DT_OK;
}
