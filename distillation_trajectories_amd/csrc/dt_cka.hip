// Layer-wise centered kernel alignment (include/dt_hip_cka.h): feature-centred fp64 Grams of pitched fp32 layers, what
// the scores need of each Gram alone, and the biased and debiased linear CKA of every pair of layers.
//
// cka_mean_kernel     one thread per feature: the rows in order, one division.  Flags a NaN or Inf.
// cka_gram_kernel     one 64 x 64 tile of the upper triangle of one slab of DT_CKA_SLAB features per workgroup: tile_product
//                     (dt_dense64.h) on a loader that walks the groups of a row and centres as it loads, float4 where base,
//                     strides, pitch and c allow and by element otherwise (the same values, the same chain).  The slab's tile
//                     goes to the workspace whole.
// cka_reduce_kernel   cell = (0.0 or what the earlier slabs left) + the slabs of this turn in index order; mirrored store.
// cka_rows_kernel     one workgroup per row: the sum of its off-diagonal cells (fixed tree); NaN fill of a flagged layer.
// cka_finish_kernel   one workgroup per layer: total, trace, and the self terms by pair_terms with L = K; the status word.
// cka_scores_kernel   one workgroup per pair: pair_terms, the two estimators.
// No atomics and plain vector stores throughout: every sum has one order.
#include <math.h>

#include "../../include/dt_hip_cka.h"
#include "dt_dense64.h"

namespace {

constexpr int kTileCells = 64 * 64;
constexpr int kFillGroups = 2048;   // workgroups of the Gram kernel that the full-width workspace keeps in flight
constexpr int kMaxTurn = 4096;      // slabs per launch at the most (grid.y)

struct Layer {
  const float *base;
  long long rs;
  int groups, c, pitch, p;
};

__device__ inline long long feature_offset(const Layer &Ly, int k) {
  const int g = k / Ly.c;
  return (long long)g * Ly.pitch + (k - g * Ly.c);
}

__global__ __launch_bounds__(kThreads) void cka_mean_kernel(Layer Ly, int n, double *__restrict__ mean,
                                                            int *__restrict__ status) {
  const int k = blockIdx.x * kThreads + threadIdx.x;
  if (k >= Ly.p) return;
  const float *col = Ly.base + feature_offset(Ly, k);
  double s = 0.0;
  bool bad = false;
  for (int i = 0; i < n; ++i) {
    const float x = col[i * Ly.rs];
    bad |= !isfinite(x);
    s += (double)x;
  }
  mean[k] = s / (double)n;
  if (bad) *status = DT_CKA_NONFINITE;   // every writer stores the same word
}

// Loader for tile_product: features k0 + k .. of a pitched row (nullptr: no such row), centred; 0.0 from kend on.
// WIDTH 4 needs c, pitch and the row's address in floats to be multiples of 4: a quad then lies inside one group.
template <int WIDTH>
struct PitchedRow {
  const float *row;
  const double *mean;
  Layer Ly;
  int k0, kend;
  static constexpr int W = WIDTH;
  __device__ void operator()(int k, double (&v)[WIDTH]) const {
#pragma unroll
    for (int i = 0; i < WIDTH; ++i) v[i] = 0.0;
    const int f = k0 + k;
    if (row && f < kend) {
      const float *src = row + feature_offset(Ly, f);
      if constexpr (WIDTH == 4) {
        const float4 x = *reinterpret_cast<const float4 *>(src);
        v[0] = (double)x.x - mean[f]; v[1] = (double)x.y - mean[f + 1];
        v[2] = (double)x.z - mean[f + 2]; v[3] = (double)x.w - mean[f + 3];
      } else {
        v[0] = (double)*src - mean[f];
      }
    }
  }
};

// part: [slabs of the turn][upper tiles][64][64]
template <int WIDTH>
__global__ __launch_bounds__(kThreads) void cka_gram_kernel(Layer Ly, int n, int nt, int slab0, const double *__restrict__ mean,
                                                            double *__restrict__ part) {
  int bi, bj;
  upper_tile(blockIdx.x, nt, bi, bj);
  const int lr = threadIdx.x / 4, lq = threadIdx.x % 4;
  const int ra = bi * 64 + lr, rb = bj * 64 + lr;
  const int k0 = (slab0 + blockIdx.y) * DT_CKA_SLAB;
  const int kend = k0 + DT_CKA_SLAB < Ly.p ? k0 + DT_CKA_SLAB : Ly.p;
  const PitchedRow<WIDTH> la{ra < n ? Ly.base + ra * Ly.rs : nullptr, mean, Ly, k0, kend};
  const PitchedRow<WIDTH> lb{rb < n ? Ly.base + rb * Ly.rs : nullptr, mean, Ly, k0, kend};
  double *out = part + ((size_t)blockIdx.y * gridDim.x + blockIdx.x) * kTileCells;
  double acc[4][4] = {};
  tile_product(kend - k0, lr, lq, la, lb, acc);
  const int tx = threadIdx.x % 16, ty = threadIdx.x / 16;
#pragma unroll
  for (int u = 0; u < 4; ++u)
#pragma unroll
    for (int w = 0; w < 4; ++w) out[(ty + 16 * u) * 64 + tx + 16 * w] = acc[u][w];
}

// grid (upper tiles, 16): one cell per thread
__global__ __launch_bounds__(kThreads) void cka_reduce_kernel(int n, int nt, int count, int first, const double *__restrict__ part,
                                                              double *__restrict__ gram) {
  int bi, bj;
  upper_tile(blockIdx.x, nt, bi, bj);
  const int cell = blockIdx.y * kThreads + threadIdx.x;
  const int r = bi * 64 + cell / 64, c = bj * 64 + cell % 64;
  if (r >= n || c >= n) return;
  double acc = first ? 0.0 : gram[(size_t)r * n + c];
  for (int s = 0; s < count; ++s) acc += part[((size_t)s * gridDim.x + blockIdx.x) * kTileCells + cell];
  gram[(size_t)r * n + c] = acc;
  if (bi != bj) gram[(size_t)c * n + r] = acc;
}

// grid (n, L)
__global__ __launch_bounds__(kThreads) void cka_rows_kernel(int n, double *__restrict__ gram, double *__restrict__ sums,
                                                            const int *__restrict__ status) {
  __shared__ double red[kThreads];
  const int i = blockIdx.x, l = blockIdx.y;
  double *row = gram + ((size_t)l * n + i) * n;
  const bool bad = status[l] & DT_CKA_NONFINITE;
  double s = 0.0;
  for (int j = threadIdx.x; j < n; j += kThreads) {
    if (bad) row[j] = __builtin_nan("");
    else if (j != i) s += row[j];
  }
  const double r = block_sum(s, red);
  if (threadIdx.x == 0) sums[(size_t)l * DT_CKA_SUMS + DT_CKA_SUM_ROWS + i] = bad ? __builtin_nan("") : r;
}

// What a pair of Grams contributes: <K, L> over all cells, over the off-diagonal cells, and (K~1)'(L~1).  One workgroup;
// each thread's share is one FMA chain in a fixed order, the shares meet in block_sum's tree.  Products commute, so
// (K, L) and (L, K) give the same bits, and (K, K) is the self term.
struct PairTerms {
  double all, off, dot;
};

__device__ PairTerms pair_terms(const double *K, const double *rK, const double *L, const double *rL, int n, double *red) {
  double a = 0.0, o = 0.0, d = 0.0;
  for (int i = 0; i < n; ++i) {
    const double *Ki = K + (size_t)i * n, *Li = L + (size_t)i * n;
    for (int j = threadIdx.x; j < n; j += kThreads) {
      const double x = Ki[j], y = Li[j];
      a = fma(x, y, a);
      if (j != i) o = fma(x, y, o);
    }
  }
  for (int i = threadIdx.x; i < n; i += kThreads) d = fma(rK[i], rL[i], d);
  PairTerms t;
  t.all = block_sum(a, red);
  t.off = block_sum(o, red);
  t.dot = block_sum(d, red);
  return t;
}

// HSIC1 of Song et al. from <K~, L~>, the two totals 1'K~1 and 1'L~1, and (K~1)'(L~1); symmetric in the two Grams
__device__ inline double hsic1(double off, double total_k, double total_l, double dot, int n) {
#pragma clang fp contract(off)
  const double nn = (double)n;
  const double c1 = (total_k * total_l) / ((nn - 1.0) * (nn - 2.0));
  const double c2 = (2.0 * dot) / (nn - 2.0);
  return ((off + c1) - c2) / (nn * (nn - 3.0));
}

// grid L
__global__ __launch_bounds__(kThreads) void cka_finish_kernel(int n, const double *__restrict__ gram, double *__restrict__ sums,
                                                              int *__restrict__ status) {
  __shared__ double red[kThreads];
  const int l = blockIdx.x, t = threadIdx.x;
  const double *K = gram + (size_t)l * n * n;
  double *S = sums + (size_t)l * DT_CKA_SUMS, *R = S + DT_CKA_SUM_ROWS;
  for (int i = n + t; i < DT_CKA_MAX_N; i += kThreads) R[i] = 0.0;
  if (status[l] & DT_CKA_NONFINITE) {   // uniform
    if (t < DT_CKA_SUM_ROWS) S[t] = t <= DT_CKA_SUM_HSIC1 ? __builtin_nan("") : 0.0;
    return;
  }
  double st = 0.0, sd = 0.0;
  for (int i = t; i < n; i += kThreads) {
    st += R[i];
    sd += K[(size_t)i * n + i];
  }
  const double total = block_sum(st, red), trace = block_sum(sd, red);
  const PairTerms self = pair_terms(K, R, K, R, n, red);
  const double h = hsic1(self.off, total, total, self.dot, n);
  if (t == 0) {
    S[DT_CKA_SUM_ALL] = self.all;
    S[DT_CKA_SUM_OFF] = self.off;
    S[DT_CKA_SUM_TOTAL] = total;
    S[DT_CKA_SUM_TRACE] = trace;
    S[DT_CKA_SUM_HSIC1] = h;
    S[5] = S[6] = S[7] = 0.0;
    status[l] = self.all == 0.0 ? DT_CKA_ZERO_VARIANCE : (h > 0.0 ? 0 : DT_CKA_SELF_NOT_POSITIVE);
  }
}

// grid (Lb, La)
__global__ __launch_bounds__(kThreads) void cka_scores_kernel(const double *__restrict__ gram_a, const double *__restrict__ sums_a,
                                                              const int *__restrict__ status_a, const double *__restrict__ gram_b,
                                                              const double *__restrict__ sums_b, const int *__restrict__ status_b,
                                                              int n, double *__restrict__ cka, double *__restrict__ unbiased,
                                                              double *__restrict__ hsic) {
#pragma clang fp contract(off)
  __shared__ double red[kThreads];
  const int ia = blockIdx.y, ib = blockIdx.x;
  const double *Sa = sums_a + (size_t)ia * DT_CKA_SUMS, *Sb = sums_b + (size_t)ib * DT_CKA_SUMS;
  const PairTerms x = pair_terms(gram_a + (size_t)ia * n * n, Sa + DT_CKA_SUM_ROWS, gram_b + (size_t)ib * n * n,
                                 Sb + DT_CKA_SUM_ROWS, n, red);
  if (threadIdx.x != 0) return;
  const double h = hsic1(x.off, Sa[DT_CKA_SUM_TOTAL], Sb[DT_CKA_SUM_TOTAL], x.dot, n);
  const int st = status_a[ia] | status_b[ib];
  const size_t pair = (size_t)ia * gridDim.x + ib;
  const double nan = __builtin_nan("");
  cka[pair] = st & (DT_CKA_NONFINITE | DT_CKA_ZERO_VARIANCE) ? nan : x.all / sqrt(Sa[DT_CKA_SUM_ALL] * Sb[DT_CKA_SUM_ALL]);
  unbiased[pair] =
      st ? nan : h / sqrt(Sa[DT_CKA_SUM_HSIC1] * Sb[DT_CKA_SUM_HSIC1]);
  if (hsic) {
    hsic[2 * pair] = x.all;
    hsic[2 * pair + 1] = h;
  }
}

// ---------------------------------------------------------------------------------------------- host
bool shape_ok(int L, int n) { return L >= 1 && L <= DT_CKA_MAX_LAYERS && n >= DT_CKA_MIN_N && n <= DT_CKA_MAX_N; }

// a call's share of a workspace: [means of one layer][slab tiles of one turn]
struct Layout {
  size_t head, per_slab;
  int ntiles, nt, slabs, fill;   // slabs of the widest layer; turn length that fills the device
  Layout(int n, int p_max) {
    nt = (n + 63) / 64;
    ntiles = nt * (nt + 1) / 2;
    head = ((size_t)p_max * sizeof(double) + 255) / 256 * 256;
    per_slab = (size_t)ntiles * kTileCells * sizeof(double);
    slabs = (p_max + DT_CKA_SLAB - 1) / DT_CKA_SLAB;
    const int want = (kFillGroups + ntiles - 1) / ntiles;
    fill = slabs < want ? slabs : want;
  }
};

// DT_OK and the widest layer's features, or the error of the first layer that is out of the limits
int check_layers(const float *const *base, const long long *rs, const int *groups, const int *c, const int *pitch, int L,
                 int *p_max) {
  for (int l = 0; l < L; ++l) {
    if (!base[l]) return DT_E_NULL;
    if (groups[l] < 1 || c[l] < 1 || c[l] > pitch[l] || rs[l] < 0 || (long long)groups[l] * c[l] > DT_CKA_MAX_P) return DT_E_SHAPE;
    if ((uintptr_t)base[l] & 3) return DT_E_ARG;
    const int p = groups[l] * c[l];
    if (p > *p_max) *p_max = p;
  }
  return DT_OK;
}

int check_outputs(const double *gram, const double *sums, const int *status) {
  if (!gram || !sums || !status) return DT_E_NULL;
  if (((uintptr_t)gram & 7) || ((uintptr_t)sums & 7) || ((uintptr_t)status & 3)) return DT_E_ARG;
  return DT_OK;
}

int check_workspace(const void *ws, size_t ws_bytes, int n, int p_max) {
  if (!ws) return DT_E_NULL;
  if ((uintptr_t)ws & 15) return DT_E_ARG;
  const Layout W(n, p_max);
  return ws_bytes < W.head + W.per_slab ? DT_E_WORKSPACE : DT_OK;
}

// arguments already checked
int launch_gram(const float *const *base, const long long *rs, const int *groups, const int *c, const int *pitch, int L, int n,
                int p_max, double *gram, double *sums, int *status, void *ws, size_t ws_bytes, hipStream_t s) {
  const Layout W(n, p_max);
  size_t fit = (ws_bytes - W.head) / W.per_slab;
  const int turn = fit < (size_t)kMaxTurn ? (int)fit : kMaxTurn;
  double *mean = (double *)ws, *part = (double *)((char *)ws + W.head);
  DT_HIP_TRY(hipMemsetAsync(status, 0, (size_t)L * sizeof(int), s));
  for (int l = 0; l < L; ++l) {
    const Layer Ly{base[l], rs[l], groups[l], c[l], pitch[l], groups[l] * c[l]};
    double *K = gram + (size_t)l * n * n;
    cka_mean_kernel<<<(Ly.p + kThreads - 1) / kThreads, kThreads, 0, s>>>(Ly, n, mean, status + l);
    DT_LAUNCH_CHECK();
    const bool quads = aligned16(Ly.base, Ly.rs, Ly.pitch) && Ly.c % 4 == 0;
    const int slabs = (Ly.p + DT_CKA_SLAB - 1) / DT_CKA_SLAB;
    for (int s0 = 0; s0 < slabs; s0 += turn) {
      const int count = slabs - s0 < turn ? slabs - s0 : turn;
      const dim3 grid(W.ntiles, count);
      if (quads) cka_gram_kernel<4><<<grid, kThreads, 0, s>>>(Ly, n, W.nt, s0, mean, part);
      else cka_gram_kernel<1><<<grid, kThreads, 0, s>>>(Ly, n, W.nt, s0, mean, part);
      DT_LAUNCH_CHECK();
      cka_reduce_kernel<<<dim3(W.ntiles, kTileCells / kThreads), kThreads, 0, s>>>(n, W.nt, count, s0 == 0, part, K);
      DT_LAUNCH_CHECK();
    }
  }
  cka_rows_kernel<<<dim3(n, L), kThreads, 0, s>>>(n, gram, sums, status);
  DT_LAUNCH_CHECK();
  cka_finish_kernel<<<L, kThreads, 0, s>>>(n, gram, sums, status);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int launch_scores(const double *gram_a, const double *sums_a, const int *status_a, int La, const double *gram_b,
                  const double *sums_b, const int *status_b, int Lb, int n, double *cka, double *unbiased, double *hsic,
                  hipStream_t s) {
  cka_scores_kernel<<<dim3(Lb, La), kThreads, 0, s>>>(gram_a, sums_a, status_a, gram_b, sums_b, status_b, n, cka, unbiased, hsic);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

int check_scores(const double *cka, const double *unbiased, const double *hsic) {
  if (!cka || !unbiased) return DT_E_NULL;
  if (((uintptr_t)cka & 7) || ((uintptr_t)unbiased & 7) || ((uintptr_t)hsic & 7)) return DT_E_ARG;
  return DT_OK;
}

}  // namespace

extern "C" size_t dt_cka_workspace_bytes(int L, int n, int p_max) {
  if (!shape_ok(L, n) || p_max < 1 || p_max > DT_CKA_MAX_P) return 0;
  const Layout W(n, p_max);
  return W.head + (size_t)W.fill * W.per_slab;
}

extern "C" size_t dt_cka_min_workspace_bytes(int n, int p_max) {
  if (!shape_ok(1, n) || p_max < 1 || p_max > DT_CKA_MAX_P) return 0;
  const Layout W(n, p_max);
  return W.head + W.per_slab;
}

extern "C" int dt_cka_gram(const float *const *base_dev, const long long *row_stride, const int *groups, const int *c,
                           const int *pitch, int L, int n, double *gram_dev, double *sums_dev, int *status_dev, void *ws,
                           size_t ws_bytes, void *stream) {
  if (!base_dev || !row_stride || !groups || !c || !pitch || !gram_dev || !sums_dev || !status_dev || !ws) return DT_E_NULL;
  if (!shape_ok(L, n)) return DT_E_SHAPE;
  int p_max = 1, rc;
  if ((rc = check_layers(base_dev, row_stride, groups, c, pitch, L, &p_max)) != DT_OK) return rc;
  if ((rc = check_outputs(gram_dev, sums_dev, status_dev)) != DT_OK) return rc;
  if ((rc = check_workspace(ws, ws_bytes, n, p_max)) != DT_OK) return rc;
  return launch_gram(base_dev, row_stride, groups, c, pitch, L, n, p_max, gram_dev, sums_dev, status_dev, ws, ws_bytes,
                     (hipStream_t)stream);
}

extern "C" int dt_cka_scores(const double *gram_a_dev, const double *sums_a_dev, const int *status_a_dev, int La,
                             const double *gram_b_dev, const double *sums_b_dev, const int *status_b_dev, int Lb, int n,
                             double *cka_dev, double *cka_unbiased_dev, double *hsic_dev, void *stream) {
  if (!gram_a_dev || !sums_a_dev || !status_a_dev || !gram_b_dev || !sums_b_dev || !status_b_dev || !cka_dev || !cka_unbiased_dev)
    return DT_E_NULL;
  if (!shape_ok(La, n) || !shape_ok(Lb, n)) return DT_E_SHAPE;
  int rc;
  if ((rc = check_outputs(gram_a_dev, sums_a_dev, status_a_dev)) != DT_OK) return rc;
  if ((rc = check_outputs(gram_b_dev, sums_b_dev, status_b_dev)) != DT_OK) return rc;
  if ((rc = check_scores(cka_dev, cka_unbiased_dev, hsic_dev)) != DT_OK) return rc;
  return launch_scores(gram_a_dev, sums_a_dev, status_a_dev, La, gram_b_dev, sums_b_dev, status_b_dev, Lb, n, cka_dev,
                       cka_unbiased_dev, hsic_dev, (hipStream_t)stream);
}

extern "C" int dt_cka(const float *const *base_a_dev, const long long *row_stride_a, const int *groups_a, const int *c_a,
                      const int *pitch_a, int La, double *gram_a_dev, double *sums_a_dev, int *status_a_dev,
                      const float *const *base_b_dev, const long long *row_stride_b, const int *groups_b, const int *c_b,
                      const int *pitch_b, int Lb, double *gram_b_dev, double *sums_b_dev, int *status_b_dev, int n,
                      double *cka_dev, double *cka_unbiased_dev, double *hsic_dev, void *ws, size_t ws_bytes, void *stream) {
  const bool two = base_b_dev != nullptr;
  if (!base_a_dev || !row_stride_a || !groups_a || !c_a || !pitch_a || !gram_a_dev || !sums_a_dev || !status_a_dev || !ws)
    return DT_E_NULL;
  if (two && (!row_stride_b || !groups_b || !c_b || !pitch_b || !gram_b_dev || !sums_b_dev || !status_b_dev)) return DT_E_NULL;
  if (!cka_dev || !cka_unbiased_dev) return DT_E_NULL;
  if (!shape_ok(La, n) || (two && !shape_ok(Lb, n))) return DT_E_SHAPE;
  int p_max = 1, rc;
  if ((rc = check_layers(base_a_dev, row_stride_a, groups_a, c_a, pitch_a, La, &p_max)) != DT_OK) return rc;
  if (two && (rc = check_layers(base_b_dev, row_stride_b, groups_b, c_b, pitch_b, Lb, &p_max)) != DT_OK) return rc;
  if ((rc = check_outputs(gram_a_dev, sums_a_dev, status_a_dev)) != DT_OK) return rc;
  if (two && (rc = check_outputs(gram_b_dev, sums_b_dev, status_b_dev)) != DT_OK) return rc;
  if ((rc = check_scores(cka_dev, cka_unbiased_dev, hsic_dev)) != DT_OK) return rc;
  if ((rc = check_workspace(ws, ws_bytes, n, p_max)) != DT_OK) return rc;
  hipStream_t s = (hipStream_t)stream;
  rc = launch_gram(base_a_dev, row_stride_a, groups_a, c_a, pitch_a, La, n, p_max, gram_a_dev, sums_a_dev, status_a_dev, ws,
                   ws_bytes, s);
  if (rc != DT_OK) return rc;
  if (two) {
    rc = launch_gram(base_b_dev, row_stride_b, groups_b, c_b, pitch_b, Lb, n, p_max, gram_b_dev, sums_b_dev, status_b_dev, ws,
                     ws_bytes, s);
    if (rc != DT_OK) return rc;
    return launch_scores(gram_a_dev, sums_a_dev, status_a_dev, La, gram_b_dev, sums_b_dev, status_b_dev, Lb, n, cka_dev,
                         cka_unbiased_dev, hsic_dev, s);
  }
  return launch_scores(gram_a_dev, sums_a_dev, status_a_dev, La, gram_a_dev, sums_a_dev, status_a_dev, La, n, cka_dev,
                       cka_unbiased_dev, hsic_dev, s);
}
