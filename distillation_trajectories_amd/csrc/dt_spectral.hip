// Spatial-frequency spectra of trajectory states (include/dt_hip_spectral.h): per-band power of one set of pictures, and
// per-band power, cross-spectrum and difference spectrum of a teacher set against a student set, in fp64 from fp32 rows
// read in place through two strides.
//
// spectral_order_kernel  one workgroup per call: the cells of the caller's bin table sorted by bin, each bin's cells in index
//                        order (a counting sort, one thread per bin), into the workspace.
// spectral_kernel        one workgroup per row.  It looks for a NaN or Inf in the whole row first (such a row is filled with
//                        NaN and left), forms the two twiddle tables, and then takes the row's channels in turn: the picture(s)
//                        go to LDS as fp32 at a pitch of W + 1, and each of A, B and Delta = double(a) - double(b) is a direct
//                        separable DFT of the columns v <= W/2, along x into LDS (lanes along y: the twiddle is one broadcast
//                        read), then along y into registers (lanes along v: again one broadcast twiddle), one chain of fused
//                        multiply-adds per coefficient.  A thread keeps the coefficients of its <= kMaxCells cells of A and B
//                        and forms the per-cell products from them; value by value these go to an LDS plane of all H x W
//                        cells (the conjugate half filled in from the computed half), and one wave per bin adds the bin's
//                        cells: 64 partial sums in cell order, then a fixed butterfly.
// spectral_sum_kernel    one thread per element of the sample sum: the rows in index order, flagged rows skipped.
// No atomics and plain vector stores throughout: every sum has one order.
#include <math.h>

#include "../../include/dt_hip_spectral.h"
#include "dt_internal.h"

using namespace dt;

namespace {

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;
constexpr int kMaxHW = DT_SPECTRAL_MAX_HW;
// cells of the half spectrum a thread owns at the most
constexpr int kMaxCells = (kMaxHW * (kMaxHW / 2 + 1) + kThreads - 1) / kThreads;
constexpr size_t kStartBytes = ((DT_SPECTRAL_MAX_BINS + 1) * sizeof(int) + 15) / 16 * 16;

struct RowSet {
  const float *base;
  long long ostride, istride;
};

// the dynamic LDS of spectral_kernel, in bytes from its start: [twiddles W][twiddles H][T: H x Wh complex | plane: H x W][a][b]
struct Lds {
  int Wh, pitch;
  size_t tw_h, t, ra, rb, bytes;
  __host__ __device__ Lds(int H, int W, bool pair) {
    Wh = W / 2 + 1;
    pitch = W + 1;
    tw_h = (size_t)W * sizeof(double2);
    t = tw_h + (size_t)H * sizeof(double2);
    ra = t + (size_t)H * Wh * sizeof(double2);
    rb = ra + (size_t)H * pitch * sizeof(float);
    bytes = pair ? rb + (size_t)H * pitch * sizeof(float) : rb;
  }
};

__global__ __launch_bounds__(kThreads) void spectral_order_kernel(const int *__restrict__ bin, int cells, int n_bins,
                                                                  int *__restrict__ start, int *__restrict__ order) {
  __shared__ int first[DT_SPECTRAL_MAX_BINS + 1];
  const int b = threadIdx.x;
  int count = 0;
  if (b < n_bins)
    for (int i = 0; i < cells; ++i) count += bin[i] == b;
  first[b + 1] = count;   // (kThreads == DT_SPECTRAL_MAX_BINS)
  __syncthreads();
  if (b == 0) {
    first[0] = 0;
    for (int k = 0; k < n_bins; ++k) first[k + 1] += first[k];
  }
  __syncthreads();
  if (b == 0) start[n_bins] = first[n_bins];
  if (b < n_bins) {
    start[b] = first[b];
    int p = first[b];
    for (int i = 0; i < cells; ++i)
      if (bin[i] == b) order[p++] = i;
  }
}

template <int MODE>
__device__ inline double pixel(const float *ra, const float *rb, int i) {
  if constexpr (MODE == 0) return (double)ra[i];
  else if constexpr (MODE == 1) return (double)rb[i];
  else return (double)ra[i] - (double)rb[i];   // exact in fp64
}

// The half spectrum of picture MODE (0 a, 1 b, 2 a - b): F[j] is the coefficient of cell threadIdx.x + j*kThreads of
// [H][Wh].  Begins with a barrier (the pictures are in LDS, T is free) and leaves T in use by the column walk.
template <int MODE>
__device__ inline void transform(int H, int W, const Lds &L, const double2 *tw_w, const double2 *tw_h, double2 *T,
                                 const float *ra, const float *rb, double2 (&F)[kMaxCells]) {
  const int Wh = L.Wh, half = H * Wh;
  __syncthreads();
  for (int idx = threadIdx.x; idx < half; idx += kThreads) {
    const int v = idx / H, y = idx - v * H;
    double re = 0.0, im = 0.0;
    int k = 0;
    for (int x = 0; x < W; ++x) {
      const double p = pixel<MODE>(ra, rb, y * L.pitch + x);
      const double2 w = tw_w[k];
      re = fma(p, w.x, re);
      im = fma(p, w.y, im);
      k += v;
      if (k >= W) k -= W;
    }
    T[y * Wh + v] = make_double2(re, im);
  }
  __syncthreads();
#pragma unroll
  for (int j = 0; j < kMaxCells; ++j) {
    const int idx = threadIdx.x + j * kThreads;
    double re = 0.0, im = 0.0;
    if (idx < half) {
      const int u = idx / Wh, v = idx - u * Wh;
      int k = 0;
      for (int y = 0; y < H; ++y) {
        const double2 z = T[y * Wh + v];
        const double2 w = tw_h[k];
        re = fma(z.x, w.x, re);
        re = fma(-z.y, w.y, re);
        im = fma(z.x, w.y, im);
        im = fma(z.y, w.x, im);
        k += u;
        if (k >= H) k -= H;
      }
    }
    F[j] = make_double2(re, im);
  }
}

// A conj B of one cell, both products of each part rounded before they meet: (a, a) is |A|^2 with an imaginary part of
// exactly 0, (b, a) has the real part of (a, b) and its imaginary part negated
__device__ inline double2 cross(double2 a, double2 b) {
#pragma clang fp contract(off)
  const double rr = a.x * b.x, ii = a.y * b.y, ir = a.y * b.x, ri = a.x * b.y;
  return make_double2(rr + ii, ir - ri);
}

template <bool PAIR>
__global__ __launch_bounds__(kThreads) void spectral_kernel(RowSet a, RowSet b, int n_inner, int C, int H, int W, int n_bins,
                                                            const int *__restrict__ start, const int *__restrict__ order,
                                                            double *__restrict__ out, int *__restrict__ status) {
  constexpr int K = PAIR ? DT_SPECTRAL_PAIR_K : 1;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  const Lds L(H, W, PAIR);
  double2 *tw_w = reinterpret_cast<double2 *>(smem), *tw_h = reinterpret_cast<double2 *>(smem + L.tw_h);
  double2 *T = reinterpret_cast<double2 *>(smem + L.t);
  double *plane = reinterpret_cast<double *>(smem + L.t);   // H*W doubles <= H*Wh double2
  float *ra = reinterpret_cast<float *>(smem + L.ra), *rb = reinterpret_cast<float *>(smem + L.rb);

  const int t = threadIdx.x, row = blockIdx.x;
  const int ro = row / n_inner, ri = row - ro * n_inner;
  const float *ga = a.base + ro * a.ostride + ri * a.istride;
  const float *gb = PAIR ? b.base + ro * b.ostride + ri * b.istride : nullptr;
  const int cells = H * W, E = C * cells, Wh = L.Wh, half = H * Wh;
  double *orow = out + (size_t)row * C * n_bins * K;

  int bad = 0;
  for (int e = t; e < E; e += kThreads) {
    bad |= !isfinite(ga[e]);
    if constexpr (PAIR) bad |= !isfinite(gb[e]);
  }
  bad = __syncthreads_or(bad);
  if (t == 0) status[row] = bad ? DT_SPECTRAL_NONFINITE : DT_SPECTRAL_OK;
  if (bad) {   // uniform
    for (int e = t; e < C * n_bins * K; e += kThreads) orow[e] = __builtin_nan("");
    return;
  }
  for (int k = t; k < W + H; k += kThreads) {
    const bool along_x = k < W;
    const int n = along_x ? W : H, m = along_x ? k : k - W;
    double sn, cs;
    sincospi(2.0 * (double)m / (double)n, &sn, &cs);
    (along_x ? tw_w : tw_h)[m] = make_double2(cs, -sn);
  }

  const int wave = t / 64, lane = t % 64;
  for (int c = 0; c < C; ++c) {
    __syncthreads();   // the plane of the channel before has been read
    for (int e = t; e < cells; e += kThreads) {
      const int y = e / W, x = e - y * W;
      ra[y * L.pitch + x] = ga[c * cells + e];
      if constexpr (PAIR) rb[y * L.pitch + x] = gb[c * cells + e];
    }
    double2 FA[kMaxCells];
    [[maybe_unused]] double2 FB[kMaxCells], FD[kMaxCells];
    transform<0>(H, W, L, tw_w, tw_h, T, ra, rb, FA);
    if constexpr (PAIR) {
      transform<1>(H, W, L, tw_w, tw_h, T, ra, rb, FB);
      transform<2>(H, W, L, tw_w, tw_h, T, ra, rb, FD);
    }
#pragma unroll
    for (int q = 0; q < K; ++q) {
      __syncthreads();   // T, or the plane of the value before, has been read
#pragma unroll
      for (int j = 0; j < kMaxCells; ++j) {
        const int idx = t + j * kThreads;
        if (idx < half) {
          const int u = idx / Wh, v = idx - u * Wh;
          double val = cross(FA[j], FA[j]).x;
          if constexpr (PAIR) {
            if (q == DT_SPECTRAL_PB) val = cross(FB[j], FB[j]).x;
            else if (q == DT_SPECTRAL_CRE) val = cross(FA[j], FB[j]).x;
            else if (q == DT_SPECTRAL_CIM) val = cross(FA[j], FB[j]).y;
            else if (q == DT_SPECTRAL_D) val = cross(FD[j], FD[j]).x;
          }
          plane[u * W + v] = val;
          if (v > 0 && 2 * v != W)   // the conjugate cell: the same values, the imaginary part of the cross term negated
            plane[(u ? H - u : 0) * W + (W - v)] = q == DT_SPECTRAL_CIM ? -val : val;
        }
      }
      __syncthreads();
      for (int bn = wave; bn < n_bins; bn += kWaves) {   // uniform per wave
        const int s1 = start[bn + 1];
        double acc = 0.0;
        for (int p = start[bn] + lane; p < s1; p += 64) acc += plane[order[p]];
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d);
        if (lane == 0) orow[((size_t)c * n_bins + bn) * K + q] = acc;
      }
    }
  }
}

__global__ __launch_bounds__(kThreads) void spectral_sum_kernel(const double *__restrict__ out, const int *__restrict__ status,
                                                                size_t total, int n_inner, int per, double *__restrict__ sum,
                                                                int *__restrict__ count) {
  for (size_t idx = (size_t)blockIdx.x * kThreads + threadIdx.x; idx < total; idx += (size_t)gridDim.x * kThreads) {
    const size_t o = idx / per, e = idx - o * per;
    double acc = 0.0;
    int n = 0;
    for (int s = 0; s < n_inner; ++s) {
      const size_t row = o * n_inner + s;
      if (status[row] != DT_SPECTRAL_OK) continue;
      acc += out[row * per + e];
      ++n;
    }
    sum[idx] = acc;
    if (e == 0) count[o] = n;
  }
}

// ---------------------------------------------------------------------------------------------- host
bool picture_ok(int H, int W, int n_bins) {
  return H >= 1 && H <= kMaxHW && W >= 1 && W <= kMaxHW && n_bins >= 1 && n_bins <= DT_SPECTRAL_MAX_BINS;
}

bool rows_ok(int n_outer, int n_inner) {
  return n_outer >= 1 && n_inner >= 1 && (long long)n_outer * n_inner <= DT_SPECTRAL_MAX_ROWS;
}

size_t workspace_bytes(int H, int W) { return kStartBytes + ((size_t)H * W * sizeof(int) + 15) / 16 * 16; }

int check_rows(const float *p, long long ostride, long long istride) {
  if (ostride < 0 || istride < 0) return DT_E_SHAPE;
  return (uintptr_t)p & 3 ? DT_E_ARG : DT_OK;
}

// b == nullptr: one set
int run(const RowSet &a, const RowSet *b, int n_outer, int n_inner, int C, int H, int W, const int *bin, int n_bins, double *out,
        int *status, void *ws, size_t ws_bytes, hipStream_t s) {
  if (!a.base || (b && !b->base) || !bin || !out || !status || !ws) return DT_E_NULL;
  if (!picture_ok(H, W, n_bins) || !rows_ok(n_outer, n_inner) || C < 1 || C > DT_SPECTRAL_MAX_C) return DT_E_SHAPE;
  int rc;
  if ((rc = check_rows(a.base, a.ostride, a.istride)) != DT_OK) return rc;
  if (b && (rc = check_rows(b->base, b->ostride, b->istride)) != DT_OK) return rc;
  if (((uintptr_t)bin & 3) || ((uintptr_t)out & 7) || ((uintptr_t)status & 3) || ((uintptr_t)ws & 15)) return DT_E_ARG;
  if (ws_bytes < workspace_bytes(H, W)) return DT_E_WORKSPACE;

  static LdsLimitOnce lds_limit;
  static const size_t widest = Lds(kMaxHW, kMaxHW, true).bytes;
  static const LdsLimit limits[] = {{(const void *)spectral_kernel<false>, widest}, {(const void *)spectral_kernel<true>, widest}};
  if ((rc = lds_limit.raise(limits, 2)) != DT_OK) return rc;

  const int rows = n_outer * n_inner, K = b ? DT_SPECTRAL_PAIR_K : 1;
  int *start = (int *)ws, *order = (int *)((char *)ws + kStartBytes);
  ProfileScope prof(KC_SPECTRAL, 0.0, (double)rows * C * (4.0 * H * W * (b ? 2 : 1) + 8.0 * n_bins * K) + 4.0 * rows, s);
  spectral_order_kernel<<<1, kThreads, 0, s>>>(bin, H * W, n_bins, start, order);
  DT_LAUNCH_CHECK();
  if (b) spectral_kernel<true><<<rows, kThreads, Lds(H, W, true).bytes, s>>>(a, *b, n_inner, C, H, W, n_bins, start, order, out, status);
  else spectral_kernel<false><<<rows, kThreads, Lds(H, W, false).bytes, s>>>(a, a, n_inner, C, H, W, n_bins, start, order, out, status);
  DT_LAUNCH_CHECK();
  return DT_OK;
}

}  // namespace

static_assert(kThreads == DT_SPECTRAL_MAX_BINS, "spectral_order_kernel: one thread per bin");

extern "C" size_t dt_spectral_workspace_bytes(int H, int W, int n_bins) {
  return picture_ok(H, W, n_bins) ? workspace_bytes(H, W) : 0;
}

extern "C" int dt_spectral_power(const float *a_dev, long long a_ostride, long long a_istride, int n_outer, int n_inner, int C,
                                 int H, int W, const int *bin_dev, int n_bins, double *out_dev, int *status_dev, void *ws,
                                 size_t ws_bytes, void *stream) {
  const RowSet a{a_dev, a_ostride, a_istride};
  return run(a, nullptr, n_outer, n_inner, C, H, W, bin_dev, n_bins, out_dev, status_dev, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int dt_spectral_pair(const float *a_dev, long long a_ostride, long long a_istride, const float *b_dev,
                                long long b_ostride, long long b_istride, int n_outer, int n_inner, int C, int H, int W,
                                const int *bin_dev, int n_bins, double *out_dev, int *status_dev, void *ws, size_t ws_bytes,
                                void *stream) {
  const RowSet a{a_dev, a_ostride, a_istride}, b{b_dev, b_ostride, b_istride};
  return run(a, &b, n_outer, n_inner, C, H, W, bin_dev, n_bins, out_dev, status_dev, ws, ws_bytes, (hipStream_t)stream);
}

extern "C" int dt_spectral_sum(const double *out_dev, const int *status_dev, int n_outer, int n_inner, int C, int n_bins, int K,
                               double *sum_dev, int *count_dev, void *stream) {
  if (!out_dev || !status_dev || !sum_dev || !count_dev) return DT_E_NULL;
  if (!rows_ok(n_outer, n_inner) || C < 1 || C > DT_SPECTRAL_MAX_C || n_bins < 1 || n_bins > DT_SPECTRAL_MAX_BINS) return DT_E_SHAPE;
  if (K != 1 && K != DT_SPECTRAL_PAIR_K) return DT_E_ARG;
  if (((uintptr_t)out_dev & 7) || ((uintptr_t)sum_dev & 7) || ((uintptr_t)status_dev & 3) || ((uintptr_t)count_dev & 3)) return DT_E_ARG;
  hipStream_t s = (hipStream_t)stream;
  const int per = C * n_bins * K;
  const size_t total = (size_t)n_outer * per;
  ProfileScope prof(KC_SPECTRAL, 0.0, 8.0 * total * (n_inner + 1.0) + 4.0 * n_outer * (n_inner + 1.0), s);
  spectral_sum_kernel<<<grid_blocks(total, 1 << 16), kThreads, 0, s>>>(out_dev, status_dev, total, n_inner, per, sum_dev, count_dev);
  DT_LAUNCH_CHECK();
  return DT_OK;
}
