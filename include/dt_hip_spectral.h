/*
 * dt_hip_spectral.h -- entry points of libdt_hip.so for spatial-frequency spectra of trajectory states: the per-band power
 * spectrum of one set of pictures and, for a teacher set against a student set, the per-band cross-spectrum and the spectrum
 * of their difference, added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace); every argument error is returned
 * before any launch.
 *
 * Rows.  A row is one state of one sample: C channel pictures of H x W fp32, contiguous inside the row (NCHW, C*H*W floats).
 * Row (i, s), 0 <= i < n_outer, 0 <= s < n_inner, starts at a + i*a_ostride + s*a_istride (strides in floats, >= 0), so a
 * slice of a step-major trajectory [n, S, E] with every k-th state, and a flat [Q, E] tensor (n_outer = 1), are read in
 * place.  Nothing has to be aligned beyond the element type.  Row (i, s) is row number r = i*n_inner + s of the outputs.
 * Limits: 1 <= H, W <= DT_SPECTRAL_MAX_HW (any value, not only powers of two), 1 <= C <= DT_SPECTRAL_MAX_C,
 * 1 <= n_bins <= DT_SPECTRAL_MAX_BINS, 1 <= n_outer * n_inner <= DT_SPECTRAL_MAX_ROWS.
 *
 * Transform.  Per channel the unnormalised forward DFT
 *   F[u][v] = sum_y sum_x x[y][x] exp(-2 pi i (u y / H + v x / W)),
 * in fp64 from the fp32 input, as a direct separable DFT: along x, then along y.  A twiddle factor is
 * (cospi(2k/N), -sinpi(2k/N)) with k = (v x) mod W or (u y) mod H, so no angle above 2 pi is formed.  Every coefficient is
 * one chain of fused multiply-adds in the order x = 0 .. W-1, then y = 0 .. H-1 (real part: T_re c - T_im s, imaginary
 * part: T_re s + T_im c, the first product of each first).  Only the columns v <= W/2 are transformed; a coefficient with
 * v > W/2 is the conjugate of the one at ((H-u) mod H, W-v), which is exact for a real picture in exact arithmetic and is
 * the definition here.
 *
 * Bins.  bin_dev [H][W] int32: the bin of coefficient (u, v) in [0, n_bins), or -1 for a coefficient that is left out (any
 * value outside [0, n_bins) is read as -1).  The library knows no binning rule.
 *
 * Outputs, all fp64 and all sums over the cells of a bin.  For rows a (teacher) and b (student) with A = DFT(a),
 * B = DFT(b) and Delta = DFT(double(a) - double(b)), transformed in its own right:
 *   out[r][c][bin][DT_SPECTRAL_PA]  sum |A|^2               out[r][c][bin][DT_SPECTRAL_PB]  sum |B|^2
 *   out[r][c][bin][DT_SPECTRAL_CRE] sum Re(A conj B)        out[r][c][bin][DT_SPECTRAL_CIM] sum Im(A conj B)
 *   out[r][c][bin][DT_SPECTRAL_D]   sum |Delta|^2
 * (DT_SPECTRAL_PAIR_K = 5 values per bin); dt_spectral_power gives out[r][c][bin][1] with sum |A|^2 alone.
 * Per cell, with both products rounded before they meet: Re = A_re B_re + A_im B_im, Im = A_im B_re - A_re B_im; |A|^2 is
 * that Re with B = A.  A bin's cells are taken in the order of their index u*W + v: the cell at position p of the bin goes
 * to partial sum p mod 64, every partial sum adds its cells in order starting from 0.0, and the 64 partial sums meet in a
 * fixed butterfly (distances 32, 16, .. 1).  No atomics: the order depends on (H, W, table) alone.  An empty bin is 0.0.
 *
 * status_dev [rows] int32: DT_SPECTRAL_OK, or DT_SPECTRAL_NONFINITE for a NaN or Inf anywhere in the row (in either row of
 * a pair): every output of that row is then NaN.  Other rows are unaffected.
 *
 * Workspace: the cells of the table sorted by bin, made anew by every call; dt_spectral_workspace_bytes says how much, a
 * larger one changes nothing.
 *
 * Contracts (tests/test_hip_spectral.py), bit for bit:
 *   1. a row's outputs depend on its own floats, on C, H, W and on the bin table only: not on the batch, the strides, the
 *      row's position, n_outer / n_inner, or the workspace;
 *   2. dt_spectral_power gives the bits of dt_spectral_pair's [DT_SPECTRAL_PA];
 *   3. swapping a and b swaps the bits of PA and PB, keeps the bits of CRE and D, and negates CIM (a zero stays +0.0);
 *   4. if b is a bitwise copy of a: D == 0.0 exactly, PB and CRE have the bits of PA, CIM == 0.0;
 *   5. multiplying both inputs by 2^k (no overflow, no underflow) multiplies every output by 4^k exactly.
 */
#ifndef DT_HIP_SPECTRAL_H
#define DT_HIP_SPECTRAL_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_SPECTRAL_MAX_HW 64
#define DT_SPECTRAL_MAX_C 64
#define DT_SPECTRAL_MAX_BINS 256
#define DT_SPECTRAL_MAX_ROWS (1 << 24)

/* values per bin of dt_spectral_pair, and their places */
#define DT_SPECTRAL_PAIR_K 5
#define DT_SPECTRAL_PA 0
#define DT_SPECTRAL_PB 1
#define DT_SPECTRAL_CRE 2
#define DT_SPECTRAL_CIM 3
#define DT_SPECTRAL_D 4

/* per-row status words */
#define DT_SPECTRAL_OK 0
#define DT_SPECTRAL_NONFINITE 1

/* Bytes of workspace of dt_spectral_power / dt_spectral_pair (0 if the shape is outside the limits): it does not grow with
 * the number of rows.  Never 0 inside the limits. */
size_t dt_spectral_workspace_bytes(int H, int W, int n_bins);

/* out_dev [n_outer*n_inner][C][n_bins][1] fp64, status_dev [n_outer*n_inner] int. */
int dt_spectral_power(const float *a_dev, long long a_ostride, long long a_istride, int n_outer, int n_inner, int C, int H,
                      int W, const int *bin_dev, int n_bins, double *out_dev, int *status_dev, void *ws, size_t ws_bytes,
                      void *stream);

/* out_dev [n_outer*n_inner][C][n_bins][DT_SPECTRAL_PAIR_K] fp64, status_dev [n_outer*n_inner] int. */
int dt_spectral_pair(const float *a_dev, long long a_ostride, long long a_istride, const float *b_dev, long long b_ostride,
                     long long b_istride, int n_outer, int n_inner, int C, int H, int W, const int *bin_dev, int n_bins,
                     double *out_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* Sums out_dev [n_outer][n_inner][C][n_bins][K] (K = 1 or DT_SPECTRAL_PAIR_K) over the inner axis: every element starts
 * from 0.0 and adds the rows s = 0 .. n_inner-1 in order, skipping rows whose status is not DT_SPECTRAL_OK.
 * sum_dev [n_outer][C][n_bins][K] fp64; count_dev [n_outer] int, the rows that were added. */
int dt_spectral_sum(const double *out_dev, const int *status_dev, int n_outer, int n_inner, int C, int n_bins, int K,
                    double *sum_dev, int *count_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_SPECTRAL_H */
