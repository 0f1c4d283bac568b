/*
 * dt_hip_cka.h -- entry points of libdt_hip.so for layer-wise centered kernel alignment (linear CKA, Kornblith et al. 2019,
 * and the debiased estimator of Song et al. 2012 as used by Nguyen, Raghu and Kornblith 2021) between two sets of layers
 * that saw the same n inputs, added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace); every argument error is returned
 * before any launch.
 *
 * Feature sets.  A layer is n rows of fp32; row i starts at base + i*row_stride (floats).  A row is `groups` runs of `c`
 * valid floats at a pitch of `pitch` floats: element (g, ch) sits at row + g*pitch + ch, and is feature k = g*c + ch of
 * p = groups*c.  A dense [n, p] matrix is groups = 1, c = pitch = p; a U-Net block output [n, h, w, cp] in the forward's
 * workspace is groups = h*w, c the real channel count, pitch = cp.  Floats at ch >= c are never read.  L layers are passed
 * as HOST arrays of length L: base pointer, row stride, groups, c and pitch.  Bases need 4-byte alignment only.
 * Limits: 4 <= n <= DT_CKA_MAX_N, 1 <= L <= DT_CKA_MAX_LAYERS, 1 <= groups*c <= DT_CKA_MAX_P, 1 <= c <= pitch,
 * row_stride >= 0.
 *
 * Gram.  For each layer: the fp64 mean of every feature, m_k = (sum of double(x_ik) in the order i = 0 .. n-1) / n; then
 * the FEATURE-CENTRED Gram K'[i][j] = sum_k (x_ik - m_k)(x_jk - m_k).  The feature axis is cut into slabs of DT_CKA_SLAB
 * features; inside a slab a cell is one fp64 fused multiply-add chain over k ascending, starting from 0.0, and a cell is
 * 0.0 plus the slabs' values added in index order.  K' is stored symmetric bit for bit.
 * sums[l] (DT_CKA_SUMS doubles) holds what the scores need of the layer alone, every sum in a fixed order:
 *   [DT_CKA_SUM_ALL]    sum of K'[i][j]^2 over all cells         [DT_CKA_SUM_OFF]   the same over i != j
 *   [DT_CKA_SUM_TOTAL]  1' K~ 1, K~ = K' with a zero diagonal    [DT_CKA_SUM_TRACE] tr K'
 *   [DT_CKA_SUM_HSIC1]  HSIC1(K, K) below                        [DT_CKA_SUM_ROWS + i], i < n: row i's sum of K~ (0 for i >= n)
 *
 * Scores of layer a (Gram K) against layer b (Gram L):
 *   cka          = <K', L'> / sqrt(<K', K'> <L', L'>),  <K, L> = sum over all cells of K_ij L_ij
 *   HSIC1(K, L)  = [ <K~, L~> + (1'K~1)(1'L~1) / ((n-1)(n-2)) - 2/(n-2) (K~1)'(L~1) ] / (n(n-3))
 *   cka_unbiased = HSIC1(K, L) / sqrt(HSIC1(K, K) HSIC1(L, L))
 * Features are centred before the Gram is formed: neither estimator changes (HKH = K', and HSIC1 is invariant to a shift
 * of the features), and the cancellation inside HSIC1 is then mild.  The self terms <K', K'> and HSIC1(K, K) in sums are
 * made by the same routine as a cross term, with L = K.
 *
 * Per-layer status bits: DT_CKA_NONFINITE a NaN or Inf among the layer's valid floats (its Gram and sums are NaN);
 * DT_CKA_ZERO_VARIANCE <K', K'> == 0; otherwise DT_CKA_SELF_NOT_POSITIVE where HSIC1(K, K) <= 0 (the debiased self term
 * is a U-statistic: for a feature-centred Gram it vanishes, for instance, on one-hot layers, K' = I - 11'/n, and rounding can
 * take such a value to or below zero).  A layer has at most one bit.  cka is NaN where either layer has NONFINITE or ZERO_VARIANCE, cka_unbiased where
 * either has any bit.  Other layers are untouched.
 *
 * Contracts (tests/test_hip_cka.py):
 *   - a layer's Gram and sums bits depend on that layer's rows, groups and c alone: not on L, on the other layers, on row
 *     stride, pitch or alignment, on the pad contents, or on the workspace size;
 *   - scores(a, b)[i][j] has the bits of scores(b, a)[j][i];
 *   - scaling a layer by a power of two (no overflow, no underflow) leaves every score bit-identical;
 *   - a layer against a bit-identical copy gives exactly 1.0 in both estimators (status 0).
 */
#ifndef DT_HIP_CKA_H
#define DT_HIP_CKA_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_CKA_MIN_N 4
#define DT_CKA_MAX_N 2048
#define DT_CKA_MAX_LAYERS 64
#define DT_CKA_MAX_P (1 << 24)
/* features per slab of the Gram's sum: part of the definition of a cell's bits */
#define DT_CKA_SLAB 1024

#define DT_CKA_SUM_ALL 0
#define DT_CKA_SUM_OFF 1
#define DT_CKA_SUM_TOTAL 2
#define DT_CKA_SUM_TRACE 3
#define DT_CKA_SUM_HSIC1 4
#define DT_CKA_SUM_ROWS 8
#define DT_CKA_SUMS (DT_CKA_SUM_ROWS + DT_CKA_MAX_N)

#define DT_CKA_NONFINITE 1
#define DT_CKA_ZERO_VARIANCE 2
#define DT_CKA_SELF_NOT_POSITIVE 4

/* Bytes of workspace with which dt_cka_gram / dt_cka run layers of up to p_max features at full width (every slab of a
 * layer in flight, up to what fills the device); 0 outside the limits.  It does not grow with L: layers take turns. */
size_t dt_cka_workspace_bytes(int L, int n, int p_max);

/* The least they accept: the means and one slab.  Slabs then go through in turns; the outputs do not depend on the size. */
size_t dt_cka_min_workspace_bytes(int n, int p_max);

/* gram_dev [L][n][n] fp64, sums_dev [L][DT_CKA_SUMS] fp64, status_dev [L] int. */
int dt_cka_gram(const float *const *base_dev, const long long *row_stride, const int *groups, const int *c, const int *pitch,
                int L, int n, double *gram_dev, double *sums_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* One workgroup per pair: cka_dev and cka_unbiased_dev [La][Lb] fp64; hsic_dev [La][Lb][2] fp64 (<K', L'> and HSIC1(K, L))
 * or NULL.  The Grams, sums and status words are those of dt_cka_gram for the same n. */
int dt_cka_scores(const double *gram_a_dev, const double *sums_a_dev, const int *status_a_dev, int La,
                  const double *gram_b_dev, const double *sums_b_dev, const int *status_b_dev, int Lb, int n, double *cka_dev,
                  double *cka_unbiased_dev, double *hsic_dev, void *stream);

/* dt_cka_gram of both sides, then dt_cka_scores.  base_b == NULL scores set a against itself: Lb and the other b arguments
 * are then ignored and the outputs are [La][La].  The Gram outputs are the caller's, as in dt_cka_gram. */
int dt_cka(const float *const *base_a_dev, const long long *row_stride_a, const int *groups_a, const int *c_a,
           const int *pitch_a, int La, double *gram_a_dev, double *sums_a_dev, int *status_a_dev,
           const float *const *base_b_dev, const long long *row_stride_b, const int *groups_b, const int *c_b,
           const int *pitch_b, int Lb, double *gram_b_dev, double *sums_b_dev, int *status_b_dev, int n, double *cka_dev,
           double *cka_unbiased_dev, double *hsic_dev, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_CKA_H */
