/*
 * dt_hip_fid.h -- entry points of libdt_hip.so for the Fréchet distance of the FID stage (analysis/metrics/fid_score.py,
 * evaluation/metrics.py): two feature sets that are already on the device in, one double out, for a batch of P
 * independent problems; added under DT_ABI_VERSION 5.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32 unless stated, a stream argument, asynchronous,
 * int status (0 ok, <0 DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows.  Problem p has two sets of rows of D floats: row i of set A at a + p*a_pstride + i*a_rstride (n_a rows), row j
 * of set B at b + p*b_pstride + j*b_rstride (n_b rows); strides in floats.  A problem stride of 0 shares a set between
 * all problems (one teacher against P students).
 * Limits: 1 <= P <= 65535, 2 <= n_a, n_b <= 32768, min(n_a, n_b) <= 2048, 4 <= D <= 2^20, D % 4 == 0, row bases
 * 16-byte aligned (pointers and strides multiples of 4 floats).
 *
 * Contract, all in fp64 on the float64 copy of the rows.  With the column means mu_A, mu_B, the centred rows A_c, B_c
 * and the sample covariances S_A = A_c^T A_c / (n_a - 1), S_B likewise,
 *     fid = |mu_A - mu_B|^2 + tr S_A + tr S_B - 2 tr sqrt(S_A S_B),
 *     tr sqrt(S_A S_B) = (sum of the singular values of M = A_c B_c^T) / sqrt((n_a - 1)(n_b - 1)),
 * and the singular values of M are the square roots of the eigenvalues of M M^T or M^T M (the smaller one, side
 * m = min(n_a, n_b)): a Householder tridiagonalisation and Sturm-count bisection for all m of them, negative ones
 * (rounding) clamped to 0.  No D x D matrix is formed.  Every sum has a fixed order: a problem's outputs do not depend on
 * P, on its neighbours or on the strides.  The result is not clamped: two equal sets give a value within rounding of 0
 * that may be negative.  A set without variance is no error: its trace and the cross term are 0.
 * Sets of more than 2048 rows each go through include/dt_hip_fid_cov.h (the same outputs by the feature-space formula).
 */
#ifndef DT_HIP_FID_H
#define DT_HIP_FID_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-problem status words written by dt_fid_distance */
#define DT_FID_OK 0
#define DT_FID_NONFINITE 1 /* a NaN or Inf in either set: fid and the four parts of the problem are NaN */

#define DT_FID_MAX_SIDE 2048 /* largest min(n_a, n_b) */
#define DT_FID_EVENTS 5

/* Bytes of workspace dt_fid_distance needs (0 if the shape is outside the limits above). */
size_t dt_fid_workspace_bytes(int P, int n_a, int n_b, int D);

/* Per problem: fid [P] fp64; parts [P][4] fp64 = (|mu_A - mu_B|^2, tr S_A, tr S_B, tr sqrt(S_A S_B)); status [P] int
 * (DT_FID_*).  ws: 16-byte aligned, ws_bytes >= dt_fid_workspace_bytes(...); its contents on entry do not matter.
 * events: NULL, or DT_FID_EVENTS hipEvent_t recorded on `stream` at the start, after the means and traces, after the two
 * products (M, then M M^T or M^T M), after the tridiagonalisation and at the end (bisection, sum, outputs). */
int dt_fid_distance(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
                    long long b_pstride, long long b_rstride, int P, int D, double *fid_dev, double *parts_dev,
                    int *status_dev, void *ws, size_t ws_bytes, void *const *events, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_FID_H */
