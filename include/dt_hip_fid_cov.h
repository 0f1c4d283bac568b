/*
 * dt_hip_fid_cov.h -- entry points of libdt_hip.so for the Fréchet distance of the FID stage by the feature-space route:
 * the same problem, arguments and outputs as include/dt_hip_fid.h, for sets with more rows than the feature width (FID as
 * it is normally reported: 10 000 to 50 000 samples per set, features of width 2048); added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32 unless stated, a stream argument, asynchronous,
 * int status (0 ok, <0 DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows.  As in dt_hip_fid.h: row i of set A of problem p at a + p*a_pstride + i*a_rstride (n_a rows of D floats), set B
 * likewise; strides in floats; a problem stride of 0 shares a set between all problems.
 * Limits: 1 <= P <= 65535, 2 <= n_a, n_b <= 131072, 4 <= D <= 2048, D % 4 == 0, row bases 16-byte aligned (pointers and
 * strides multiples of 4 floats).  Nothing ties n to D: n < D is legal, only slower than the sample-space route.
 *
 * Contract, all in fp64 on the float64 copy of the rows.  With the column means mu_A, mu_B, the centred rows A_c, B_c
 * and C_A = A_c^T A_c, C_B = B_c^T B_c (D x D, exactly symmetric; S_A = C_A / (n_a - 1)),
 *     fid = |mu_A - mu_B|^2 + tr S_A + tr S_B - 2 tr sqrt(S_A S_B),
 *     C_A = L_A L_A^T, C_B = L_B L_B^T, N = L_A^T L_B,
 *     tr sqrt(S_A S_B) = (sum of the singular values of N) / sqrt((n_a - 1)(n_b - 1)):
 * A_c = Q_A L_A^T and B_c = Q_B L_B^T with orthonormal Q, so N has the non-zero singular values of A_c B_c^T.  They are
 * the square roots of the eigenvalues of N N^T (side D), found as in dt_hip_fid.h: Householder tridiagonalisation,
 * Sturm-count bisection for all D of them, negative ones (rounding) clamped to 0, summed in index order.
 * The factor is the Cholesky factor without pivoting, lower-triangular, in 64-wide panels, with a zero-pivot rule for
 * covariances that are only positive semi-definite (constant columns, duplicated rows, n <= D):
 *     tol = D * 2^-52 * max_i C[i][i];  a pivot that is not > tol gives an all-zero column of L, and no division
 * (for a PSD matrix a zero Schur diagonal implies a zero Schur row, so the rule is exact in exact arithmetic).
 * The traces are the sums of squared deviations / (n - 1), not read off C.
 * Every sum has a fixed order that depends on (n_a, n_b, D) only (the means and squared deviations over chunks of 1024
 * rows, then the chunks in order; the covariance products over up to 8 slabs of rows, a number fixed by (n, D), then the
 * slabs in order), so a problem's outputs do not depend on P, on its neighbours, on strides or sharing, or on what the
 * workspace held.  fid == parts[0] + parts[1] + parts[2] - 2 parts[3] exactly.  The result is not clamped: two equal sets
 * give a value within rounding of 0 that may be negative.  A set without variance is no error: its trace and the cross
 * term are exactly 0.  A NaN or Inf in either set gives status 1 and NaN outputs for that problem only.
 * Where both routes apply they agree to rounding, not to the bit.
 */
#ifndef DT_HIP_FID_COV_H
#define DT_HIP_FID_COV_H

#include "dt_hip_fid.h" /* DT_FID_OK, DT_FID_NONFINITE: the same two status words */

#ifdef __cplusplus
extern "C" {
#endif

#define DT_FID_COV_MAX_ROWS 131072 /* largest n_a, n_b */
#define DT_FID_COV_MAX_WIDTH 2048  /* largest D */
#define DT_FID_COV_EVENTS 7

/* Bytes of workspace dt_fid_cov_distance needs (0 if the shape is outside the limits above; no overflow inside them).
 * Per problem: 3 matrices of D x D doubles (C_A and C_B, factored in place; N; N N^T takes C_A's place), for each set
 * whose rows are split into s > 1 slabs s more of them (s <= 8, and s = 1 from D = 1024 up: 96 MB per problem at D = 2048),
 * 2 (ceil(n_a / 1024) + ceil(n_b / 1024)) + 10 vectors of D doubles, 16 doubles; then P ints rounded up to 256 bytes. */
size_t dt_fid_cov_workspace_bytes(int P, int n_a, int n_b, int D);

/* Arguments, outputs and status words as dt_fid_distance: fid [P] fp64; parts [P][4] fp64 = (|mu_A - mu_B|^2, tr S_A,
 * tr S_B, tr sqrt(S_A S_B)); status [P] int (DT_FID_*).  ws: 16-byte aligned, ws_bytes >=
 * dt_fid_cov_workspace_bytes(...); its contents on entry do not matter.
 * events: NULL, or DT_FID_COV_EVENTS hipEvent_t recorded on `stream` at the start, after the means and traces, after the
 * covariance products, after the factorisations, after N and N N^T, after the tridiagonalisation and at the end
 * (bisection, sum, outputs). */
int dt_fid_cov_distance(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev,
                        int n_b, long long b_pstride, long long b_rstride, int P, int D, double *fid_dev,
                        double *parts_dev, int *status_dev, void *ws, size_t ws_bytes, void *const *events, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_FID_COV_H */
