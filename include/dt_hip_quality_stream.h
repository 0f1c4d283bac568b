/*
 * dt_hip_quality_stream.h -- the row-panel route of the sample-quality scores of include/dt_hip_quality.h (KID, improved
 * precision / recall, density / coverage) for sets of up to 131072 rows each; entries added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip_quality.h: borrowed device pointers, fp32 rows, a stream argument, asynchronous, int status
 * (0 ok, <0 DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows.  As in dt_hip_quality.h: row i of set A of problem p at a + p*a_pstride + i*a_rstride, row j of set B at
 * b + p*b_pstride + j*b_rstride, strides in floats, A the "real" set (the teacher), B the "generated" one (a student).
 * Limits: 1 <= P <= 65535, 2 <= n_a, n_b <= 131072, 4 <= D <= 2^20, D % 4 == 0, 1 <= k <= min(n_a, n_b) - 1 and
 * k <= 1023, panel_rows a multiple of 64 in 64 .. 4096, row bases 16-byte aligned (pointers and strides multiples of 4
 * floats).  Sets shorter than 2049 rows are legal.
 *
 * Definitions.  Those of dt_hip_quality.h, all in fp64 on the float64 copy of the rows: d2(x, y) = max(0, G(x,x) + G(y,y)
 * - 2 G(x,y)); r2 the (k+1)-th smallest entry of a row of d2(A, A) / d2(B, B), self included, duplicates counted; the four
 * integer counts with strict <; the unbiased full-set KID with kappa(x, y) = (G(x,y) / D + 1)^3, the diagonal left out by
 * index; status words DT_QUALITY_OK / DT_QUALITY_NONFINITE, and for a non-finite problem NaN doubles and counts of -1.
 * This entry takes no subset tables.
 *
 * Method.  No matrix with n rows on both sides is ever held.  Per problem the workspace holds one panel of panel_rows
 * rows of a Gram matrix (panel_rows x max(n_a, n_b) doubles) and the vectors (diagonals, squared radii, kappa row sums,
 * integer hit words).  Panels of A x A, of B x B and of A x B are formed in turn, each consumed by the selection,
 * kernel-sum and counting launches before the next overwrites it.
 *
 * Gram entries.  G(x, y) = sum_k x_k y_k on the fp64 matrix instruction: every entry of every panel, and every G(x, x)
 * of the diagonals, runs through the same instruction sequence on the products x_k y_k (k ascending, four per
 * instruction), and the product commutes, so the same two rows give the same bits wherever they meet.  The self-distance
 * is exactly 0, and so is the distance of two rows with equal bits.  The summation order differs from the FMA chain of
 * dt_quality_scores: where both routes apply they agree to rounding (radii, KID) and, where every comparison that is not
 * an exact tie is decided by a margin above the rounding of both, exactly in the counts -- not to the bit.
 *
 * Determinism.  Every floating-point sum has a fixed order (Gram entries as above; kappa row sums: lanes over the columns
 * in ascending order, then one butterfly; then one fixed tree over the row sums), the radii are exact order statistics and
 * the counts are integers.  A problem's outputs do not depend on P, on the other problems of the call, on the strides, on
 * whether A is shared (a_pstride == 0) or copied P times, on the workspace contents on entry, or on panel_rows.
 *
 * Shared teacher.  With a_pstride == 0 and P > 1 the A side (its diagonals, radii and A x A kernel sums) is formed once
 * and read by every problem; a non-finite value in a shared A makes every problem DT_QUALITY_NONFINITE.  A non-finite
 * problem leaves its neighbours' bits alone.
 */
#ifndef DT_HIP_QUALITY_STREAM_H
#define DT_HIP_QUALITY_STREAM_H

#include "dt_hip_quality.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_QUALITY_STREAM_MAX_ROWS 131072 /* largest n_a, n_b */
#define DT_QUALITY_STREAM_MAX_K 1023      /* largest k: k + 1 keys stay in the selection's LDS buffer */
#define DT_QUALITY_STREAM_EVENTS 6

/* Bytes of workspace dt_quality_stream_scores needs (0 if the shape is outside the limits above): per problem
 * panel_rows * max(n_a, n_b) + 6 (n_a + n_b) doubles or fewer besides, never n^2. */
size_t dt_quality_stream_workspace_bytes(int P, int n_a, int n_b, int D, int panel_rows);

/* Per problem: kid [P] fp64; counts [P][4] int64 = (precision_hits, recall_hits, density_pairs, coverage_hits); radii:
 * NULL, or [P][n_a + n_b] fp64, the squared radii, A's then B's; status [P] int (DT_QUALITY_*).  ws: 16-byte aligned,
 * ws_bytes >= dt_quality_stream_workspace_bytes(...); its contents on entry do not matter.  events: NULL, or
 * DT_QUALITY_STREAM_EVENTS hipEvent_t recorded on `stream` at the start, after the diagonals and the non-finite flag,
 * after the A side (radii and A x A kernel sums), after the B side, after the A x B panels (counts and kernel sums) and
 * at the end (the fixed trees, KID and the outputs). */
int dt_quality_stream_scores(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev,
                             int n_b, long long b_pstride, long long b_rstride, int P, int D, int k, int panel_rows,
                             double *kid_dev, long long *counts_dev, double *radii_dev, int *status_dev, void *ws,
                             size_t ws_bytes, void *const *events, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_QUALITY_STREAM_H */
