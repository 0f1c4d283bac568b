/*
 * dt_hip_quality.h -- entry points of libdt_hip.so for the set-level sample-quality numbers beside FID
 * (analysis/metrics/sample_quality.py): KID, improved precision / recall (Kynkäänniemi et al. 2019) and density / coverage
 * (Naeem et al. 2020) of two feature sets that are already on the device, for a batch of P independent problems; added
 * under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip_fid.h: borrowed device pointers, fp32 rows, a stream argument, asynchronous, int status
 * (0 ok, <0 DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows.  Problem p has two sets of rows of D floats: row i of set A at a + p*a_pstride + i*a_rstride (n_a rows), row j
 * of set B at b + p*b_pstride + j*b_rstride (n_b rows); strides in floats.  A problem stride of 0 shares a set between
 * all problems (one teacher against P students).  A is the "real" set (the teacher), B the "generated" set (a student).
 * Limits: 1 <= P <= 65535, 2 <= n_a, n_b <= 2048, 4 <= D <= 2^20, D % 4 == 0, 1 <= k <= min(n_a, n_b) - 1, row bases
 * 16-byte aligned (pointers and strides multiples of 4 floats).
 *
 * Contract, all in fp64 on the float64 copy of the rows.
 *
 * Gram matrices.  G(x, y) = sum_k x_k y_k is one FMA chain over k ascending, so the same two rows give the same bits
 * whichever of the three matrices (A x A, B x B, A x B) they appear in.  d2(x, y) = max(0, G(x,x) + G(y,y) - 2 G(x,y));
 * the self-distance is exactly 0, and so is the distance of two rows with equal bits.
 *
 * Radii.  r2_A[i] is the (k+1)-th smallest entry of row i of d2(A, A), self included (the k-th nearest-neighbour
 * distance as the `prdc` package defines it); r2_B[j] likewise in d2(B, B).  The value counts: duplicates count as often
 * as they occur.
 *
 * Counts, integers, every comparison a strict <, as in `prdc`:
 *     precision_hits = #{ j : exists i, d2(a_i, b_j) < r2_A[i] }
 *     recall_hits    = #{ i : exists j, d2(a_i, b_j) < r2_B[j] }
 *     density_pairs  = #{ (i, j) : d2(a_i, b_j) < r2_A[i] }
 *     coverage_hits  = #{ i : min_j d2(a_i, b_j) < r2_A[i] }
 * so precision = precision_hits / n_b, recall = recall_hits / n_a, density = density_pairs / (k n_b),
 * coverage = coverage_hits / n_a.
 *
 * KID.  With kappa(x, y) = (G(x,y) / D + 1)^3, the full-set unbiased estimator
 *     kid = sum_{i != j} kappa(a_i, a_j) / (n_a (n_a - 1)) + sum_{i != j} kappa(b_i, b_j) / (n_b (n_b - 1))
 *           - 2 sum_{i, j} kappa(a_i, b_j) / (n_a n_b),
 * the diagonal left out by index.  Every sum has a fixed order (row sums, then one fixed tree), so a problem's bits do not
 * depend on P, on its neighbours, on the strides or on the workspace contents.  Optionally S subsets of size m
 * (1 <= S <= 1024, 2 <= m <= min(n_a, n_b)) are given as two int32 device tables [S][m], one of row numbers of A and
 * one of B, shared by all problems; each row of a table holds distinct indices in range (the caller checks that: the
 * kernel clamps an index into range so that it reads nothing outside the matrices, and no more).  The same estimator on
 * the gathered sub-blocks of the Gram matrices gives one KID per subset.  The tables are made on the host.
 *
 * Each problem keeps its own three matrices in the workspace.
 */
#ifndef DT_HIP_QUALITY_H
#define DT_HIP_QUALITY_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* per-problem status words written by dt_quality_scores */
#define DT_QUALITY_OK 0
#define DT_QUALITY_NONFINITE 1 /* a NaN or Inf in either set: the doubles of the problem are NaN, its counts -1 */

#define DT_QUALITY_MAX_ROWS 2048    /* largest n_a, n_b */
#define DT_QUALITY_MAX_SUBSETS 1024 /* largest S */
#define DT_QUALITY_EVENTS 5

/* Bytes of workspace dt_quality_scores needs (0 if the shape is outside the limits above). */
size_t dt_quality_workspace_bytes(int P, int n_a, int n_b, int D);

/* Per problem: kid [P][1 + S] fp64, the full-set value first, then one per subset; counts [P][4] int64 =
 * (precision_hits, recall_hits, density_pairs, coverage_hits); radii: NULL, or [P][n_a + n_b] fp64, the squared radii,
 * A's then B's; status [P] int (DT_QUALITY_*).  sub_a / sub_b: the subset tables, both NULL when S == 0 (m is then
 * ignored).  ws: 16-byte aligned, ws_bytes >= dt_quality_workspace_bytes(...); its contents on entry do not matter.
 * events: NULL, or DT_QUALITY_EVENTS hipEvent_t recorded on `stream` at the start, after the three Gram matrices, after
 * the radii, after the counts and at the end (the kernel sums, KID and the outputs). */
int dt_quality_scores(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
                      long long b_pstride, long long b_rstride, int P, int D, int k, const int *sub_a_dev,
                      const int *sub_b_dev, int S, int m, double *kid_dev, long long *counts_dev, double *radii_dev,
                      int *status_dev, void *ws, size_t ws_bytes, void *const *events, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_QUALITY_H */
