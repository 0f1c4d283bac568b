/*
 * dt_hip_align.h -- entry points of libdt_hip.so for trajectory alignment: the matrix of Euclidean distances between every
 * state of one trajectory and every state of another, and dynamic time warping (DTW) and the discrete Frechet distance over
 * it, for a batch of P independent problems, added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace); every argument error is returned
 * before any launch.
 *
 * Rows are addressed as in include/dt_hip_tsne.h: problem p has n_a rows a + p*a_pstride + i*a_rstride and n_b rows
 * b + p*b_pstride + j*b_rstride of E floats (strides in floats), so step-major trajectories [n, S, E] and contiguous
 * [P, n, E] are both used in place.  Nothing has to be aligned beyond the element type and E need not be a multiple of 4.
 * Limits: 1 <= P <= 65535, 2 <= n_a, n_b <= DT_ALIGN_MAX_N, 1 <= E <= 2^28, 0 <= band <= 2^20.
 *
 * Cost matrix: cost[p][i][j] = sqrt(sum_e (double(a_e) - double(b_e))^2), the sum taken with one fused multiply-add per
 * element in the order e = 0, 1, ..., E-1 for EVERY cell.  A cell's bits depend on its two rows and E only -- not on its
 * place in the matrix, on P, on the strides or on which operand is called a: cost(b, a) is the bitwise transpose of
 * cost(a, b), cells of bit-identical rows are exactly 0.0, and a problem's bits do not depend on the batch.
 *
 * Dynamic programme, on any [n_a][n_b] fp64 matrix D:
 *   DTW      C[0][0] = D[0][0], C[i][j] = m + D[i][j]      (one fp64 addition)
 *   Frechet  C[0][0] = D[0][0], C[i][j] = max(D[i][j], m)
 * where m is the smallest of C[i-1][j-1], C[i-1][j], C[i][j-1] among those that exist, ties taken in that order.  The value
 * is C[n_a-1][n_b-1]; the path runs from (0, 0) to (n_a-1, n_b-1) along the chosen predecessors.  band > 0 is a Sakoe-Chiba
 * band in integers: cell (i, j) is allowed iff |i*(n_b-1) - j*(n_a-1)| <= band * max(n_a-1, n_b-1); a cell outside it has
 * C = +Inf and is never chosen over a finite one.  band == 0: no band.  There is no reduction whose order could vary: value
 * and path are a function of the bits of D.
 *
 * Per-problem status: a NaN or an Inf anywhere in a problem's rows, or in its matrix (band or not), gives
 * DT_ALIGN_NONFINITE, value NaN and path_len 0; an infinite end value gives DT_ALIGN_NO_PATH, value +Inf and path_len 0.
 * (Every band >= 1 contains the staircase i = round(j*(n_a-1)/(n_b-1)) or its mirror image, so NO_PATH is a guard, not a
 * state a finite matrix reaches.)  Other problems of the batch are not affected.
 */
#ifndef DT_HIP_ALIGN_H
#define DT_HIP_ALIGN_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_ALIGN_MAX_N 1024
#define DT_ALIGN_MAX_BAND (1 << 20)

/* kinds, and their bits in a kind_mask */
#define DT_ALIGN_DTW 0
#define DT_ALIGN_FRECHET 1
#define DT_ALIGN_MASK_DTW 1
#define DT_ALIGN_MASK_FRECHET 2

/* per-problem status words */
#define DT_ALIGN_OK 0
#define DT_ALIGN_NONFINITE 1
#define DT_ALIGN_NO_PATH 2

/* Longest path: n_a + n_b - 1 cells. */
#define DT_ALIGN_PATH_CELLS(n_a, n_b) ((n_a) + (n_b)-1)

/* Bytes of workspace that hold all P problems at once (0 if the shape is outside the limits).  want_path: a path is asked
 * for (one predecessor byte per cell); cost_given: the caller provides the cost matrices (dt_align_dp always; dt_align with
 * cost_out_dev), otherwise they live in the workspace.  Never 0 inside the limits. */
size_t dt_align_workspace_bytes(int P, int n_a, int n_b, int want_path, int cost_given);

/* The same for one problem: the least dt_align accepts. */
size_t dt_align_min_workspace_bytes(int n_a, int n_b, int want_path, int cost_given);

/* cost_dev [P][n_a][n_b] fp64; status_dev [P] int: DT_ALIGN_OK or DT_ALIGN_NONFINITE (a NaN or Inf in a row of a or b). */
int dt_align_cost(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
                  long long b_pstride, long long b_rstride, int P, int E, double *cost_dev, int *status_dev, void *stream);

/* One workgroup per problem over cost_dev [P][n_a][n_b] (from dt_align_cost or made by the caller), kind DT_ALIGN_DTW or
 * DT_ALIGN_FRECHET.  value_dev [P] fp64.  path_dev [P][n_a+n_b-1][2] int32 with path_len_dev [P] int, or both NULL:
 * path[p][k] = (i, j) for k < path_len[p], in order from (0, 0), and (-1, -1) after it.  status_dev [P] int (DT_ALIGN_*).
 * The workspace holds all P problems (dt_align_workspace_bytes(P, n_a, n_b, path_dev != NULL, 1)). */
int dt_align_dp(const double *cost_dev, int P, int n_a, int n_b, int kind, int band, double *value_dev, int *path_dev,
                int *path_len_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* dt_align_cost once, then dt_align_dp for every kind of kind_mask (DT_ALIGN_MASK_*): dtw_dev / frechet_dev [P] fp64
 * (required for a kind asked for, ignored otherwise), the paths as in dt_align_dp, each pair NULL or set; cost_out_dev
 * [P][n_a][n_b] fp64 or NULL.  Problems go through in chunks of as many as the workspace holds: any workspace of at least
 * dt_align_min_workspace_bytes(n_a, n_b, a path is asked for, cost_out_dev != NULL) is accepted and the outputs do not
 * depend on its size. */
int dt_align(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
             long long b_pstride, long long b_rstride, int P, int E, int kind_mask, int band, double *cost_out_dev,
             double *dtw_dev, double *frechet_dev, int *dtw_path_dev, int *dtw_path_len_dev, int *frechet_path_dev,
             int *frechet_path_len_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_ALIGN_H */
