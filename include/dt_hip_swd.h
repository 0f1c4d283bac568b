/*
 * dt_hip_swd.h -- entry points of libdt_hip.so for the sliced Wasserstein distance between two sets of states: both sets
 * are projected onto L caller-supplied directions, every projection is sorted, and the exact 1-D Wasserstein distance W_p^p
 * between the two empirical distributions is taken per direction, with its mean and its maximum over the directions.
 * Added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace); every argument error is returned
 * before any launch.
 *
 * Rows.  A problem is one state.  Its set A has n_a rows of E fp32; row i of problem q is at a + q*a_ps + i*a_rs (strides
 * in floats, >= 0), set B likewise.  Rows are read in place, element by element, and need the alignment of a float only, so
 * a view of a step-major trajectory [n, S, E] (every k-th state, a slice or a stride of the samples) needs no copy.
 * a_ps == 0 is one set shared by every problem.
 * Directions.  theta [L][E] fp32, row l at theta + l*theta_rs, shared by all problems.  The library knows no sampling
 * rule and does not normalise.
 * Limits: 1 <= n_a, n_b <= DT_SWD_MAX_N (they may differ), 1 <= E <= DT_SWD_MAX_E (any value), 1 <= L <= DT_SWD_MAX_L,
 * 1 <= P <= DT_SWD_MAX_P, p in {1, 2}.  Outside them: DT_E_SHAPE (p: DT_E_ARG).
 *
 * Arithmetic: fp64 throughout, every sum in one fixed order, no atomics on values.
 *   Projection  proj[q][l][i] = sum_e double(theta[l][e]) * double(x[i][e]): one chain of fused multiply-adds per cell,
 *               starting from +0.0, e = 0 .. E-1 ascending (every product is exact in fp64).  The walk is padded to a
 *               multiple of 16 with zeros, which changes no bit.
 *   Sort        the n projections of a (problem, direction) ascending (a bitonic network over the next power of two, padded
 *               with +Inf).  Only the values matter: the result is the sorted multiset.
 *   Distance    between the two empirical quantile functions.  "big" is the larger set (A on a tie), sizes nB >= nS.
 *               Element i of big overlaps elements j = floor(i*nS/nB) .. ceil((i+1)*nS/nB) - 1 of small with the integer
 *               weight w_ij = min((i+1)*nS, (j+1)*nB) - max(i*nS, j*nB).  For every i, starting from 0.0 and over j
 *               ascending: acc = fma(double(w_ij), c, acc) with c = |big_i - small_j| (p = 1) or the rounded square of
 *               that difference (p = 2).  The nB partial sums, padded with 0.0 to the next power of two N, are added in
 *               the tree part[i] += part[i + h], h = N/2, N/4, .. 1: its shape depends on nB alone.  That total is T_l, and
 *               w[q][l] = T_l / double(nB*nS).
 *   Mean        the T_l, padded with 0.0 to the next power of two of L, are added in the same tree (fixed by L alone), and
 *               mean_w[q] = sum / (double(nB*nS) * double(L)): the mean of w over the directions with one rounding of the
 *               quotient, not the sum of the rounded w.
 *   Maximum     max_w[q] = max_l w[q][l], argmax[q] the first l that reaches it.
 * The p-th root is left to the caller.
 *
 * status [P] int32: DT_SWD_OK, or DT_SWD_NONFINITE when any element of the problem's rows (of either set) or any element of
 * theta is NaN or Inf.  Every fp64 output of that problem is then NaN (its part of a sorted buffer too) and argmax is -1.
 * Other problems are unaffected (a non-finite theta flags all of them).
 *
 * Contracts (tests/test_hip_swd.py), bit for bit:
 *   1. a problem's outputs depend on its rows, theta and p only: not on the batch, the strides, the alignment, its position
 *      in the batch, the size of the workspace or how the call was cut into chunks;
 *   2. permuting the rows of a set changes no bit;
 *   3. swapping A and B changes no bit of w, mean_w, max_w or argmax;
 *   4. if B is a bitwise copy of A, or a row permutation of it, every output is exactly 0.0 and argmax is 0;
 *   5. multiplying both sets by 2^k multiplies w, mean_w and max_w by 2^(k*p) exactly (no overflow, no underflow);
 *   6. dt_swd_sorted on both sets followed by dt_swd_distance gives the bits of dt_swd; a shared sorted buffer (problem
 *      stride 0) gives the bits of P copies of it;
 *   7. for integer-valued rows and axis-unit directions every intermediate value is exact (while it stays below 2^53) and
 *      w, mean_w and max_w are the correctly rounded quotients of the exact rational results.
 */
#ifndef DT_HIP_SWD_H
#define DT_HIP_SWD_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_SWD_MAX_N 2048
#define DT_SWD_MAX_E (1 << 20)
#define DT_SWD_MAX_L 4096
#define DT_SWD_MAX_P (1 << 16)

/* per-problem status words */
#define DT_SWD_OK 0
#define DT_SWD_NONFINITE 1

/* workspace of dt_swd_sorted: a few flags, whatever the shape */
#define DT_SWD_SORTED_WORKSPACE_BYTES 256

/* Bytes of a sorted buffer [P][L][n] fp64 (0 outside the limits). */
size_t dt_swd_sorted_bytes(int P, int n, int L);

/* Bytes of workspace with which dt_swd takes P problems in one chunk (0 outside the limits).  The value for P = 1 is the
 * least that dt_swd accepts; with anything from there on it takes as many problems at a time as fit. */
size_t dt_swd_workspace_bytes(int P, int n_a, int n_b, int L);

/* The same for dt_swd_distance, which keeps the per-direction totals there: P = 1 gives the least it accepts. */
size_t dt_swd_distance_workspace_bytes(int P, int L);

/* Projects one set and sorts every column: sorted_dev [P][L][n] fp64, status_dev [P] int32.  The projections are written
 * to sorted_dev and sorted in place; ws_bytes >= DT_SWD_SORTED_WORKSPACE_BYTES. */
int dt_swd_sorted(const float *x_dev, long long x_ps, long long x_rs, int n, int E, const float *theta_dev, long long theta_rs,
                  int L, int P, double *sorted_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* The distances of two sorted buffers made with the same theta.  Problem q reads sa_dev + q*sa_ps ([L][n_a] fp64) and
 * status_a_dev[q]; sa_ps == 0 is one shared set, whose status is status_a_dev[0]; otherwise sa_ps >= L*n_a.  B likewise.
 * w_dev [P][L] fp64 may be NULL; mean_w_dev, max_w_dev [P] fp64; argmax_dev, status_dev [P] int32 (status_dev must not be an
 * input status array). */
int dt_swd_distance(const double *sa_dev, long long sa_ps, const int *status_a_dev, int n_a, const double *sb_dev,
                    long long sb_ps, const int *status_b_dev, int n_b, int L, int P, int p, double *w_dev, double *mean_w_dev,
                    double *max_w_dev, int *argmax_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* Both steps in one call, in chunks of as many problems as the workspace holds.  Outputs as in dt_swd_distance. */
int dt_swd(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev, long long b_ps, long long b_rs,
           int n_b, int E, const float *theta_dev, long long theta_rs, int L, int P, int p, double *w_dev, double *mean_w_dev,
           double *max_w_dev, int *argmax_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_SWD_H */
