/*
 * dt_hip_pca.h -- entry points of libdt_hip.so for the dimensionality analysis (analysis/dimensionality/): an exact,
 * deterministic PCA of a batch of P independent problems, added under DT_ABI_VERSION 5.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32 unless stated, a stream argument, asynchronous,
 * int status (0 ok, <0 DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows.  Problem p has n = n_a + n_b rows of E floats: row i < n_a at a + p*a_pstride + i*a_rstride, row n_a + j at
 * b + p*b_pstride + j*b_rstride (strides in floats; b may be NULL with n_b = 0).  A pair of step-major trajectories
 * X [nX][S][E], Y [nY][S][E] is used in place with row stride S*E and problem stride E.
 * Limits: 1 <= P <= 65535, n >= 2, 1 <= k <= min(16, n - 1, E), E % 4 == 0, row bases 16-byte aligned (pointers and
 * strides multiples of 4 floats).
 *
 * Contract: the result of sklearn.decomposition.PCA(n_components=k, svd_solver="full") on the float64 copy of the rows:
 * the column mean, the top k eigenpairs (lambda, u) of the centred Gram matrix G = Xc Xc^T (fp64), singular values
 * sqrt(lambda), explained variance lambda / (n - 1), ratio lambda / trace(G), components Xc^T u / sqrt(lambda) and scores
 * sqrt(lambda) * u, each component negated so that its entry of largest magnitude (first index on ties) is positive.
 * Every output element is summed in a fixed order: a problem's result does not depend on P or on its neighbours.
 *
 * Repeated eigenvalues.  Where lambda repeats (or nearly does), the contract is the subspace and not the basis: the
 * components of the group are an orthonormal basis of the same span as sklearn's, each with the sign rule applied, and
 * scores = Xc . components^T holds for them; which basis is returned is fixed (the result is still bit-stable), but it is
 * not sklearn's.
 *
 * Null directions.  The eigen stage resolves lambda no finer than n * DBL_EPSILON * ||T||, T the tridiagonal form of G (the
 * amount it widens its own Gershgorin interval by).  A top-k lambda_j at or below that (a rank below k) is reported as
 * null: its singular value, explained variance and ratio are exactly 0, its component and its score column are exactly
 * 0, and the status stays DT_PCA_OK.  sklearn returns an arbitrary unit vector there; this library returns zeros, as it
 * does for a whole problem under DT_PCA_ZERO_VARIANCE, so that the sign of a rounding error never decides an output.
 */
#ifndef DT_HIP_PCA_H
#define DT_HIP_PCA_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_PCA_MAX_K 16

/* per-problem status words written by dt_pca_fit */
#define DT_PCA_OK 0
#define DT_PCA_NONFINITE 1     /* a NaN or Inf in the rows: every output of the problem is NaN */
#define DT_PCA_ZERO_VARIANCE 2 /* trace(G) == 0: singular values, variances, scores, components 0; ratio NaN */

/* Bytes of workspace dt_pca_fit needs (0 if the shape is outside the limits above). */
size_t dt_pca_workspace_bytes(int P, int n, int E, int k);

/* Per problem: mean [P][E], components [P][k][E], scores [P][n][k] (rows in input order, a rows first) fp32;
 * singular, variance, ratio [P][k] fp64; status [P] int (DT_PCA_*).
 * events: NULL, or 4 hipEvent_t recorded on `stream` at the start, after the mean and Gram stage, after the eigen stage
 * (tridiagonalisation, bisection, inverse iteration, back-transformation) and at the end (components, signs, scores). */
int dt_pca_fit(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
               long long b_pstride, long long b_rstride, int P, int E, int k, float *mean_dev, float *components_dev,
               float *scores_dev, double *singular_dev, double *variance_dev, double *ratio_dev, int *status_dev,
               void *ws, size_t ws_bytes, void *const *events, void *stream);

/* scores [P][n][k] = (row - mean) . components^T with fp64 accumulation, for rows addressed as above.  mean [E] and
 * components [k][E] of problem p at mean_dev + p*mean_pstride and components_dev + p*comp_pstride (floats); a stride of
 * 0 gives every problem the same basis.  Both 16-byte aligned, strides multiples of 4.  Limits: n >= 1, 1 <= k <= 16. */
int dt_pca_project(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev, int n_b,
                   long long b_pstride, long long b_rstride, int P, int E, int k, const float *mean_dev,
                   long long mean_pstride, const float *components_dev, long long comp_pstride, float *scores_dev,
                   void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_PCA_H */
