/*
 * dt_hip_tsne.h -- entry points of libdt_hip.so for the t-SNE of the dimensionality analysis (analysis/dimensionality/):
 * exact t-SNE (sklearn.manifold.TSNE(method="exact"), 2 components) of a batch of P independent problems, added under
 * DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace).
 *
 * Rows are addressed as in include/dt_hip_pca.h: problem p has n = n_a + n_b rows of E floats, row i < n_a at
 * a + p*a_pstride + i*a_rstride, row n_a + j at b + p*b_pstride + j*b_rstride (strides in floats; b may be NULL with
 * n_b = 0), so a pair of step-major trajectories is used in place.
 * Limits: 1 <= P <= 65535, 4 <= n <= 512, E >= 4, E % 4 == 0, row bases 16-byte aligned (pointers and strides multiples
 * of 4 floats), 0 < perplexity < n.
 *
 * Every sum runs in an order that depends only on n: a problem's bits do not depend on P, on its neighbours, or on how a
 * range of iterations is cut into calls.
 */
#ifndef DT_HIP_TSNE_H
#define DT_HIP_TSNE_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_TSNE_MAX_N 512

/* per-problem status words written by dt_tsne_affinities */
#define DT_TSNE_OK 0
#define DT_TSNE_NONFINITE 1 /* a NaN or Inf in the rows: the problem's affinities (and then its embedding and KL) are NaN */

/* stop reasons (ctl[3] of a problem's state) */
#define DT_TSNE_RUNNING 0
#define DT_TSNE_NO_PROGRESS 1 /* no better error for more than n_iter_without_progress iterations */
#define DT_TSNE_GRAD_NORM 2   /* norm of the gain-scaled gradient <= min_grad_norm */

/* Doubles of state per problem: y, update, gains, each [n][2], then ctl = {best_error, best_iter, iterations done,
 * stop reason}.  A fresh state is y = Y0, update = 0, gains = 1, ctl = {DBL_MAX, 0, 0, 0}. */
#define DT_TSNE_STATE_DOUBLES(n) (6 * (size_t)(n) + 4)

/* sklearn's schedule; its defaults in brackets */
typedef struct dt_tsne_params {
  double early_exaggeration;  /* [12] alpha while it < exaggeration_iters, 1 afterwards */
  double learning_rate;       /* ["auto": max(n / early_exaggeration / 4, 50)] */
  double momentum[2];         /* [0.5, 0.8] in the exaggerated stage and after it */
  double min_gain;            /* [0.01] */
  double min_grad_norm;       /* [1e-7] */
  int exaggeration_iters;     /* [250] */
  int n_iter_check;           /* [50] the stop rules run when (it + 1) % n_iter_check == 0 */
  int n_iter_without_progress[2]; /* [250, 300] in the exaggerated stage and after it */
} dt_tsne_params;

/* Bytes of workspace dt_tsne_affinities needs (0 if the shape is outside the limits above). */
size_t dt_tsne_workspace_bytes(int P, int n, int E);

/* Joint probabilities p_dev [P][n][n] fp64 of sklearn's exact method: squared distances from the centred fp64 Gram
 * matrix (D_ij = G_ii + G_jj - 2 G_ij, clamped at 0), per row the binary search for the precision (at most 100 steps,
 * |H - log perplexity| <= 1e-5, a zero row sum replaced by 1e-8), P = (C + C^T) / sum floored at DBL_EPSILON, diagonal 0.
 * status [P] int (DT_TSNE_*). */
int dt_tsne_affinities(const float *a_dev, int n_a, long long a_pstride, long long a_rstride, const float *b_dev,
                       int n_b, long long b_pstride, long long b_rstride, int P, int E, double perplexity,
                       double *p_dev, int *status_dev, void *ws, size_t ws_bytes, void *stream);

/* Iterations [it_begin, it_end) of sklearn's exact gradient descent on KL(P || Q), all in fp64, one workgroup per
 * problem and one launch for the range.  state_dev [P][DT_TSNE_STATE_DOUBLES(n)] is read and written; params is a host
 * pointer, read before the call returns.  At it == exaggeration_iters, update is zeroed, gains are set to 1 and
 * best_error / best_iter restart (sklearn's second _gradient_descent call).  A problem whose stop reason is not 0 does no
 * work; a stop in the exaggerated stage is final too (sklearn would go on to its second stage).
 * On return embedding_dev [P][n][2] is y rounded to fp32 and kl_dev [P] the plain KL of the current y. */
int dt_tsne_descend(const double *p_dev, int P, int n, double *state_dev, int it_begin, int it_end,
                    const dt_tsne_params *params, float *embedding_dev, double *kl_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_TSNE_H */
