/*
 * dt_hip_sinkhorn.h -- entry points of libdt_hip.so for the entropic optimal-transport cost between two sets of states
 * with uniform weights, by Sinkhorn iterations on the dual potentials in the log domain.  The debiased Sinkhorn divergence
 * S_eps(A,B) = OT_eps(A,B) - 1/2 OT_eps(A,A) - 1/2 OT_eps(B,B) (Feydy et al. 2019) is three calls of dt_sinkhorn_ot and one
 * expression of the caller's.  Added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, a stream argument, asynchronous, int status (0 ok, <0
 * DT_E_*, >0 a hipError_t); no allocation: scratch comes from the caller (workspace); every argument error is returned
 * before any launch.
 *
 * Rows, as in include/dt_hip_swd.h.  A problem is one state.  Its set A has n_a rows of E fp32; row i of problem q is at
 * a + q*a_ps + i*a_rs (strides in floats, >= 0), set B likewise.  Rows are read in place, element by element, and need the
 * alignment of a float only.  a_ps == 0 is one set shared by every problem.  Both sets carry uniform weights 1/n_a, 1/n_b.
 * Limits: 1 <= n_a, n_b <= DT_SINKHORN_MAX_N (they may differ), 1 <= E <= DT_SINKHORN_MAX_E, 1 <= P <= DT_SINKHORN_MAX_P,
 * 1 <= max_iter <= DT_SINKHORN_MAX_ITER: outside them DT_E_SHAPE.  p in {1, 2}, tol >= 0 and finite: otherwise DT_E_ARG.
 * eps [P] fp64 is read from device memory, one value per problem.
 *
 * Arithmetic: fp64 throughout, every sum in one fixed order that depends on (n_a, n_b, E) alone, no atomics on values.
 * exp, log and expm1 are the device's; nothing transcendental comes from the host.  Apart from the fused multiply-adds named
 * below, every operation is rounded on its own (fp contract is off in the whole translation unit).
 *   Cost        c_ij = sum_e d*d, d = double(a_ie) - double(b_je) (exact): one chain acc = fma(d, d, acc) from +0.0, e
 *               ascending.  The walk is padded to a multiple of 16 with zeros, which changes no bit.  C_ij = c_ij (p = 2)
 *               or sqrt(c_ij) (p = 1).  C_ij is never negative and exactly 0 for two equal rows.
 *   Mean cost   r_i = sum_j C_ij: lane l of a wave of 64 adds the j = l, l + 64, .. ascending from 0.0, the 64 lane sums
 *               meet in the butterfly s += s(lane ^ m), m = 32, 16, .. 1.  The r_i, padded with 0.0 to the next power of
 *               two N of n_a, are added in the tree part[i] += part[i + h], h = N/2, .. 1, and
 *               mean_cost = sum / double(n_a*n_b).
 *   Start       g = 0.  r = 1.0 / eps, one rounded reciprocal; every "/ eps" below is a multiplication by r.
 *   Step k = 1, 2, ..
 *     half 1    z_j = (g_j - C_ij) * r; m = max_j z_j; s = sum_j exp(z_j - m) in the order of r_i above (lanes along j,
 *               then the butterfly);  f_i = -eps * ((m + log(s)) - log(double(n_b))).
 *     half 2    z_i = (f_i - C_ij) * r; m = max_i z_i; wave w of the kColWaves = 16 of a workgroup adds exp(z_i - m) for
 *               i = w, w + 16, .. ascending from 0.0, the 16 partial sums are added w ascending from the first;
 *               g'_j = -eps * ((m + log(s)) - log(double(n_a))).
 *     error     e_j = |expm1((g_j - g'_j) * r)|; the e_j, padded with 0.0 to the next power of two of n_b, are added in the
 *               tree above, and err_k = sum / double(n_b): the L1 distance between the column marginal of the plan before
 *               the g-update and b.  Then g = g'.
 *     freezing  with tol > 0 and err_k <= tol the problem is frozen: iters = k, and the later launches return at once for
 *               it (a flag in the workspace; the host never waits).  With tol == 0 exactly max_iter steps run.
 *   Value       ot = (sum_i f_i) / double(n_a) + (sum_j g_j) / double(n_b), both sums in the tree above (padded to the
 *               next power of two of their own length).  After a g-update the plan's mass is 1, so this is the full dual
 *               objective.
 *
 * status [P] int32, bits: DT_SINKHORN_NONFINITE (a NaN or Inf in the rows of either set: ot, err, f, g and mean_cost are
 * NaN, iters 0), DT_SINKHORN_BAD_EPS (eps not finite or <= 0: the same), DT_SINKHORN_NOT_CONVERGED (tol > 0 and err at
 * step max_iter is above tol: the values are still those of max_iter steps).  Other problems are unaffected.
 *
 * Contracts (tests/test_hip_sinkhorn.py), bit for bit:
 *   1. a problem's outputs depend on its rows, eps, p, max_iter and tol only: not on the batch, its position in it, the
 *      strides, the alignment, the size of the workspace or how the call was cut into chunks;
 *   2. with tol > 0 a frozen problem's outputs are those of a run with tol = 0 and max_iter = iters;
 *   3. dt_sinkhorn_ot(A, B') with B' a bitwise copy of A gives the bits of dt_sinkhorn_ot(A, A), and so do (B', B') and
 *      (B', A): all three terms of a divergence take this one path, so it is exactly 0.0 for a copy;
 *   4. multiplying both sets by 2^k and eps by 2^(k*p) multiplies ot, f, g and mean_cost by 2^(k*p) exactly and keeps the
 *      bits of err and iters (no overflow, no underflow);
 *   5. f and g as written out are the values the sums of ot read.
 */
#ifndef DT_HIP_SINKHORN_H
#define DT_HIP_SINKHORN_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define DT_SINKHORN_MAX_N 2048
#define DT_SINKHORN_MAX_E (1 << 20)
#define DT_SINKHORN_MAX_P (1 << 16)
#define DT_SINKHORN_MAX_ITER 10000

/* per-problem status bits */
#define DT_SINKHORN_OK 0
#define DT_SINKHORN_NONFINITE 1
#define DT_SINKHORN_BAD_EPS 2
#define DT_SINKHORN_NOT_CONVERGED 4

/* Bytes of workspace with which both entries take P problems in one chunk (0 outside the limits).  The value for P = 1
 * is the least they accept; with anything from there on they take as many problems at a time as fit, with the same bits. */
size_t dt_sinkhorn_workspace_bytes(int P, int n_a, int n_b);

/* mean_cost_dev [P] fp64: the mean over all (i, j) of C_ij; status_dev [P] int32 (DT_SINKHORN_NONFINITE or 0). */
int dt_sinkhorn_mean_cost(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev, long long b_ps,
                          long long b_rs, int n_b, int E, int P, int p, double *mean_cost_dev, int *status_dev, void *ws,
                          size_t ws_bytes, void *stream);

/* ot_dev, err_dev [P] fp64 (err: the marginal error of the last step run); iters_dev, status_dev [P] int32; f_dev [P][n_a]
 * and g_dev [P][n_b] fp64 may each be NULL. */
int dt_sinkhorn_ot(const float *a_dev, long long a_ps, long long a_rs, int n_a, const float *b_dev, long long b_ps,
                   long long b_rs, int n_b, int E, int P, int p, const double *eps_dev, int max_iter, double tol,
                   double *ot_dev, double *err_dev, int *iters_dev, int *status_dev, double *f_dev, double *g_dev, void *ws,
                   size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_SINKHORN_H */
