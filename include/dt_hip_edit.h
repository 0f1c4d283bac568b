/*
 * dt_hip_edit.h -- entry points of libdt_hip.so for the editing stage (editing/masked_inpainting.py,
 * editing/latent_manipulation.py, editing/prompt_editing.py), added under DT_ABI_VERSION 6.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32 unless stated, a stream
 * argument, asynchronous, int status (0 ok, <0 DT_E_*, >0 a hipError_t).
 *
 * The known-region blend (masked_inpainting.py:181, :218) is, per element,
 *     out = m * x' + (1 - m) * k
 * in un-contracted fp32 in the reference's order (two products, 1 - m, one sum): bit-identical to
 * torch CPU for any mask, and equal to k where m == 0 and to x' where m == 1.  Image b of a batch
 * reads row mask_row[b] of mask[.][E] and row known_row[b] of known[.][E]; a null row table is the
 * identity (row b), so one mask or one known image can serve many batch rows without being
 * replicated.  Row tables are int32 device arrays of B entries; the rows they name must exist.
 */
#ifndef DT_HIP_EDIT_H
#define DT_HIP_EDIT_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Known rows and start states of B editing cells from n_img images in [0, 1] (masked_inpainting.py:178, :181):
 *   known_out[i][e] = 2 * img[i][e] - 1                                 i < n_img (one product, one subtraction)
 *   x_out[b][e]     = m * z[z_row[b]][e] + (1 - m) * known_out[img_row[b]][e],   m = mask[mask_row[b]][e]
 * img_dev [n_img][E], known_out [n_img][E], x_out [B][E]; img_row / z_row / mask_row: null = row b (img_row null needs
 * n_img >= B).  E % 4 == 0, every tensor 16-byte aligned.  x_out may be slot 0 of a trajectory. */
int dt_edit_start(const float *img_dev, const int32_t *img_row, int n_img, const float *z_dev, const int32_t *z_row,
                  const float *mask_dev, const int32_t *mask_row, float *known_out, float *x_out, int B, int E,
                  void *stream);

/* dt_cfg_update followed by the blend: out = m * rule(x, eps, z) + (1 - m) * k.  The first fourteen arguments are
 * dt_cfg_update's.  The ENGINE step without noise (t == 0) copies x unblended, as the reference's loop does.
 * mask_dev / known_dev 16-byte aligned. */
int dt_cfg_update_masked(int rule, const float *x_dev, const float *eps_u_dev, const float *eps_c_dev, const float *z_dev,
                         const int32_t *z_row, const float coef[4], int has_noise, const float *w_dev, float w_scalar,
                         float *out_dev, int B, int E, void *stream, const float *mask_dev, const int32_t *mask_row,
                         const float *known_dev, const int32_t *known_row);

/* The sampler loop of dt_sample_trajectory / dt_sample_trajectory_mixed with the blend after every update, on the fused and
 * on the layered path.  n_pass 1: B_single must be 0.  n_pass 2: images [0, B_single) take one pass and the others two
 * (B_single == 0: a plain CFG batch; 0 < B_single < B: dt_sample_trajectory_mixed's conditions on tb_div hold and w_dev is
 * required).  Row r of a step's forward uses time-bias row r / tb_div.  All three rules.  Never replayed from a captured graph. */
int dt_sample_trajectory_masked(const dt_unet *h, int rule, int B, int n_pass, int B_single, int H, int W, int n_steps,
                                const float *tb_dev, int tb_div, const float *coef_host, const int32_t *has_noise_host,
                                const float *z_dev, const int32_t *z_row, const int64_t *z_shift_host, const float *w_dev,
                                float w_scalar, const float *mask_dev, const int32_t *mask_row, const float *known_dev,
                                const int32_t *known_row, float *traj_dev, void *ws_dev, size_t ws_bytes, void *stream);

/* Hole statistics of two trajectories x, y [n][B][E] against the known image, in fp64:
 *   out[b][i] = { sum m (x - y)^2, sum m (x - k)^2, sum m (y - k)^2, sum (1 - m) (x - y)^2 }        out_dev [B][n][4] doubles
 * with m, k the mask and known rows of image b.  Differences, products and sums are formed in fp64 from the fp32 inputs;
 * the summation order is fixed (no atomics): repeated calls give the same bits.  E % 4 == 0, n <= 65535, B <= 65535;
 * x / y / mask / known 16-byte aligned. */
int dt_masked_pair_stats(const float *x_dev, const float *y_dev, int n, int B, int E, const float *mask_dev,
                         const int32_t *mask_row, const float *known_dev, const int32_t *known_row, double *out_dev,
                         void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_EDIT_H */
