/*
 * dt_hip_noise.h -- entry points of libdt_hip.so for the noise-prediction analysis
 * (analysis/noise_prediction/noise_analysis.py), added with DT_ABI_VERSION 5.
 * Same rules as include/dt_hip.h: borrowed device pointers, fp32 unless stated, a stream
 * argument, asynchronous, int status (0 ok, <0 DT_E_*, >0 a hipError_t).
 */
#ifndef DT_HIP_NOISE_H
#define DT_HIP_NOISE_H

#include "dt_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Forward noising of n_groups timesteps at once (analysis/noise_prediction/noise_analysis.py:268):
 *   out[g][b][e] = a_g * x0[b][e] + s_g * z[g][b][e],   coef_dev[g] = {a_g, s_g} = {sqrt(ab_t), sqrt(1 - ab_t)} fp32
 * (:253-262).  x0_dev [B][E], z_dev / out_dev [n_groups][B][E]; E % 4 == 0, x0 / z / out 16-byte aligned, coef 8-byte
 * aligned.  Un-contracted fp32 in the reference's order (two products, then the sum): bit-identical to torch CPU. */
int dt_q_sample(const float *x0_dev, const float *z_dev, const float *coef_dev, int n_groups, int B, int E,
                float *out_dev, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DT_HIP_NOISE_H */
