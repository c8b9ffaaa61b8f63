/*
 * mi355x_refiners_sde_step.h -- the stochastic solver updates of libmi355x_refiners.so (refiners_amd/csrc/solver_step.hip).
 *
 * An extension of mi355x_refiners.h with the conventions of mi355x_refiners_solver_step.h: plain C, raw device pointers, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of mi355x_refiners.h's negative
 * MI355X_E* codes (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing.  It is a header of its own because
 * mi355x_refiners.h is a frozen list; refiners_amd.native reads every header the same way.
 *
 * They are mi355x_cfg_linear_step / mi355x_linear_step with a FIFTH operand, the step's Gaussian draw, for the SDE form of DPM-Solver++
 * 2M (solvers/dpm.py:241-246, 284-290 with SolverParams(sde_variance=1.0)):
 *   eps = u + cfg (c - u)                                  guided form only; the other reads eps = unet_out
 *   d   = hx x + he eps
 *   x'  = kx x + ke eps + kd d + kp hist + kn noise
 *   hist = d;  model_in = s_next x'
 * coef = {cfg, hx, he, kx, ke, kd, kp, s_next, kn}: NINE float32 in DEVICE memory (a captured graph is replayed with new step
 * coefficients), the first eight the row of mi355x_cfg_linear_step.  The update is that kernel's device function followed by exactly
 * one fused multiply-add, so with kn = 0 the results compare equal to mi355x_cfg_linear_step / mi355x_linear_step on the same operands,
 * and the guidance-free form is bit-equal to the guided one on cat(unet_out, unet_out) at any guidance scale.
 * x, hist, noise: n elements; noise is read only.  Arithmetic is float32 whatever the storage type, there are no atomics and no workspace,
 * every output element is written by exactly one lane.  Any n > 0: 16-byte vectors, then n % (16 / sizeof dtype) single elements;
 * operands that are not 16-byte aligned take the single-element loop throughout (in the guided form the second halves of unet_out and
 * model_in count as operands: they are aligned when n is a whole number of vectors).
 */
#ifndef MI355X_REFINERS_SDE_STEP_H
#define MI355X_REFINERS_SDE_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_cfg_sde_step -- classifier-free guidance + the update above: unet_out = [uncond ; cond], 2n elements; model_in: 2n elements (both
 * halves receive s_next x', the next step's model input) or NULL; it must not overlap the other operands.
 * EARG: x, unet_out, hist, noise or coef NULL, n <= 0. */
int mi355x_cfg_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef, int64_t n, void* stream);

/* mi355x_sde_step -- the same for a model that runs without classifier-free guidance: unet_out and model_in (may be NULL) have n elements;
 * coef[0] is not read.  EARG: x, unet_out, hist, noise or coef NULL, n <= 0. */
int mi355x_sde_step(int32_t dtype, void* x, const void* unet_out, void* hist, const void* noise, void* model_in, const float* coef, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_SDE_STEP_H */
