/*
 * mi355x_refiners_solver_step.h -- the guidance-free solver updates of libmi355x_refiners.so (refiners_amd/csrc/solver_step.hip).
 *
 * An extension of mi355x_refiners.h with the same conventions: plain C, raw device pointers, `stream` a hipStream_t passed as void*,
 * dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E* codes (EDTYPE -1, ESHAPE -2,
 * ELAUNCH -3, EARG -4).  A refused call launches nothing.  It is a header of its own because mi355x_refiners.h is a frozen list (ABI
 * version 7: its 39 prototypes and 24 structs are pinned); refiners_amd.native reads both headers the same way.
 *
 * They are mi355x_cfg_ddim_step / mi355x_cfg_linear_step for a model that runs WITHOUT classifier-free guidance
 * (latent_diffusion/model.py:128-159 with classifier_free_guidance = False: LCM, LCM-LoRA, SDXL-Lightning): `unet_out` has the n
 * elements of x, not [uncond ; cond], and eps = unet_out.  The update is the same device function the guided kernels call, so a call
 * here is bit-equal to the guided call on cat(unet_out, unet_out) at any guidance scale.  coef is the guided kernels' row of eight
 * float32 in DEVICE memory (a captured graph is replayed with new step coefficients); coef[0], the guidance scale, is not read.
 * Arithmetic is float32 whatever the storage type, there are no atomics and no workspace, every output element is written by exactly
 * one lane.  Any n > 0: 16-byte vectors, then n % (16 / sizeof dtype) single elements; operands that are not 16-byte aligned take the
 * single-element loop throughout.
 */
#ifndef MI355X_REFINERS_SOLVER_STEP_H
#define MI355X_REFINERS_SOLVER_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* mi355x_ddim_step -- DDIM.__call__ (solvers/ddim.py:56-95) on n elements, in place:
 *   x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t);  x' = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps;  model_in = x'
 * coef = {-, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev), -, -, -}.  model_in (n elements, may be NULL, must not overlap
 * x) receives the stored x': the next step's model input, so no copy of the latents precedes the next UNet pass.
 * EARG: x, unet_out or coef NULL, n <= 0. */
int mi355x_ddim_step(int32_t dtype, void* x, const void* unet_out, void* model_in, const float* coef, int64_t n, void* stream);

/* mi355x_linear_step -- one step of any solver that is linear in (x, eps, one kept quantity): Euler with noise prediction
 * (solvers/euler.py:99-100: kx = 1, ke = sigma' - sigma) or sample prediction (:94-97: kx = sigma' / sigma, ke = 1 - kx), DPM-Solver++
 * 2M (solvers/dpm.py:224-329), LCM (solvers/lcm.py:100-150; the step's noise draw is put into `hist` before the call):
 *   d = hx x + he eps;  x' = kx x + ke eps + kd d + kp hist;  hist = d;  model_in = s_next x'
 * coef = {-, hx, he, kx, ke, kd, kp, s_next}; x, hist, unet_out, model_in: n elements; model_in may be NULL (Solver.scale_model_input
 * of the NEXT step, applied to the stored x').  EARG: x, unet_out, hist or coef NULL, n <= 0. */
int mi355x_linear_step(int32_t dtype, void* x, const void* unet_out, void* hist, void* model_in, const float* coef, int64_t n, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_SOLVER_STEP_H */
