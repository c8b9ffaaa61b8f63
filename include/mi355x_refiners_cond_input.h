/*
 * mi355x_refiners_cond_input.h -- step-constant UNet input channels of libmi355x_refiners.so (refiners_amd/csrc/cond_input.hip).
 *
 * An extension of mi355x_refiners.h with the conventions of mi355x_refiners_solver_step.h: plain C, raw device pointers, `stream` a
 * hipStream_t passed as void*, dtype = MI355X_F32 (0) or MI355X_BF16 (1), return value 0 or one of that header's negative MI355X_E* codes
 * (EDTYPE -1, ESHAPE -2, ELAUNCH -3, EARG -4).  A refused call launches nothing.  Arithmetic is float32 whatever the storage type, there are
 * no atomics and no workspace, every output element is written by exactly one lane.
 *
 * A UNet whose input has more channels than the latents (SD1.5 inpainting: cat(x, mask_latents, target_image_latents), 9 channels; IC-Light:
 * cat(x, condition), 8) reads `model_in` [n or 2n][C + E][hw] where the latents x are [n][C][hw]: the E extra channels are constant over a
 * trajectory up to the solver's input scale (latent_diffusion/model.py:137-159 scales the whole concatenation).  All tensors are
 * NCHW-contiguous; hw = h * w.  cond is [nc][E][hw] with nc = 1 (one condition for the whole batch) or nc = n.
 *
 * ESHAPE (every entry point): a tensor of more than 2^40 elements.
 *
 * Vector path: 16-byte vectors when hw * sizeof(dtype) is a multiple of 16 and every pointer given is 16-byte aligned; otherwise single
 * elements throughout (a channel row of 35 elements is legal).
 */
#ifndef MI355X_REFINERS_COND_INPUT_H
#define MI355X_REFINERS_COND_INPUT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* `form` of mi355x_cond_step */
#define MI355X_COND_DDIM 0
#define MI355X_COND_LINEAR 1

/* mi355x_cond_step -- the step's last launch when E > 0: the latent update of mi355x_cfg_ddim_step / mi355x_cfg_linear_step (guided = 1:
 * unet_out is [2n][C][hw] = [uncond ; cond], eps = u + coef[0] (c - u)) or mi355x_ddim_step / mi355x_linear_step (guided = 0: unet_out is
 * [n][C][hw]), through the same device functions, so x and hist come out bit-equal to those kernels on the same operands; then the next
 * step's model input:
 *   model_in[img][0:C]     = s_next x'                       (both halves, img and n + img, when guided)
 *   model_in[img][C:C + E] = s_next cond[nc == 1 ? 0 : img % n]   if cond is non-NULL; untouched if it is NULL
 * s_next = coef[7] for MI355X_COND_LINEAR, 1 for MI355X_COND_DDIM.  coef: the eight float32 of the existing kernels, in DEVICE memory.
 * hist is read and written by the LINEAR form only (may be NULL for DDIM).
 * EARG: x, unet_out, model_in or coef NULL; hist NULL with LINEAR; form or guided outside {0, 1}; n, C or hw <= 0; E < 0; nc outside {1, n}
 * when cond is given; model_in overlapping x, hist, unet_out or cond. */
int mi355x_cond_step(int32_t dtype, int32_t form, int32_t guided, void* x, const void* unet_out, void* hist, void* model_in, const void* cond,
                     const float* coef, int32_t n, int32_t C, int32_t E, int32_t nc, int64_t hw, void* stream);

/* mi355x_cond_fill -- primes a model input (set_inputs / the first step) and builds the second-pass input of Self-Attention Guidance
 * from the contiguous output of mi355x_sag_degrade:
 *   model_in[b][0:C]     = s x[b % n]                        if x is non-NULL
 *   model_in[b][C:C + E] = s cond[nc == 1 ? 0 : b % n]       if cond is non-NULL              for b < B, B = n or 2n
 * s is read from one float32 in DEVICE memory; a NULL s means 1.
 * EARG: model_in NULL; x and cond both NULL; cond given with E = 0; n, C or hw <= 0; E < 0; B outside {n, 2n}; nc outside {1, n} when
 * cond is given; model_in overlapping x or cond. */
int mi355x_cond_fill(int32_t dtype, const void* x, const void* cond, void* model_in, const float* s, int32_t n, int32_t B, int32_t C, int32_t E,
                     int32_t nc, int64_t hw, void* stream);

/* mi355x_inpaint_conditions -- what StableDiffusion_1_Inpainting.set_inpainting_conditions (stable_diffusion_1/model.py:259-286) computes
 * in front of the autoencoder, in one launch.
 *   image [n][H][W][3] uint8 (RGB, as numpy.array(pil_image) gives it);  mask [nm][H][W] uint8, nm = 1 or n
 *   m = (mask / 255 > 0.5);  v = image / 255 rounded to dtype;  t = 2 v - 1 rounded to dtype
 *   masked_image [n][3][H][W] (dtype)  = t (1 - m[nm == 1 ? 0 : img])
 *   mask_latents [nm][1][h][w] (dtype) = m at the source pixel of torch's `nearest` rule: min(floor(dst * (float(H) / h)), H - 1) per axis,
 *                                        evaluated in float32; any (h, w)
 * EARG: a NULL pointer; n, H, W, h or w <= 0; nm outside {1, n}. */
int mi355x_inpaint_conditions(int32_t dtype, const void* image, const void* mask, void* masked_image, void* mask_latents, int32_t n, int32_t nm,
                              int32_t H, int32_t W, int32_t h, int32_t w, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MI355X_REFINERS_COND_INPUT_H */
