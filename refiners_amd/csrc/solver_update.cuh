// The solver updates of one latent element, shared by every kernel that ends a denoising step: the flat kernel behind the six batch entry points
// (solver_step.hip: guided eps = u + cfg (c - u), or guidance-free eps = the UNet's output; DDIM, linear or SDE), cond_step_kernel (cond_input.hip)
// and md_target_step_kernel (multi_diffusion.hip).  One set of expressions, so that a guidance-free step is bit-equal to the guided step on
// cat(out, out), an SDE step with kn = 0 to the linear one, and a target under its own coefficient row to the batch.  Sharing the SOURCE is not
// enough for that: which products the compiler fuses into the sums around them depends on the loop an expression is inlined into (a 16-byte vector
// loop fused a product the one-element loop left alone).  So contraction is off inside these functions and the fused operations are spelled out --
// the ones the guided kernels have always run, including the one place where the two storage types differ.  That difference (d fused in float32
// storage, unfused in bfloat16) is HISTORICAL, not numerical: it is what the compiler chose in the two instantiations of the one-element-per-lane
// kernel the guided linear step once had, and the guided path's results are pinned to it bit for bit
// (tests/golden/solver_step_bits.safetensors).  Do not "fix" it.
#pragma once
#include "common.cuh"

// DDIM (solvers/ddim.py:56-95): x0 = (x - sqrt(1 - a_t) eps) / sqrt(a_t);  x' = sqrt(a_prev) x0 + sqrt(1 - a_prev) eps  (two products, one sum)
MI_DEV float ddim_update(float xv, float eps, float sa, float s1a, float sap, float s1ap) {
#pragma clang fp contract(off)
    const float x0 = fmaf(-s1a, eps, xv) / sa;
    return sap * x0 + s1ap * eps;
}

// Any solver linear in (x, eps, one kept quantity): d = hx x + he eps;  x' = kx x + ke eps + kd d + kp hist.  Returns x', leaves d in `d`.
// T = the storage type: d is one fused multiply-add in float32 storage and two products and a sum in bfloat16.
template <typename T> MI_DEV float linear_update(float xv, float eps, float hv, float hx, float he, float kx, float ke, float kd, float kp, float& d) {
#pragma clang fp contract(off)
    if constexpr (sizeof(T) == 4)
        d = fmaf(hx, xv, he * eps);
    else
        d = hx * xv + he * eps;
    return fmaf(kp, hv, fmaf(kd, d, fmaf(kx, xv, ke * eps)));
}

// The same with a fifth operand, the step's Gaussian draw (SDE DPM-Solver++ 2M, solvers/dpm.py:241-246, 284-290): x' = linear_update + kn noise.
// Exactly one more fused multiply-add around the list above, so kn = 0 gives what linear_update gives, guided or not.
template <typename T>
MI_DEV float sde_update(float xv, float eps, float hv, float nz, float hx, float he, float kx, float ke, float kd, float kp, float kn, float& d) {
#pragma clang fp contract(off)
    return fmaf(kn, nz, linear_update<T>(xv, eps, hv, hx, he, kx, ke, kd, kp, d));
}

// One latent element of a step's last launch.  k = the step's coefficient row: {cfg, sqrt(a_t), sqrt(1 - a_t), sqrt(a_prev), sqrt(1 - a_prev)} (DDIM),
// {cfg, hx, he, kx, ke, kd, kp, s_next} (LINEAR) or the same with kn behind it (SDE); a form reads only its own entries.  GUIDED: u, c = the
// unconditional and conditional halves of the UNet's output and eps = fma(cfg, c - u, u); otherwise eps = u.  Returns x', leaves the quantity the next
// step keeps in `d` (DDIM keeps nothing: 0).
enum StepForm { STEP_DDIM, STEP_LINEAR, STEP_SDE };
template <typename T, StepForm FORM, bool GUIDED> MI_DEV float step_elem(float xv, float u, float c, float hv, float nz, const float (&k)[9], float& d) {
#pragma clang fp contract(off)
    const float eps = GUIDED ? fmaf(k[0], c - u, u) : u;
    if constexpr (FORM == STEP_SDE) return sde_update<T>(xv, eps, hv, nz, k[1], k[2], k[3], k[4], k[5], k[6], k[8], d);
    if constexpr (FORM == STEP_LINEAR) return linear_update<T>(xv, eps, hv, k[1], k[2], k[3], k[4], k[5], k[6], d);
    d = 0.0f;
    return ddim_update(xv, eps, k[1], k[2], k[3], k[4]);
}
