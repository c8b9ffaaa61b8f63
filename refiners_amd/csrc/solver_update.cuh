// The solver updates of one latent element, shared by the guided kernels (elementwise.hip: eps = u + cfg (c - u)) and the guidance-free ones
// (solver_step.hip: eps = the UNet's output).  One set of expressions, so that a guidance-free step is bit-equal to the guided step on
// cat(out, out).  Sharing the SOURCE is not enough for that: which products the compiler fuses into the sums around them depends on the loop an
// expression is inlined into (a 16-byte vector loop fused a product the one-element loop left alone).  So contraction is off inside these
// functions and the fused operations are spelled out -- the ones the guided kernels have always run (the same list as multi_diffusion.hip's
// ddim_elem / linear_elem, which tests/test_multi_diffusion_kernels_gpu.py holds bit-equal to them), including the one place where the two
// storage types differ.  That difference (d fused in float32 storage, unfused in bfloat16) is HISTORICAL, not numerical: it is what the compiler
// chose in cfg_linear_kernel's two instantiations, and the guided path's results are pinned to it bit for bit.  Do not "fix" it.
// multi_diffusion.hip still carries its own copy of this list (ddim_elem / linear_elem); it can include this header instead.
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
// Exactly one more fused multiply-add around the list above, so kn = 0 gives what linear_update gives (sde_step.hip, both of its forms).
template <typename T>
MI_DEV float sde_update(float xv, float eps, float hv, float nz, float hx, float he, float kx, float ke, float kd, float kp, float kn, float& d) {
#pragma clang fp contract(off)
    return fmaf(kn, nz, linear_update<T>(xv, eps, hv, hx, he, kx, ke, kd, kp, d));
}
