// Host-side check of the three entry points of refiners_amd/csrc/cond_input.hip: every refused-argument case returns its code before
// anything is launched (argument validation, overlap and grid arithmetic run on the host).  A stand-alone program, meant to be built with
// the host sanitizers and run on a machine WITHOUT a GPU -- no refused call reaches the HIP runtime:
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -Xarch_host -fsanitize=address,undefined -Xarch_host -fno-sanitize-recover=undefined \
//         refiners_amd/csrc/cond_input.hip tools/cond_input_refusals.cpp -o cond_input_refusals && ./cond_input_refusals
// The pointers are addresses inside one host array, never dereferenced: a refused call reads no operand.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../include/mi355x_refiners.h"
#include "../include/mi355x_refiners_cond_input.h"

static int failures = 0;
#define EXPECT(call, code)                                                              \
    do {                                                                                \
        const int got = (call);                                                         \
        if (got != (code)) { std::printf("FAIL %s -> %d, expected %d\n", #call, got, (code)); ++failures; } \
    } while (0)

int main() {
    const int n = 3, C = 4, E = 5, hw = 64;
    std::vector<float> arena(1 << 16);
    float* x = arena.data();                       // n C hw
    float* hist = x + n * C * hw;                  // n C hw
    float* uo = hist + n * C * hw;                 // 2 n C hw
    float* cond = uo + 2 * n * C * hw;             // n E hw
    float* mi = cond + n * E * hw;                 // 2 n (C + E) hw
    float* coef = mi + 2 * n * (C + E) * hw;       // 8
    const int F32 = MI355X_F32, LIN = MI355X_COND_LINEAR, DDIM = MI355X_COND_DDIM;

    // mi355x_cond_step
    EXPECT(mi355x_cond_step(F32, LIN, 1, nullptr, uo, hist, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, nullptr, hist, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, nullptr, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, nullptr, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, nullptr, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, 0, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, -1, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, n, 0, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, n, C, -1, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, n, C, E, n, 0, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, n, C, E, 2, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, n, C, 0, n, hw, nullptr), MI355X_EARG);  // constants given, E = 0
    EXPECT(mi355x_cond_step(F32, 2, 1, x, uo, hist, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, DDIM, 2, x, uo, hist, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, x, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);     // model_in over x
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, hist, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);  // ... over hist
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, uo, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);    // ... over unet_out
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, cond, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);  // ... over cond
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, cond - 1, cond, coef, n, C, E, n, hw, nullptr), MI355X_EARG);  // ... by one element
    EXPECT(mi355x_cond_step(7, LIN, 1, x, uo, hist, mi, cond, coef, n, C, E, n, hw, nullptr), MI355X_EDTYPE);
    // sizes whose products leave 64 bits: refused as a shape, never undefined behaviour
    EXPECT(mi355x_cond_step(F32, LIN, 1, x, uo, hist, mi, cond, coef, INT32_MAX, INT32_MAX, INT32_MAX, 1, (int64_t)1 << 40, nullptr), MI355X_ESHAPE);
    EXPECT(mi355x_cond_step(F32, LIN, 0, x, uo, hist, mi, nullptr, coef, 1, 1, 0, 1, INT64_MAX, nullptr), MI355X_ESHAPE);

    // mi355x_cond_fill
    EXPECT(mi355x_cond_fill(F32, x, cond, nullptr, nullptr, n, 2 * n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, nullptr, nullptr, mi, nullptr, n, 2 * n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, 0, 0, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, n + 1, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, 2 * n, 0, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, 2 * n, C, -1, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, 2 * n, C, 0, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, 2 * n, C, E, 2, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, n, 2 * n, C, E, n, 0, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, x, nullptr, n, 2 * n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(F32, x, cond, cond, nullptr, n, 2 * n, C, E, n, hw, nullptr), MI355X_EARG);
    EXPECT(mi355x_cond_fill(7, x, cond, mi, nullptr, n, 2 * n, C, E, n, hw, nullptr), MI355X_EDTYPE);
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, INT32_MAX, -2, C, E, 1, hw, nullptr), MI355X_EARG);  // 2n wraps to -2 in 32 bits: compared in 64
    EXPECT(mi355x_cond_fill(F32, x, cond, mi, nullptr, INT32_MAX, INT32_MAX, INT32_MAX, INT32_MAX, 1, (int64_t)1 << 40, nullptr), MI355X_ESHAPE);

    // mi355x_inpaint_conditions
    const uint8_t* img = reinterpret_cast<const uint8_t*>(arena.data());
    EXPECT(mi355x_inpaint_conditions(F32, nullptr, img, mi, x, 2, 2, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, nullptr, mi, x, 2, 2, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, nullptr, x, 2, 2, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, nullptr, 2, 2, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 0, 1, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 2, 3, 8, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 2, 2, 0, 8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 2, 2, 8, -8, 2, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 2, 2, 8, 8, 0, 2, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, 2, 2, 8, 8, 2, 0, nullptr), MI355X_EARG);
    EXPECT(mi355x_inpaint_conditions(F32, img, img, mi, x, INT32_MAX, 1, INT32_MAX, INT32_MAX, 2, 2, nullptr), MI355X_ESHAPE);
    EXPECT(mi355x_inpaint_conditions(7, img, img, mi, x, 2, 2, 8, 8, 2, 2, nullptr), MI355X_EDTYPE);

    std::printf("%s: %d refused-argument cases failed\n", failures ? "FAILED" : "ok", failures);
    return failures ? 1 : 0;
}
