// Instantiations of the 8-wave / eight-phase main loop (gemm8_kernel.cuh): plain GEMM and implicit-GEMM convolution, bf16 and f32 (parity mode);
// entered through mi355x_gemm (gemm.hip) for the tile configurations of that loop (gemm_tiles.cuh).
#include "gemm8_kernel.cuh"

namespace mi355x {
int launch_gemm8_f32(const GemmP& p, hipStream_t stream, const Tile& t) { return launch_gemm8<float, false>(p, stream, t); }
int launch_gemm8_bf16(const GemmP& p, hipStream_t stream, const Tile& t) { return launch_gemm8<bf16_t, false>(p, stream, t); }
int launch_conv8_f32(const GemmP& p, hipStream_t stream, const Tile& t) { return launch_gemm8<float, true>(p, stream, t); }
int launch_conv8_bf16(const GemmP& p, hipStream_t stream, const Tile& t) { return launch_gemm8<bf16_t, true>(p, stream, t); }
}  // namespace mi355x
