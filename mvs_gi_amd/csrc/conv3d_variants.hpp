// Kernel variants of conv3d.hip (shared with conv3d_f16.hip, which holds the fp16-split instantiations of the split kernels): the
// enum of the rows of conv3d_variants.inc, and the launch of each split-kernel wrapper family.
#pragma once
namespace {
enum Variant {
    V_DIRECT1, V_DIRECT4, V_HEAD,
#define MVSGI_MFMA(V, ...) V,
#define MVSGI_B3(V, K, ...) V,
#include "conv3d_variants.inc"
#undef MVSGI_MFMA
#undef MVSGI_B3
    V_COUNT
};
}  // namespace

// launch_bf16x3 (conv3d_bf16x3.hpp) of a MVSGI_B3 row in the split F16, by its wrapper family: MVSGI_B3_LAUNCH##kernel(F16, args...)
#define MVSGI_B3_LAUNCH_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, F16>
#define MVSGI_B3_LAUNCH_d32_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, 1, 3, false, false, false, false, F16, true>
#define MVSGI_B3_LAUNCH_d32_dk_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, 1, 3, false, false, false, false, F16, true, true>
#define MVSGI_B3_LAUNCH_d32_dk2_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, 1, 3, false, false, false, false, F16, true, true, 3>
#define MVSGI_B3_LAUNCH_d32u_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, 1, 3, true, false, false, false, F16, true>
#define MVSGI_B3_LAUNCH_d32u_dk_kernel(F16, ...) launch_bf16x3<__VA_ARGS__, 1, 3, true, false, false, false, F16, true, true>

namespace mvsgi {
// conv3d_f16.hip: the split kernel variants (B3*) in the fp16 split; `args` is a ConvArgs
int conv3d_launch_b3_f16(int variant, const void* args, hipStream_t st);
}  // namespace mvsgi
