// Every kernel variant of mvsgi_conv3d_f32 / mvsgi_conv3d_up2_f32 but the direct and head kernels, once (conv3d_variants.hpp expands
// it into the enum; conv3d.hip into the bf16-split and exact-fp32 launches and every reported name; conv3d_f16.hip into the
// fp16-split launches).  The argument text of a row is both the template argument list of its launch and the one in the name.
//
// MVSGI_MFMA(variant, NW, MW, WM, WN, TD, TH, TW, S): the exact-fp32 kernel conv3d_mfma_kernel (conv3d_f32mfma.hpp)
MVSGI_MFMA(V_S1_N16_B256, 1, 4, 4, 1, 4, 8, 8, 1)
MVSGI_MFMA(V_S1_N32_B256, 2, 4, 4, 1, 4, 8, 8, 1)
MVSGI_MFMA(V_S1_N32_B64, 2, 1, 4, 1, 2, 4, 8, 1)
MVSGI_MFMA(V_S1_N64_B128, 2, 4, 2, 2, 2, 8, 8, 1)
MVSGI_MFMA(V_S1_N64_B64, 2, 2, 2, 2, 2, 4, 8, 1)
MVSGI_MFMA(V_S2_N32_B64, 2, 1, 4, 1, 2, 4, 8, 2)
MVSGI_MFMA(V_S2_N64_B64, 2, 2, 2, 2, 2, 4, 8, 2)

// MVSGI_B3(variant, kernel, template arguments): the streaming split kernel (conv3d_bf16x3.hpp) in either split.  `kernel` is the
// suffix of its __global__ wrappers, conv3d_bf16x3<kernel> and conv3d_f16x3<kernel>; conv3d_variants.hpp maps it to the launch.
//
// _kernel (NW, MW, WM, WN, TD, TH, TW, S, KD, UPS, PLANE, V32, WLDS): 16-wide bricks (conflict-free LDS reads); N = couts per workgroup
MVSGI_B3(B3_N16, _kernel, 1, 4, 4, 1, 4, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N32, _kernel, 2, 4, 4, 1, 4, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N48, _kernel, 3, 4, 4, 1, 4, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N64, _kernel, 2, 4, 2, 2, 2, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N64_H5, _kernel, 2, 5, 2, 2, 2, 5, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N96, _kernel, 3, 4, 2, 2, 2, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N96_H5, _kernel, 3, 5, 2, 2, 2, 5, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N128_P, _kernel, 2, 4, 1, 4, 1, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N128_PH5, _kernel, 2, 5, 1, 4, 1, 5, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N192_PH5, _kernel, 3, 5, 1, 4, 1, 5, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N64_S, _kernel, 2, 2, 2, 2, 1, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_N16_TW, _kernel, 1, 1, 4, 1, 1, 4, 16, 1, 3, false, false, false, true)
MVSGI_B3(B3_N32_TB, _kernel, 1, 2, 2, 2, 1, 4, 16, 1, 3, false, false, false, false)
MVSGI_B3(B3_S2_N32B, _kernel, 1, 2, 2, 2, 2, 4, 8, 2, 3, false, false, false, false)
MVSGI_B3(B3_S2_N64, _kernel, 2, 2, 2, 2, 2, 4, 8, 2, 3, false, false, false, false)
MVSGI_B3(B3_S2_N96, _kernel, 3, 2, 2, 2, 2, 4, 8, 2, 3, false, false, false, false)
MVSGI_B3(B3_S2_N128, _kernel, 2, 4, 1, 4, 2, 4, 8, 2, 3, false, false, false, false)
MVSGI_B3(B3_S2_N192, _kernel, 3, 4, 1, 4, 2, 4, 8, 2, 3, false, false, false, false)
// bricks 10 rows x 8 columns: planes whose width is 8 mod 16 and whose height is a multiple of 10 (the 10 x 40 planes of UNet
// level 2) are covered exactly where the 5 x 16 bricks pad 40 columns to 48 (the siblings of the *_H5 / *_PH5 variants)
MVSGI_B3(B3_N64_W8, _kernel, 2, 5, 2, 2, 2, 10, 8, 1, 3, false, false, false, false)
MVSGI_B3(B3_N96_W8, _kernel, 3, 5, 2, 2, 2, 10, 8, 1, 3, false, false, false, false)
MVSGI_B3(B3_N128_PW8, _kernel, 2, 5, 1, 4, 1, 10, 8, 1, 3, false, false, false, false)
MVSGI_B3(B3_N192_PW8, _kernel, 3, 5, 1, 4, 1, 10, 8, 1, 3, false, false, false, false)
// with the trilinear x2 upsample fused into the producers (even bricks only)
MVSGI_B3(B3U_N16, _kernel, 1, 4, 4, 1, 4, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N32, _kernel, 2, 4, 4, 1, 4, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N32_M, _kernel, 2, 2, 4, 1, 2, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N48, _kernel, 3, 4, 4, 1, 4, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N64, _kernel, 2, 4, 2, 2, 2, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N96, _kernel, 3, 4, 2, 2, 2, 4, 16, 1, 3, true, false, false, false)
MVSGI_B3(B3U_N32_TB, _kernel, 1, 2, 2, 2, 2, 2, 16, 1, 3, true, false, false, false)
// Cout == 16 plane schedule (weights from mvsgi_conv3d_pack_weights_bf16x3_c16), plain and fused-upsample
MVSGI_B3(B3P_N16, _kernel, 1, 4, 4, 1, 4, 4, 16, 1, 3, false, true, false, false)
MVSGI_B3(B3PU_N16, _kernel, 1, 4, 4, 1, 4, 4, 16, 1, 3, true, true, false, false)
// 32x32x16 schedule (Cout % 32 == 0, stride 1; weights from mvsgi_conv3d_pack_weights_bf16x3_v32), plain / fused upsample
MVSGI_B3(B3V_N32, _kernel, 1, 2, 4, 1, 4, 4, 16, 1, 3, false, false, true, false)
MVSGI_B3(B3V_N64, _kernel, 1, 2, 2, 2, 2, 4, 16, 1, 3, false, false, true, false)
MVSGI_B3(B3VU_N32, _kernel, 1, 2, 4, 1, 4, 4, 16, 1, 3, true, false, true, false)
MVSGI_B3(B3VU_N64, _kernel, 1, 2, 2, 2, 2, 4, 16, 1, 3, true, false, true, false)
// _d32_kernel (NW, MW, WM, WN, TD, TH, TW): 32-channel slices (MVSGI_CONV_BF16X3_D32; weights from
// mvsgi_conv3d_pack_weights_split(layout D32)): Cin % 32 == 0, stride 1, the plain stride-1 bricks of up to 160 voxels (four 16-channel
// sub-images must fit the LDS), each the sibling of the B3_* variant of the same shape.  _d32_dk_kernel: with the depth skip -- the
// one-plane bricks (dispatched to one-plane volumes only) multiply the kd = 1 taps alone, the B3D2_* two-plane bricks (for volumes
// exactly two planes deep) two of the three kd per plane.
MVSGI_B3(B3D_N64, _d32_kernel, 2, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3D_N64_H5, _d32_kernel, 2, 5, 2, 2, 2, 5, 16)
MVSGI_B3(B3D_N64_W8, _d32_kernel, 2, 5, 2, 2, 2, 10, 8)
MVSGI_B3(B3D_N96, _d32_kernel, 3, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3D_N96_H5, _d32_kernel, 3, 5, 2, 2, 2, 5, 16)
MVSGI_B3(B3D_N96_W8, _d32_kernel, 3, 5, 2, 2, 2, 10, 8)
MVSGI_B3(B3D_N128_P, _d32_dk_kernel, 2, 4, 1, 4, 1, 4, 16)
MVSGI_B3(B3D_N128_PH5, _d32_dk_kernel, 2, 5, 1, 4, 1, 5, 16)
MVSGI_B3(B3D_N128_PW8, _d32_dk_kernel, 2, 5, 1, 4, 1, 10, 8)
MVSGI_B3(B3D_N192_PH5, _d32_dk_kernel, 3, 5, 1, 4, 1, 5, 16)
MVSGI_B3(B3D_N192_PW8, _d32_dk_kernel, 3, 5, 1, 4, 1, 10, 8)
// the small-launch units (a frame to a dozen)
MVSGI_B3(B3D_N32_TB, _d32_kernel, 1, 2, 2, 2, 1, 4, 16)
MVSGI_B3(B3D_N64_S, _d32_kernel, 2, 2, 2, 2, 1, 4, 16)
MVSGI_B3(B3D2_N64, _d32_dk_kernel, 2, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3D2_N64_H5, _d32_dk_kernel, 2, 5, 2, 2, 2, 5, 16)
MVSGI_B3(B3D2_N64_W8, _d32_dk_kernel, 2, 5, 2, 2, 2, 10, 8)
MVSGI_B3(B3D2_N96, _d32_dk_kernel, 3, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3D2_N96_H5, _d32_dk_kernel, 3, 5, 2, 2, 2, 5, 16)
MVSGI_B3(B3D2_N96_W8, _d32_dk_kernel, 3, 5, 2, 2, 2, 10, 8)
// _d32_dk2_kernel: one-plane small-launch units in a volume TWO planes deep (the window of 18 slots starts per unit)
MVSGI_B3(B3D2_N32_TB, _d32_dk2_kernel, 1, 2, 2, 2, 1, 4, 16)
MVSGI_B3(B3D2_N64_S, _d32_dk2_kernel, 2, 2, 2, 2, 1, 4, 16)
// _d32u_kernel: the fused upsample + conv on 32-channel slices (D32 + UPS): the 2 x 4 x 16 bricks (four 34.5 KB sub-images; the
// 4 x 4 x 16 bricks' would not fit).  _d32u_dk_kernel: with the depth skip, for an upsampled volume two planes deep.
MVSGI_B3(B3DU_N64, _d32u_kernel, 2, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3DU_N96, _d32u_kernel, 3, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3DU2_N64, _d32u_dk_kernel, 2, 4, 2, 2, 2, 4, 16)
MVSGI_B3(B3DU2_N96, _d32u_dk_kernel, 3, 4, 2, 2, 2, 4, 16)
