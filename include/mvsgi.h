/*
 * mvsgi.h -- C ABI of the MI355X (gfx950) plane-sweep hot path of castacks/mvs_gi.
 *
 * The reference is pure Python/PyTorch and has no FFI of its own; the precedent for
 * handing this path raw device pointers is its TensorRT back end
 * (api/inference_trt.py:128-142, context.execute_async_v2 with device addresses).
 * Each entry point below replaces one stage of
 *   dsta_mvs/model/mvs_model/torch_only.py:32-34
 *     vol   = cv_builder(feats, grids, grid_masks, masks)
 *     costs = cv_regulator(vol)
 *     inv_dist, norm_costs = dist_regressor(costs)
 * and is what a ctypes / cgo / JNI binding on the reference side would bind
 * (INTEGRATION.md shows the ctypes stub that mvs_gi_amd/_lib.py uses).
 *
 * Conventions
 *   - every pointer is a DEVICE pointer (HBM), caller-owned, never freed or retained;
 *   - `stream` is a hipStream_t passed as void* (0 = the null stream); all work is
 *     enqueued on it and nothing synchronises the host;
 *   - activations are fp32, channels-last: [B][D][H][W][C] ("NDHWC"); the 2-D inputs of
 *     the sweep keep the reference's own layouts (stated per function);
 *   - return value: 0 = enqueued, non-zero = rejected (nothing enqueued);
 *     mvsgi_last_error() returns a thread-local description of the last failure
 *     (the Python layer raises RuntimeError with it, mirroring the reference's
 *     assert/exception behaviour, e.g. backports.py:32).
 *   - no global mutable state but the range report's sticky words (mvsgi_saturation_flags):
 *     every call is re-entrant per stream, one process per GPU.
 */
#ifndef MVSGI_H
#define MVSGI_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MVSGI_ABI_VERSION 8   /* 8: mvsgi_reproject_f32 (back-projection: point cloud and warped camera views), and, added later without a new number (an addition: older callers are unaffected, and the binding refuses a library that lacks a symbol it binds), mvsgi_metrics_f32, mvsgi_metrics_ws_bytes (validation metrics), mvsgi_cloud_pack_f32, mvsgi_cloud_ws_bytes (packed point cloud), mvsgi_losses_f32, mvsgi_losses_ws_bytes (loss functions), mvsgi_photo_consistency_f32, mvsgi_photo_ws_bytes (photometric consistency); 7: mvsgi_resample_bilinear_u8_f32, mvsgi_resample_bilinear_f32, mvsgi_resample_validity_u8, mvsgi_resample_u8_table_f32, mvsgi_rays_equirect_surrogate_f32 (fisheye -> surrogate-view resampler); 6: mvsgi_sweep_max_cams (masked-variance sweep for rigs of up to 8 cameras); 5: mvsgi_softargmin_scaled_f32 (soft-argmin at any interp_scale_factor); 4: mvsgi_instance_norm_f32, mvsgi_instance_norm_ws_bytes (norm_type 'instance'); 3: mvsgi_conv3d_d32_applies, mvsgi_conv3d_up2_d32_applies + MVSGI_CONV_BF16X3_D32; 2: mvsgi_saturation_flags; the symbol set of round 5 */

typedef void* mvsgi_stream_t;

/* conv3d implementation selector */
#define MVSGI_CONV_AUTO   0   /* MFMA implicit GEMM when Cin%16==0 && Cout%16==0, else direct */
#define MVSGI_CONV_DIRECT 1   /* VALU direct convolution (any channel counts; Cout==1 head)   */
#define MVSGI_CONV_MFMA   2   /* LDS-tiled: v_mfma_f32_16x16x4_f32 implicit GEMM (exact fp32),
                                 or the LDS-tiled VALU head kernel when Cout == 1               */
#define MVSGI_CONV_BF16X3 3   /* split-bf16 implicit GEMM on v_mfma_f32_16x16x32_bf16: x = hi + lo,
                                 hi*hi + hi*lo + lo*hi, fp32 accumulate (~2^-16 per product);
                                 w_packed must come from mvsgi_conv3d_pack_weights_bf16x3.
                                 Falls back to the exact paths for Cout == 1 / odd channel counts */
#define MVSGI_CONV_BF16X3_C16 4 /* the same arithmetic for Cout == 16, stride 1 (post_vol, out_costs.0): "plane"
                                   schedule -- one activation fragment feeds the kd = 0, 1, 2 taps of three output
                                   planes -- with weights from mvsgi_conv3d_pack_weights_bf16x3_c16            */
#define MVSGI_CONV_BF16X3_V32 5 /* the same arithmetic on v_mfma_f32_32x32x16_bf16 (one tap x 16 channels per MFMA, half the
                                   issue-port time per flop) where mvsgi_conv3d_v32_applies(); weights from
                                   mvsgi_conv3d_pack_weights_bf16x3_v32                                                  */
#define MVSGI_CONV_BF16X3_D32 6 /* the same arithmetic on 32-channel slices: the K = 32 of an MFMA is ONE tap of 32 input channels
                                   (27 k-steps per 32 channels; the tap-pair layout of MVSGI_CONV_BF16X3 needs 28, its 14th pair
                                   half empty) and a unit has half as many slices to synchronise on.  Cin % 32 == 0, stride 1, launches
                                   large enough for a 128- / 160-voxel brick: where mvsgi_conv3d_d32_applies(); weights from
                                   mvsgi_conv3d_pack_weights_split(layout = MVSGI_CONV_BF16X3_D32 [| MVSGI_CONV_F16]), sized by
                                   mvsgi_conv3d_packed_weight_bytes_bf16x3 (the packer zeroes the 28th k-step's share).  Same products, another order. */

#define MVSGI_CONV_F16 0x100   /* FLAG, OR-ed into MVSGI_CONV_BF16X3 / _C16 / _V32 (impl of mvsgi_conv3d_f32, w_layout of
                                  mvsgi_conv3d_up2_f32, layout of mvsgi_conv3d_pack_weights_split): the same kernels and packed
                                  layouts in the fp16 split ("f16x3") -- hi = fp16(x), lo = fp16(x - hi), v_mfma_*_f16: 11 + 11
                                  significant bits per operand instead of 8 + 8 at the same matrix rate (~10x closer to the
                                  fp32 reference); operands are clamped to fp16's range (+-65504), and callers pre-scale each
                                  output channel's weights by a power of two (undone in `scale`) so that their lo parts are
                                  normal fp16 numbers                                                                    */

#define MVSGI_SPLIT_F16 1      /* `fmt` of the *_fmt entry points: split-padded activations / packed weights hold fp16 pairs (the
                                  "f16x3" arithmetic, see MVSGI_CONV_F16) instead of bf16 pairs (fmt 0)                     */

int         mvsgi_abi_version(void);
const char* mvsgi_last_error(void);

/* ---- range report of the fp16 split ------------------------------------------------------
 * The reference computes in fp32 with no clamp (dsta_mvs/model/common/common_modules.py:105-115,
 * distance_regressor/distance_regressor.py:51-79); the "f16x3" arithmetic (MVSGI_CONV_F16 / MVSGI_SPLIT_F16) saturates
 * what it writes or stages in fp16 pieces at +-65504, and the Winograd level's fp32-padded records at +-16376.  Every
 * kernel that clamps reports a clamp that ENGAGED (a value at or beyond the bound) into sticky per-process words of pinned
 * host memory; this call reads them (no stream operation, no copy: ask after synchronising the streams whose launches
 * the question is about) and optionally clears them.  Results computed while a bit was raised are NOT the reference's:
 * re-run in the bf16 split (fmt 0 / no MVSGI_CONV_F16: fp32's range) or in the exact fp32 mode.
 *   flags  out, may be NULL: OR of the MVSGI_SAT_* bits raised since the last clear
 */
#define MVSGI_SAT_SWEEP 1u     /* the sweep's split-padded cost volume (the one un-normalised tensor of the path) reached +-65504 */
#define MVSGI_SAT_SPLIT 2u     /* an activation written or staged in fp16 pieces by a conv layer reached +-65504                */
/* (MVSGI_SAT_SPLIT, out of range: the Winograd-form polyphase layer's fp16-pair output saturates hi and lo separately and can reach
 * 2 x 65504; its fp32-record output, mvsgi_conv3d_up2_poly_rec32, is unclamped and mvsgi_conv3d_head_rec32_f16 clamps what it loads
 * to exactly +-65504 -- the bit is raised in both forms, by the writer in the first and by the reader in the second.) */
#define MVSGI_SAT_WINO  4u     /* an activation of the Winograd level reached +-16376, or a transformed sum of four +-65504      */
int mvsgi_saturation_flags(int clear, unsigned* flags);
int mvsgi_saturation_words(unsigned* words8);      /* diagnostics: the 8 raw words (a kernel only ever stores 1 into one of them) */

/* ---- K1: fused spherical sweep -------------------------------------------------------
 * Replaces SphericalSweepStdMasked.sweep (cost_volume_builder/spherical_sweep_avg.py:38-136)
 * including both bilinear_grid_sample calls per candidate (backports/backports.py:34-86).
 *   feats      [B][N][C][Hi][Wi]      fp32 (the feature extractor's NCHW output)
 *   grids      [B][N][D][Ho][Wo][2]   fp32 normalised (x, y), align_corners=False
 *   grid_masks [B][N][D][Ho][Wo][1]   uint8/bool (grid_mask_is_f32 == 0) or fp32 (== 1)
 *   masks      [B][N][1][Hm][Wm]      fp32
 *   vol        [B][D][Ho][Wo][C]      fp32 out: population variance over the valid cameras,
 *                                     0 where fewer than two cameras are valid
 * N <= mvsgi_sweep_max_cams() (8: one validity bit per camera in a byte); the cameras are added in order, camera 0 first.
 */
int mvsgi_sweep_max_cams(void);
int mvsgi_sweep_std_f32(const float* feats, const float* grids, const void* grid_masks,
                        int grid_mask_is_f32, const float* masks, float* vol,
                        int B, int N, int C, int Hi, int Wi, int Hm, int Wm,
                        int D, int Ho, int Wo, mvsgi_stream_t stream);

/* Replaces SphericalSweep.sweep (cost_volume_builder/spherical_sweep.py:38-68):
 *   vol [B][D][Ho][Wo][N*C], channel = cam*C + c (spherical_sweep.py:60-61). */
int mvsgi_sweep_cat_f32(const float* feats, const float* grids, float* vol,
                        int B, int N, int C, int Hi, int Wi,
                        int D, int Ho, int Wo, mvsgi_stream_t stream);

/* The same two sweeps on channels-last feature maps, feats [B][N][Hi][Wi][C] (C % 4 == 0; mvsgi_sweep_std_nhwc_f32: N <= 4,
 * the kernels that read the validity byte below: N <= 8):
 * one 64-byte texel per tap instead of C strided planes.  The Python layer transposes the
 * feature extractor's NCHW output once (mvsgi_ncv_to_nvc_f32) unless it already is channels-last. */
int mvsgi_sweep_std_nhwc_f32(const float* feats, const float* grids, const void* grid_masks,
                             int grid_mask_is_f32, const float* masks, float* vol,
                             int B, int N, int C, int Hi, int Wi, int Hm, int Wm,
                             int D, int Ho, int Wo, mvsgi_stream_t stream);
int mvsgi_sweep_cat_nhwc_f32(const float* feats, const float* grids, float* vol,
                             int B, int N, int C, int Hi, int Wi,
                             int D, int Ho, int Wo, mvsgi_stream_t stream);

/* Rig-constant validity.  The mask half of SphericalSweepStdMasked.sweep -- (bilinear_grid_sample(
 * masks) > 0) & grid_masks, spherical_sweep_avg.py:92-102 -- depends only on grids / grid_masks /
 * masks, which the reference builds once per camera rig (api/inference_class.py:40-45).
 * mvsgi_sweep_validity_u8 evaluates it once into vmask [B][D][Ho][Wo] (bit cam set = camera cam is
 * valid; N <= 8); mvsgi_sweep_std_nhwc_valid_f32 is mvsgi_sweep_std_nhwc_f32 reading that byte
 * instead of re-sampling the masks every frame, for N <= 8 (five cameras and more: two groups of four per lane quad).
 * Bit-identical output. */
int mvsgi_sweep_validity_u8(const float* grids, const void* grid_masks, int grid_mask_is_f32,
                            const float* masks, unsigned char* vmask,
                            int B, int N, int Hm, int Wm, int D, int Ho, int Wo, mvsgi_stream_t stream);
int mvsgi_sweep_std_nhwc_valid_f32(const float* feats, const float* grids, const unsigned char* vmask,
                                   float* vol, int B, int N, int C, int Hi, int Wi,
                                   int D, int Ho, int Wo, mvsgi_stream_t stream);
/* The same with ONE rig for the whole batch: grids [1][N][D][Ho][Wo][2], vmask [1][D][Ho][Wo] (the rig constants are
 * frame-independent, api/inference_class.py:40-45); feats / vol keep their batch. */
int mvsgi_sweep_std_nhwc_valid_rig_f32(const float* feats, const float* grids, const unsigned char* vmask,
                                       float* vol, int B, int N, int C, int Hi, int Wi, int D, int Ho, int Wo,
                                       mvsgi_stream_t stream);

/* ---- K2: 3x3x3 convolution block -----------------------------------------------------
 * Replaces BaseConvBlk3d.forward (common/common_modules.py:107-115):
 *   y = act( conv3d(x, w, pad=1, stride) * scale[co] + shift[co] (+ res) )
 * eval-mode BatchNorm3d is the per-channel (scale, shift); a conv bias is shift with
 * scale = 1; act(v) = v > 0 ? v : v * neg_slope  (LeakyReLU: 0.01, ReLU: 0, identity: 1).
 *   x   [B][Din][Hin][Win][Cin]   y / res [B][Do][Ho][Wo][Cout],  Do = (Din-1)/stride+1 ...
 *   w_packed: output of mvsgi_conv3d_pack_weights_f32 (needed by the tiled paths -- MFMA, and
 *             the Cout == 1 cost head; may be NULL when impl == MVSGI_CONV_DIRECT);
 *   w_oidhw:  the PyTorch [Cout][Cin][3][3][3] tensor (needed by the direct path; may be NULL
 *             when impl == MVSGI_CONV_MFMA).
 * mvsgi_conv3d_variant_f32 names the kernel the dispatcher will launch for a problem (the
 * demangled kernel name as rocprofv3 prints it; NULL + last_error when unservable), so that
 * a benchmark can attribute time to the kernel that actually ran.
 */
size_t mvsgi_conv3d_packed_weight_floats(int Cout, int Cin);
int mvsgi_conv3d_pack_weights_f32(const float* w_oidhw, float* w_packed, int Cout, int Cin,
                                  mvsgi_stream_t stream);
size_t mvsgi_conv3d_packed_weight_bytes_bf16x3(int Cout, int Cin);
int mvsgi_conv3d_pack_weights_bf16x3(const float* w_oidhw, void* w_packed, int Cout, int Cin,
                                     mvsgi_stream_t stream);
/* weights for a split kernel in either split: layout = MVSGI_CONV_BF16X3 | _C16 | _V32, optionally | MVSGI_CONV_F16; w_packed sized by
 * mvsgi_conv3d_packed_weight_bytes_bf16x3 / _c16 / _v32 (the two splits share the layouts) */
int mvsgi_conv3d_pack_weights_split(const float* w_oidhw, void* w_packed, int Cout, int Cin, int layout, mvsgi_stream_t stream);
int mvsgi_conv3d_f32(const float* x, const float* w_oidhw, const float* w_packed,
                     const float* scale, const float* shift, const float* res, float* y,
                     int B, int Cin, int Din, int Hin, int Win, int Cout,
                     int stride, float neg_slope, int impl, mvsgi_stream_t stream);
const char* mvsgi_conv3d_variant_f32(int B, int Cin, int Din, int Hin, int Win, int Cout,
                                     int stride, int impl);

/* ResizeConv3d.forward (common/common_modules.py:332-355) in ONE launch: the trilinear x2 upsample
 * (F.interpolate, align_corners=False) of x [B][Dl][Hl][Wl][Cin] is evaluated inside the convolution's
 * staging path, so neither the resize kernel nor the upsampled tensor exist:
 *   y [B][2Dl][2Hl][2Wl][Cout] = act( conv3d(upsample2(x), w, pad=1) * scale + shift (+ res) )
 * Split-bf16 MFMA arithmetic; w_packed from mvsgi_conv3d_pack_weights_bf16x3; Cin, Cout % 16 == 0.
 * (Odd target sizes -- the second re-interpolation of :343-350 -- use mvsgi_resize_trilinear_f32 + mvsgi_conv3d_f32.) */
int mvsgi_conv3d_up2_f32(const float* x, const void* w_packed, int w_layout /* MVSGI_CONV_BF16X3 | _C16 | _V32 */,
                         const float* scale, const float* shift, const float* res, float* y,
                         int B, int Cin, int Dl, int Hl, int Wl, int Cout, float neg_slope, mvsgi_stream_t stream);
const char* mvsgi_conv3d_up2_variant_f32(int B, int Cin, int Dl, int Hl, int Wl, int Cout, int w_layout);
/* 32x32x16-MFMA schedule (MVSGI_CONV_BF16X3_V32): Cout % 32 == 0, stride 1, enough bricks to fill the chip */
int mvsgi_conv3d_v32_applies(int B, int Cin, int Din, int Hin, int Win, int Cout, int stride);
/* 1 when mvsgi_conv3d_f32 accepts impl = MVSGI_CONV_BF16X3_D32 [| MVSGI_CONV_F16] for this problem (replaces nothing in the reference:
 * a second schedule of BaseConvBlk3d's convolution, dsta_mvs/model/common/common_modules.py:107-115) */
int mvsgi_conv3d_d32_applies(int B, int Cin, int Din, int Hin, int Win, int Cout, int stride);
/* ... and mvsgi_conv3d_up2_f32 with w_layout = MVSGI_CONV_BF16X3_D32 (ResizeConv3d, common_modules.py:332-355; low-resolution sizes) */
int mvsgi_conv3d_up2_d32_applies(int B, int Cin, int Dl, int Hl, int Wl, int Cout);
size_t mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(int Cout, int Cin);
int mvsgi_conv3d_pack_weights_bf16x3_v32(const float* w_oidhw, void* w_packed, int Cout, int Cin, mvsgi_stream_t stream);
/* weights of a Cout == 16 layer in the plane-schedule layout (MVSGI_CONV_BF16X3_C16) */
size_t mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(int Cin);
int mvsgi_conv3d_pack_weights_bf16x3_c16(const float* w_oidhw, void* w_packed, int Cin, mvsgi_stream_t stream);

/* ---- K2-2D: convolution block of the feature extractor ----------
 * Replaces BaseConvBlk2d.forward (common/common_modules.py:56-70) on channels-last images:
 *   y = act( conv2d(x, w, pad k/2, stride) * scale[co] + shift[co] (+ res) )
 *   x [B][Hin][Win][Cin]; in_nchw == 1: the caller's fp32 NCHW images (direct path only);
 *   in_nchw == 2: uint8 [B][Hin][Win][3] camera images, converted as `.float() / 255.0`
 *   (api/inference_class.py:104-107) inside the 5x5 stride-2 3->16 stem kernel,
 *   y / res [B][Ho][Wo][Cout], w_oihw [Cout][Cin][k][k], k odd <= 7, stride 1|2.
 * impl: MVSGI_CONV_BF16X3 = split-bf16 MFMA kernel (k == 3, Cin, Cout multiples of 16, w_packed from
 * mvsgi_conv2d_pack_weights_bf16x3); MVSGI_CONV_MFMA = exact fp32 MFMA kernel (k == 3, Cin % 16 == 0,
 * Cout in {16, 32}, w_packed from mvsgi_conv2d_pack_weights_f32); anything else, or AUTO/DIRECT = exact
 * fp32 direct kernels (incl. the LDS-tiled 5x5 stride-2 RGB stem). */
size_t mvsgi_conv2d_packed_weight_floats(int Cout, int Cin);            /* exact-fp32 MFMA path (MVSGI_CONV_MFMA) */
int mvsgi_conv2d_pack_weights_f32(const float* w_oihw, float* w_packed, int Cout, int Cin,
                                  mvsgi_stream_t stream);
/* uint8 HWC camera images into the 5x5 stride-2 3 -> 16 stem (simple_feature_extractor.py:21-31 after the /255 of
 * api/inference_class.py:104-107): weights / 255 cut into three bf16 pieces for the matrix cores.  Pass the packed buffer
 * as w_packed of mvsgi_conv2d_f32 together with in_nchw == 2 (needs Win % 4 == 0; otherwise the LDS-tiled kernel runs). */
size_t mvsgi_conv2d_stem_packed_weight_bytes(void);
int mvsgi_conv2d_stem_pack_weights(const float* w_oihw, void* w_packed, mvsgi_stream_t stream);
size_t mvsgi_conv2d_packed_weight_bytes_bf16x3(int Cout, int Cin);
int mvsgi_conv2d_pack_weights_bf16x3(const float* w_oihw, void* w_packed, int Cout, int Cin,
                                     mvsgi_stream_t stream);
int mvsgi_conv2d_f32(const float* x, const float* w_oihw, const void* w_packed,
                     const float* scale, const float* shift, const float* res, float* y,
                     int B, int Cin, int Hin, int Win, int Cout, int ksize, int stride,
                     float neg_slope, int impl, int in_nchw, mvsgi_stream_t stream);
const char* mvsgi_conv2d_variant_f32(int Cin, int Cout, int ksize, int stride, int impl, int in_nchw);

/* ---- K3: trilinear resize ------------------------------------------------------------
 * Replaces F.interpolate(mode='trilinear', align_corners=False, size=...) inside
 * ResizeConv3d.forward (common/common_modules.py:333-350), for x2 and for the odd-size
 * re-interpolation to the skip tensor's shape.  x [B][Di][Hi][Wi][C] -> y [B][Do][Ho][Wo][C]. */
int mvsgi_resize_trilinear_f32(const float* x, float* y, int B, int C,
                               int Di, int Hi, int Wi, int Do, int Ho, int Wo,
                               mvsgi_stream_t stream);

/* ---- K4: fused upsample + soft-argmin ------------------------------------------------
 * Replaces DistanceRegressorWithFixedCandidates.forward (distance_regressor/
 * distance_regressor.py:51-79): bilinear x`scale` (scale in {1,2}; 1 = no interpolation; other factors: mvsgi_softargmin_scaled_f32),
 * softmax over D, expectation of inv_idx[d] = bf / dist[d].
 *   costs [B][D][H][W] (the C==1 volume), inv_idx [D],
 *   inv_dist [B][1][sH][sW], norm_costs [B][D][sH][sW] or NULL (inference discards it). */
int mvsgi_softargmin_f32(const float* costs, const float* inv_idx, float* inv_dist,
                         float* norm_costs, int B, int D, int H, int W, int scale,
                         mvsgi_stream_t stream);

/* Same with the post-processing of api/inference_class.py:111-114 folded in: inv_dist is divided by
 * post_div (= bf) after the expectation (post_div == 1 reproduces mvsgi_softargmin_f32). */
int mvsgi_softargmin_div_f32(const float* costs, const float* inv_idx, float* inv_dist,
                             float* norm_costs, int B, int D, int H, int W, int scale,
                             float post_div, mvsgi_stream_t stream);

/* The same at any factor F.interpolate(scale_factor = scale, mode = 'bilinear', align_corners = False) accepts (scale finite
 * and > 0; fractional and down-scaling factors included).  OH, OW are the output sizes the caller allocated; they must equal
 * floor(H * scale), floor(W * scale) as computed here in double, anything else is rejected (never an overrun).
 *   inv_dist [B][1][OH][OW], norm_costs [B][D][OH][OW] or NULL.
 * scale 1 and 2 forward to mvsgi_softargmin_div_f32 (identical results); integer factors 3 .. 64 take a row-band kernel that
 * stages each low-resolution row pair in LDS once; every other factor takes a thread-per-pixel kernel (correct, not tuned).
 * variant: MVSGI_SA_AUTO, or MVSGI_SA_PIXEL / MVSGI_SA_BAND to force one kernel (BAND: integer factors 3 .. 64 only). */
#define MVSGI_SA_AUTO  0
#define MVSGI_SA_PIXEL 1
#define MVSGI_SA_BAND  2
int mvsgi_softargmin_scaled_f32(const float* costs, const float* inv_idx, float* inv_dist,
                                float* norm_costs, int B, int D, int H, int W, double scale,
                                int OH, int OW, float post_div, int variant, mvsgi_stream_t stream);

/* ---- confidence maps of the soft-argmin's softmax (an addition beyond the reference's interface) -------------------------
 * Per output pixel of mvsgi_softargmin_scaled_f32 (same coordinate rule, output size floor(in * scale), zero-weight tap rule
 * and fp32 weights), with v_d the blended cost of candidate d, m = max_d v_d, g_d = m - v_d, e_d = exp(-g_d), S = sum e_d,
 * p_d = e_d / S and mu = sum p_d inv_idx[d]:
 *   max_prob [B][1][OH][OW] fp32   max_d p_d = 1 / S
 *   entropy  [B][1][OH][OW] fp32   -sum p_d ln p_d = ln S + (sum e_d g_d) / S, natural log; normalize_entropy != 0: divided by
 *                                  ln D (D == 1: 0 either way)
 *   spread   [B][1][OH][OW] fp32   sqrt(sum p_d (inv_idx[d] - mu)^2) / post_div: the unit of inv_dist / post_div
 *   argmax   [B][1][OH][OW] int32  the lowest d with v_d == m; -1 where the float maps are NaN
 * Any of the four outputs may be NULL (that map is neither computed for storing nor stored), not all of them.  One launch on
 * `stream`, no atomics, no host synchronisation, no workspace: capturable.  A NaN or +inf cost under a non-zero weight, or
 * every candidate -inf, gives NaN / -1 at that pixel; a single -inf candidate has p = 0 exactly.
 * Returns non-zero (mvsgi_last_error()) on a non-finite or non-positive scale, OH / OW other than floor(H * scale),
 * floor(W * scale) as computed here in double, post_div == 0, or four NULL outputs. */
int mvsgi_confidence_f32(const float* costs, const float* inv_idx, float* max_prob, float* entropy,
                         float* spread, int* argmax, int B, int D, int H, int W, double scale,
                         int OH, int OW, float post_div, int normalize_entropy, mvsgi_stream_t stream);

/* ---- layout helpers for the module boundary ------------------------------------------
 * [B][C][D*H*W] <-> [B][D*H*W][C]; V = D*H*W.  Used when a caller hands the regulator a
 * contiguous NCDHW tensor (e.g. produced by the reference's own cv_builder). */
int mvsgi_ncv_to_nvc_f32(const float* x, float* y, int B, int C, long long V, mvsgi_stream_t stream);
int mvsgi_nvc_to_ncv_f32(const float* x, float* y, int B, int C, long long V, mvsgi_stream_t stream);

/* ResConvBlk2d.forward (common/common_modules.py:165-176) for 16 -> 16 channels, 3x3, stride 1 in ONE launch
 * (the extractor's residual blocks are HBM-bound; fused, the intermediate never leaves the CU):
 *   y = act( conv2( act( conv1(x) * scale1 + shift1 ) ) * scale2 + shift2 + x ),   x / y [N][H][W][16], x != y
 * w_packed1 / w_packed2 from mvsgi_conv2d_pack_weights_bf16x3(Cout = Cin = 16); split-bf16 MFMA arithmetic. */
int mvsgi_resblock2d_f32(const float* x, const void* w_packed1, const float* scale1, const float* shift1,
                         const void* w_packed2, const float* scale2, const float* shift2, float* y,
                         int N, int H, int W, float neg_slope, mvsgi_stream_t stream);

/* The same block on PRE-SPLIT activations (csrc/resblock2d_rs.hip): the extractor's chain of residual blocks hands its
 * activations on in the 2-D split-padded format
 *   [N][H + 4][W + 4][64 B],  pixel record = [hi(c 0-7) | hi(c 8-15) | lo(c 0-7) | lo(c 8-15)] bf16,  x = hi + lo,
 * with a two-pixel zero border that no kernel writes (the caller zeroes a buffer once; mvsgi_split2d_bytes gives its size).
 * Staging is then a pure copy (LDS-DMA), two workgroups share a CU, and the skip connection is read from LDS.
 * w_packed1 / w_packed2 from mvsgi_resblock2d_split_pack_weights ([16][16][3][3] fp32 each, the per-channel scale folded
 * in: y = act(conv2'(act(conv1'(x) + shift1)) + shift2 + x)).  y: the same format
 * (y_is_split != 0) or plain fp32 [N][H][W][16] (the hand-over to a kernel that stages fp32).  x_split != y.
 * mvsgi_conv2d_f32_out_split2d = mvsgi_conv2d_f32 writing that format (Cout == 16: the RGB stem and the split-bf16 3x3
 * kernels); mvsgi_f32_to_split2d / mvsgi_split2d_to_f32 convert at module boundaries and in tests. */
size_t mvsgi_split2d_bytes(int N, int H, int W);
int mvsgi_f32_to_split2d(const float* x, void* y_split, int N, int H, int W, mvsgi_stream_t stream);
int mvsgi_split2d_to_f32(const void* x_split, float* y, int N, int H, int W, mvsgi_stream_t stream);
size_t mvsgi_resblock2d_split_packed_weight_bytes(void);
int mvsgi_resblock2d_split_pack_weights(const float* w_oihw, const float* scale, void* w_packed, mvsgi_stream_t stream);
int mvsgi_resblock2d_split(const void* x_split, const void* w_packed1, const float* shift1,
                           const void* w_packed2, const float* shift2, void* y, int y_is_split,
                           int N, int H, int W, float neg_slope, mvsgi_stream_t stream);
/* BaseConvBlk2d 16 -> 16, 3x3, stride 2 between two runs of residual blocks, split-padded in and out (w_packed from
 * mvsgi_resblock2d_split_pack_weights): y_split [N][Ho+4][Wo+4][64 B], Ho = (H - 1) / 2 + 1 */
int mvsgi_conv2d_s2_split(const void* x_split, const void* w_packed, const float* shift, void* y_split,
                          int N, int H, int W, float neg_slope, mvsgi_stream_t stream);
int mvsgi_conv2d_f32_out_split2d(const float* x, const float* w_oihw, const void* w_packed,
                                 const float* scale, const float* shift, const float* res, void* y_split,
                                 int B, int Cin, int Hin, int Win, int Cout, int ksize, int stride,
                                 float neg_slope, int impl, int in_nchw, mvsgi_stream_t stream);

/* ---- sampling-grid generator ---------------------------------------
 * The closed forms of dsta_mvs/support/dataset/torch_cuda_sweep.py, composed as
 * MultiViewCameraModelDataset.make_sweep_grid_cuda does (support/dataset/multi_view_camera_model_dataset.py:474-521):
 *   rays   = RayMaker_UEPanorama.make_rays_for_candidates        (:76-132)   [3][N][H][W]
 *   points = transform_3D_points_torch(inverse camera pose, rays) (:385-408)  [B][3][M]
 *   grid, mask = DoubleSphereSampleGridMaker.make_grid(points)    (:262-298)  [B][M][2], [B][M] u8
 *   grid       = EquirectangularSampleGridMaker.make_grid(points) (:305-335)  [B][M][2]
 * fp32, operation order of the reference's torch expressions.  Run once per rig. */
int mvsgi_rays_panorama_f32(const float* dist, float* rays, int N, int H, int W,
                            float lat0, float lat1, float lon0, float lon1, mvsgi_stream_t stream);
int mvsgi_transform_points_f32(const float* T /* [B][4][4] */, const float* points, float* out,
                               int B, long long M, mvsgi_stream_t stream);
int mvsgi_grid_double_sphere_f32(const float* points, float* grid, unsigned char* mask, int B, long long M,
                                 float xi, float alpha, float fx, float fy, float cx, float cy,
                                 int calib_h, int calib_w, float w2, mvsgi_stream_t stream);
int mvsgi_grid_equirect_f32(const float* points, float* grid, int B, long long M, mvsgi_stream_t stream);
/* rays [3][H][W] of the pixel centres of an H x W equirectangular surrogate view (align_corners=False): u = (2j+1)/W - 1,
 * v = (2i+1)/H - 1, lon = pi u, lat = pi v / 2, p = (cos lat cos lon, sin lat, -cos lat sin lon); mvsgi_grid_equirect_f32
 * of these rays returns (u, v). */
int mvsgi_rays_equirect_surrogate_f32(float* rays, int H, int W, mvsgi_stream_t stream);

/* ---- raw camera image -> surrogate view -------------------------------
 * The reference's sample_input=True step (api/inference_pytorch.py:61-74) for double-sphere cameras, DEFINED as the
 * composition of the reference's own closed forms (its image_sampler package is an empty submodule, so parity with that
 * package is unpinned): per output pixel
 *     out = valid ? bilinear_grid_sample(img, grid, align_corners=False) : invalid_value
 * (model/backports/backports.py:11-86: zero padding, weights from the unclamped coordinates, Ia*wa + Ib*wb + Ic*wc + Id*wd
 * left to right, no contraction).  The taps of an invalid pixel are not fetched; its grid may hold anything.
 *   grid  [T][H][W][2] fp32, grid_sample coordinates of the raw image (16-byte aligned when W % 4 == 0)
 *   valid [T][H][W]    uint8, non-zero = sample (4-byte aligned when W % 4 == 0)
 *   out   [M][C][H][W] fp32 planar (16-byte aligned when W % 4 == 0); every element is written
 * Image m uses table m % T (T cameras, M = frames x cameras; M % T == 0).
 * _u8_f32: imgs [M][Hr][Wr][3] uint8, each byte converted as RN(k / 255.0f) (inference_pytorch.py:58-59); C = 3.
 * _f32:    imgs [M][C][Hr][Wr] fp32, any C >= 1.
 * Limits: raw row bytes < 2^23 and (Hr + 2) rows within 2^31 bytes; H * W < 2^31; M < 2^31. */
int mvsgi_resample_bilinear_u8_f32(const unsigned char* imgs, const float* grid, const unsigned char* valid, float* out,
                                   long long M, int T, int Hr, int Wr, int H, int W, float invalid_value, mvsgi_stream_t stream);
int mvsgi_resample_bilinear_f32(const float* imgs, const float* grid, const unsigned char* valid, float* out, long long M, int T,
                                int C, int Hr, int Wr, int H, int W, float invalid_value, mvsgi_stream_t stream);
/* valid[i] = ds_mask[i] && |grid[i].x| <= 1 && |grid[i].y| <= 1 for n table entries (a NaN coordinate is invalid); once per rig */
int mvsgi_resample_validity_u8(const float* grid, const unsigned char* ds_mask, unsigned char* valid, long long n,
                               mvsgi_stream_t stream);
/* the uint8 conversion table of the resampler, RN(k / 255.0f) for k = 0..255, copied to 256 host floats */
int mvsgi_resample_u8_table_f32(float* table256);

/* ---- back-projection of the prediction (csrc/reproject.hip) ----------------------------------
 * SphericalSweepStereo._create_warped_inputs (dsta_mvs/model/mvs_model/spherical_sweep_stereo.py:417-471) for double-sphere
 * and equirectangular cameras: the rig camera's point cloud and the camera images warped into the rig camera's view, one
 * launch for all frames and cameras.  Per frame b, pixel (i, j) of the H x W map and camera n (fp32, no contraction):
 *     d = bf / inv[b][i][j]                 (:422, IEEE single division; bf = 96 for the regressor's raw output, 1 for a metric map)
 *     p = rays[:, i, j] * d                 (:435)  -> xyz
 *     q = T[n] p                            (the arithmetic of mvsgi_transform_points_f32)
 *     g, in_fov = projection of camera n    (mvsgi_grid_double_sphere_f32 or mvsgi_grid_equirect_f32 with in_fov = 1)
 *     valid = in_fov && |gx| <= 1 && |gy| <= 1           (mvsgi_resample_validity_u8; a NaN coordinate is invalid)
 *     warped = valid ? bilinear_grid_sample(img[b][n], g, align_corners=False) : invalid_value      (mvsgi_resample_bilinear_*)
 * The result is defined as the bits of that chain of entry points.  The taps of an invalid pixel are not fetched.
 *   device, in:   inv  [B][H][W] fp32;  rays [3][H][W] fp32, the rig camera's rays (mvsgi_rays_panorama_f32 with dist = [1], or
 *                 any other table);  imgs: img_kind 0 = uint8 [B*N][Hr][Wr][3] (each byte converted as RN(k / 255.0f)),
 *                 1 = fp32 [B*N][C][Hr][Wr]; NULL exactly when warped is NULL (img_kind, C, Hr, Wr are then ignored)
 *   device, out:  xyz [B][3][H][W], warped [B][N][C][H][W], grid [B][N][H][W][2] fp32, valid [B][N][H][W] uint8 (0 / 1); each may be
 *                 NULL (not computed), not all of them; 16-byte aligned.  inv and rays are 16-byte aligned when W % 4 == 0.
 *   host:         T [N][16] fp32: row-major 4 x 4 transforms taking rig-camera points into camera n's frame (the fp32 image of
 *                 the float64 inverse camera pose);  cams [N][10] fp32: model id (0 = double sphere, 1 = equirectangular), xi,
 *                 alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1 (the nine after the id are read for model 0 only; the last
 *                 two are whole numbers >= 1, as for the ints of mvsgi_grid_double_sphere_f32).
 *                 Both are copied into the kernel's arguments by the call: no device copy, nothing to keep alive.
 * 1 <= N <= mvsgi_sweep_max_cams().  Limits of the images as for mvsgi_resample_bilinear_*; H * W < 2^31, B < 2^31. */
int mvsgi_reproject_f32(const float* inv, const float* rays, const void* imgs, int img_kind, const float* T_host,
                        const float* cams_host, float* xyz, float* warped, unsigned char* valid, float* grid,
                        long long B, int N, int C, int Hr, int Wr, int H, int W, float bf, float invalid_value,
                        mvsgi_stream_t stream);

/* ---- deformable 2-D convolution with a given offset field ------------
 * SphereConvEquirect2d.forward + SphereConvBlk (common/common_modules.py:411-425, :509-547):
 *   y = act( deform_conv2d(x, offset, w, stride, padding, dilation) * scale + shift (+ res) )
 * with torchvision.ops.deform_conv2d's definition (offset channel 2*(i*Kw+j) = dy, +1 = dx of tap (i, j);
 * bilinear sampling, zero outside the image; no modulation mask).  Channels-last:
 *   x [N][H][W][Cin], offset [2*Kh*Kw][Ho][Wo] (shared) or [N][2*Kh*Kw][Ho][Wo] (offset_per_image),
 *   w_packed [Kh*Kw][Cin][Cout] from mvsgi_deform_conv2d_pack_weights_f32, y / res [N][Ho][Wo][Cout]. */
int mvsgi_deform_conv2d_pack_weights_f32(const float* w_oihw, float* w_packed, int Cout, int Cin, int Kh, int Kw,
                                         mvsgi_stream_t stream);
int mvsgi_deform_conv2d_f32(const float* x, const float* offset, int offset_per_image, const float* w_packed,
                            const float* scale, const float* shift, const float* res, float* y,
                            int N, int Cin, int H, int W, int Cout, int Kh, int Kw, int stride_h, int stride_w,
                            int pad_h, int pad_w, int dil_h, int dil_w, float neg_slope, mvsgi_stream_t stream);

/* mvsgi_sweep_std_nhwc_valid_f32 with the volume written split-padded (C == 16; see below), rig_batch in {1, B} */
int mvsgi_sweep_std_nhwc_valid_split(const float* feats, const float* grids, const unsigned char* vmask,
                                     void* vol_split, int B, int N, int C, int Hi, int Wi, int D, int Ho, int Wo,
                                     int rig_batch, mvsgi_stream_t stream);

/* ---- split-padded activations and the register-stationary conv (csrc/conv3d_rs.hip) ----------------------
 * Split-padded format of a channels-last activation tensor:  [B][D+2][H+2][W+2][C/16][4][8] bf16, where a voxel's
 * 16-channel slice is [hi(c 0-7) | hi(c 8-15) | lo(c 0-7) | lo(c 8-15)], x = hi + lo (hi = bf16(x), lo = bf16(x - hi));
 * the one-voxel border is zero (Conv3d's padding=1, common_modules.py:97-101) and is never written by any kernel:
 * allocate the buffer zero-filled once.  Same 4 bytes per element as fp32.
 *   mvsgi_act_split_bytes      size of such a buffer
 *   mvsgi_act_f32_to_split     fp32 [B][D][H][W][C] -> interior of a split-padded buffer
 *   mvsgi_act_split_to_f32     the inverse (hi + lo)
 *   mvsgi_conv3d_rs_split      BaseConvBlk3d.forward (common_modules.py:107-115) for Cin = Cout = 32, stride 1, on
 *                              split-padded x / res / y with the layer's weights resident in registers
 *                              (w_packed from mvsgi_conv3d_rs_pack_weights); same arithmetic as MVSGI_CONV_BF16X3;
 *                              neg_slope in [0, 1]; y_is_f32 != 0: y is a plain fp32 [B][D][H][W][32] tensor (the
 *                              hand-over to a kernel that reads fp32), otherwise split-padded
 */
int mvsgi_conv3d_f32_out_split(const float* x, const float* w_packed_b3, const float* scale, const float* shift,
                               const float* res, void* y_split, int B, int Cin, int Din, int Hin, int Win, int Cout,
                               int stride, float neg_slope, mvsgi_stream_t stream);   /* mvsgi_conv3d_f32 (MVSGI_CONV_BF16X3) writing a split-padded y */
/* post_vol (Cin = Cout = 16, stride 1, no residual) on a split-padded volume, fp32 [B][D][H][W][16] out; weights from
 * mvsgi_conv3d_rs_pack_weights(16, 16) */
int mvsgi_conv3d_rs16_split(const void* x_split, const void* w_packed_rs, const float* scale, const float* shift, float* y,
                            int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
/* the same layer writing a split-padded [B][D+2][H+2][W+2][16] tensor (zero-bordered by the caller, interior written): the
 * hand-over to mvsgi_conv3d_s2rs */
int mvsgi_conv3d_rs16_split_out_split(const void* x_split, const void* w_packed_rs, const float* scale, const float* shift,
                                      void* y_split, int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
/* UNetDownBlk.first of level 0 (unet_regulator.py:286-303: BaseConvBlk3d 16 -> 32, 3x3x3, stride 2, padding 1 + BN + LeakyReLU)
 * on split-padded activations (csrc/conv3d_s2rs.hip): x_split [B][D+2][H+2][W+2][64 B] -> y_split [B][Do+2][Ho+2][Wo+2][128 B],
 * Do = (D - 1) / 2 + 1 (likewise Ho, Wo), y = act(conv(x) * scale + shift); the scale is folded into w_packed by
 * mvsgi_conv3d_s2rs_pack_weights ([32][16][27] fp32 weights, scale[32]).  Staging by LDS-DMA: the layer is HBM-bound. */
size_t mvsgi_conv3d_s2rs_packed_weight_bytes(void);
int mvsgi_conv3d_s2rs_pack_weights(const float* w_oidhw, const float* scale, void* w_packed, mvsgi_stream_t stream);
int mvsgi_conv3d_s2rs(const void* x_split, const void* w_packed, const float* shift, void* y_split,
                      int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
size_t mvsgi_conv3d_rs_packed_weight_bytes(int Cout, int Cin);
int mvsgi_conv3d_rs_pack_weights(const float* w_oidhw, void* w_packed, int Cout, int Cin, mvsgi_stream_t stream);
size_t mvsgi_act_split_bytes(int B, int C, int D, int H, int W);
int mvsgi_act_f32_to_split(const float* x, void* y_split, int B, int C, int D, int H, int W, mvsgi_stream_t stream);
int mvsgi_act_split_to_f32(const void* x_split, float* y, int B, int C, int D, int H, int W, mvsgi_stream_t stream);
int mvsgi_conv3d_rs_split(const void* x_split, const void* w_packed_rs, const float* scale, const float* shift,
                          const void* res_split, void* y, int y_is_f32, int B, int Cin, int D, int H, int W, int Cout,
                          float neg_slope, mvsgi_stream_t stream);

/* ---- polyphase ResizeConv3d (csrc/conv3d_up2poly.hip) ------------------------------------------------------
 * ResizeConv3d.forward (dsta_mvs/model/common/common_modules.py:332-355) for Cin = 32, Cout = 16, no skip input --
 * out_costs.0 of the (16, 32) regulator (cost_volume_regulator/unet_regulator.py:52-60): trilinear x2 (align_corners=False,
 * :335-341) + Conv3d(k 3, padding 1) + eval BatchNorm + LeakyReLU evaluated as 8 phase convolutions over the LOW-resolution
 * tensor (weights folded at plan time; the faces of the volume, where ATen's clamp and the conv's zero padding change the
 * folded centre taps, by separate small launches).
 *   mvsgi_conv3d_up2_poly_plan_bytes   size of the plan for a low-resolution input of D x H x W voxels (0: bad dims)
 *   mvsgi_conv3d_up2_poly_plan         HOST function, no GPU call: w_oidhw_host [16][32][3][3][3] fp32 in host memory ->
 *                                      plan_host (position independent: copy the bytes to the device unchanged)
 *   mvsgi_conv3d_up2_poly_f32          x_split: split-padded [B][D+2][H+2][W+2][32]; y: fp32 [B][2D][2H][2W][16];
 *                                      scale / shift: 16 floats each; neg_slope in [0, 1]
 */
int mvsgi_conv3d_up2_f32_out_split(const float* x, const void* w_packed, int w_layout, const float* scale, const float* shift,
                                   const float* res, void* y_split, int B, int Cin, int Dl, int Hl, int Wl, int Cout,
                                   float neg_slope, mvsgi_stream_t stream);   /* mvsgi_conv3d_up2_f32 writing a split-padded y */
/* the polyphase layer with a split-padded result [B][2D+2][2H+2][2W+2][16], and the cost head (out_costs.1: Conv3d(Cin -> 1, k 3,
 * bias), unet_regulator.py:61-68) reading that format: hi | lo fragments straight into the matrix cores, split-bf16 arithmetic.
 * scale / shift of the head are passed by value (NoOp norm: 1 and the bias); neg_slope 1 = no activation. */
int mvsgi_conv3d_up2_poly_split(const void* x_split, const void* plan_dev, const float* scale, const float* shift, void* y_split,
                                int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
size_t mvsgi_conv3d_head_split_packed_weight_bytes(int Cin);
int mvsgi_conv3d_head_split_pack_weights(const float* w_oidhw, void* w_packed, int Cin, mvsgi_stream_t stream);
int mvsgi_conv3d_head_split(const void* x_split, const void* w_packed, float scale, float shift, float* y, int B, int Cin,
                            int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
/* the head in the fp16 split: x_split written by a kernel of the fp16 split (mvsgi_conv3d_up2_f32_out_split with w_layout |
 * MVSGI_CONV_F16); weights pre-scaled by a power of two by the caller, its inverse folded into `scale` */
int mvsgi_conv3d_head_split_pack_weights_f16(const float* w_oidhw, void* w_packed, int Cin, mvsgi_stream_t stream);
int mvsgi_conv3d_head_split_f16(const void* x_split, const void* w_packed, float scale, float shift, float* y, int B, int Cin,
                            int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
/* the hand-over between the two as FP32 RECORDS (fp16 split, Winograd-form main kernel: D == 8, H even, W a multiple of 32, an error
 * elsewhere): y_rec32 [B][2D+2][2H+2][2W+2][16 fp32], the same padded geometry (64 bytes per voxel, zero border never written),
 * the activated values neither clamped nor split; mvsgi_conv3d_head_rec32_f16 reads such records (Cin fp32 per voxel) and splits
 * every value it loads into the fp16 pair mvsgi_conv3d_head_split_f16 would have read (weights:
 * mvsgi_conv3d_head_split_pack_weights_f16).  Inside +-65504 the costs are bit for bit those of the pair of calls above. */
int mvsgi_conv3d_up2_poly_rec32(const void* x_split, const void* plan_dev, const float* scale, const float* shift, void* y_rec32,
                                int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
int mvsgi_conv3d_head_rec32_f16(const void* x_rec32, const void* w_packed, float scale, float shift, float* y, int B, int Cin,
                                int D, int H, int W, float neg_slope, mvsgi_stream_t stream);
size_t mvsgi_conv3d_up2_poly_plan_bytes(int D, int H, int W);
int mvsgi_conv3d_up2_poly_plan(const float* w_oidhw_host, void* plan_host, int D, int H, int W);
int mvsgi_conv3d_up2_poly_f32(const void* x_split, const void* plan_dev, const float* scale, const float* shift, float* y,
                              int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);

/* ---- the split-padded kernels in either 16-bit split (round 5) ---------------------------------------------------
 * The *_fmt forms of the entry points above: fmt = 0 runs the bf16 split (identical to the un-suffixed function), fmt =
 * MVSGI_SPLIT_F16 the fp16 split -- every split-padded tensor the call reads or writes, its packed weights and its residual then
 * hold fp16 pairs (x = hi + lo, 11 + 11 significant bits, values clamped to +-65504), and the products run on
 * v_mfma_f32_16x16x32_f16.  Weights of an fp16 call are pre-scaled by the caller with a power of two per output channel and its
 * inverse folded into `scale` (MVSGI_CONV_F16 above); mvsgi_conv3d_s2rs_fmt, whose epilogue has no per-channel multiplier, takes
 * one power of two for the layer (`unscale`, with `scale` at packing and `shift` multiplied by 1 / unscale).  Same reference ops
 * as the un-suffixed functions (BaseConvBlk3d / ResizeConv3d forward, common/common_modules.py:107-115, 332-355;
 * SphericalSweepStdMasked.sweep, cost_volume_builder/spherical_sweep_avg.py:38-136). */
int mvsgi_act_f32_to_split_fmt(const float* x, void* y_split, int B, int C, int D, int H, int W, int fmt, mvsgi_stream_t stream);
int mvsgi_act_split_to_f32_fmt(const void* x_split, float* y, int B, int C, int D, int H, int W, int fmt, mvsgi_stream_t stream);
int mvsgi_sweep_std_nhwc_valid_split_fmt(const float* feats, const float* grids, const unsigned char* vmask, void* vol_split,
                                         int B, int N, int C, int Hi, int Wi, int D, int Ho, int Wo, int rig_batch, int fmt,
                                         mvsgi_stream_t stream);
int mvsgi_conv3d_f32_out_split_fmt(const float* x, const float* w_packed_b3, const float* scale, const float* shift,
                                   const float* res, void* y_split, int B, int Cin, int Din, int Hin, int Win, int Cout,
                                   int stride, float neg_slope, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_rs_pack_weights_fmt(const float* w_oidhw, void* w_packed, int Cout, int Cin, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_rs_split_fmt(const void* x_split, const void* w_packed_rs, const float* scale, const float* shift,
                              const void* res_split, void* y, int y_is_f32, int B, int Cin, int D, int H, int W, int Cout,
                              float neg_slope, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_rs16_split_fmt(const void* x_split, const void* w_packed_rs, const float* scale, const float* shift, void* y,
                                int y_is_split, int B, int D, int H, int W, float neg_slope, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_s2rs_pack_weights_fmt(const float* w_oidhw, const float* scale, void* w_packed, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_s2rs_fmt(const void* x_split, const void* w_packed, const float* shift, void* y_split, int B, int D, int H, int W,
                          float neg_slope, float unscale, int fmt, mvsgi_stream_t stream);
/* y_f32p != 0 (MVSGI_SPLIT_F16 only): y is written "fp32-padded" (the padded geometry, plain fp32 records): see mvsgi_conv3d_wino32_f16 */
int mvsgi_conv3d_s2rs_out_fmt(const void* x_split, const void* w_packed, const float* shift, void* y_split, int B, int D, int H, int W,
                              float neg_slope, float unscale, int fmt, int y_f32p, mvsgi_stream_t stream);
int mvsgi_conv3d_up2_poly_plan_fmt(const float* w_oidhw_host, void* plan_host, int D, int H, int W, int fmt);
/* y_is_split: 0 = fp32 [B][2D][2H][2W][16]; 1 = split-padded [B][2D+2][2H+2][2W+2][16], main kernel by the dispatcher: with
 * MVSGI_SPLIT_F16, D == 8, H even, W a multiple of 32 and enough frames to fill the chip (mvsgi_conv3d_up2_poly_wino_pays) the
 * Winograd form (csrc/conv3d_wino_up2.hip: polyphase over (H, W) x Winograd F(2x2, 3x3) x an explicit upsample along D, 2.25 x fewer
 * matrix instructions; the same ResizeConv3d.forward, common_modules.py:332-355), else the direct register-stationary kernel;
 * 3 = split-padded, the direct kernel whatever the dispatcher would choose; 5 = split-padded, the Winograd form (rejected where it
 * does not apply) */
int mvsgi_conv3d_up2_poly_fmt(const void* x_split, const void* plan_dev, const float* scale, const float* shift, void* y,
                              int y_is_split, int B, int D, int H, int W, float neg_slope, int fmt, mvsgi_stream_t stream);
int mvsgi_conv3d_up2_poly_wino_pays(int B, int D, int H, int W);      /* 1: y_is_split = 1 in the fp16 split runs the Winograd form */

/* ---- Winograd F(2x2, 3x3) x direct-D form of the 32 -> 32 convolutions (csrc/conv3d_wino.hip) -------------------------
 * BaseConvBlk3d.forward (dsta_mvs/model/common/common_modules.py:107-115) for Cin = Cout = 32, stride 1, on split-padded
 * activations in the fp16 split (MVSGI_SPLIT_F16), D = 8 or 16, H even, W a multiple of 32: 2.25 x fewer matrix instructions than the direct
 * form.  Weights: U = G g G^T per (cout, cin, kd), pre-scaled per cout by a power of two (its inverse folded into `scale`),
 * split, as [a 4][b 4][kd 3][cout tile 2][hi | lo][64 lanes][16 B]. */
size_t mvsgi_conv3d_wino32_packed_weight_bytes(void);
int mvsgi_conv3d_wino32_applies(int Cin, int Cout, int D, int H, int W, int stride, float neg_slope);
/* w_oidhw [32][32][3][3][3] -> w_packed (mvsgi_conv3d_wino32_packed_weight_bytes()), unscale [32] (2^-k per cout: multiply the layer's scale by it) */
int mvsgi_conv3d_wino32_pack_weights(const float* w_oidhw, void* w_packed, float* unscale, mvsgi_stream_t stream);
/* y: split-padded fp16 [B][D+2][H+2][W+2][32] (y_is_f32 == 0) or plain fp32 [B][D][H][W][32]; res_split: split-padded fp16 or NULL.
 * act_f32p != 0: x, res and a padded y are "fp32-padded" instead -- the same padded geometry with plain fp32 records (32 floats per
 * voxel, zero border): the hand-over between Winograd layers, which split their operands behind the transform anyway. */
int mvsgi_conv3d_wino32_f16(const void* x_split, const void* w_packed, const float* scale, const float* shift, const void* res_split,
                            void* y, int y_is_f32, int act_f32p, int B, int D, int H, int W, float neg_slope, mvsgi_stream_t stream);

/* ---- instance norm (csrc/instnorm.hip) ------------------------------------------------------------------------------
 * nn.InstanceNorm3d / nn.InstanceNorm2d with input statistics (track_running_stats=False, train or eval: F.instance_norm's
 * use_input_stats) in a conv block, common/common_modules.py:107-115, applied after the conv:
 *   y[b][s][c] = act( (x[b][s][c] - mean[b][c]) / sqrt(var[b][c] + eps) * gamma[c] + beta[c] (+ res[b][s][c]) )
 * mean / var (biased) over the S spatial positions of frame b, channel c; act(v) = v > 0 ? v : v * neg_slope (0 = ReLU,
 * 1 = none).  x / res / y are channels-last [B][S][C] (NDHWC with S = D*H*W, or NHWC with S = H*W), 16-byte aligned;
 * res, gamma and beta may be NULL (no residual, gamma = 1, beta = 0); y may alias x (in place).  C % 4 == 0, C <= 1024, S >= 2.
 * Two launches (statistics partials into `ws`, then merge + apply); no atomics: frame b's result depends on frame b alone.
 * ws: caller-owned device scratch of mvsgi_instance_norm_ws_bytes(B, S, C) bytes (0 = invalid arguments). */
size_t mvsgi_instance_norm_ws_bytes(int B, int S, int C);
int mvsgi_instance_norm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y, float* ws,
                            int B, int S, int C, float eps, float neg_slope, mvsgi_stream_t stream);

/* ---- validation metrics (csrc/metrics.hip) ----------------------------------------------------------------------------
 * dsta_mvs/support/loss_function/metrics.py: RMSEMetric, MAEMetric, BadPixelRatioMetric and SSIMMetric, each also behind
 * InverseMetricWrapper, as validation_step (model/mvs_model/spherical_sweep_stereo_2024.py:145-231) applies them -- for every frame
 * of a batch and pooled, forward only, in at most four launches, without atomics: the same inputs give the same bits.
 * preds, target: [B][H][W] fp32, 16-byte aligned; preds is the regressor's raw output (not divided by bf).  Per pixel, in fp32
 * without contraction, p = preds[b][i][j], t = target[b][i][j]:
 *   direct form     P = p / bf, T = clamp(t, cmin, cmax) / bf                  (MVSMetric.clamp_and_scale, :27-37; torch.clamp: a
 *                   NaN stays a NaN); cmin / cmax = min / max(bf / Tensor(dist_list)) as fp32, computed by the caller (:23-25)
 *   distance form   the same on p' = 1.0f / p, t' = 1.0f / t                   (InverseMetricWrapper, :160-183, literally: the
 *                   clamp to the inverse-distance range is applied to 1 / t)
 *   validity v      mask_kind MVSGI_METRICS_MASK_NONE: every pixel; _TENSOR: mask[b][i][j] != 0 (bytes; 4-byte aligned); _RANGE:
 *                   lo <= t <= hi on the raw t for both forms (validation_step's mask_labels, :198-199).  A select: a NaN
 *                   at an invalid pixel changes nothing.
 *   e = P - T, a = |e|, s = e * e; over the valid pixels of a frame S2 = sum s, S1 = sum a (float64, compensated: the sums
 *   of the fp32 addends to ~2^-100 relative, rounded once), n = count, NB = #{a > thresh} (thresh for the direct form, thresh_dist for the other)
 *   rmse = sqrt(S2 / n), mae = S1 / n (n = 0: NaN), bad = n > 0 ? NB / n : 1.0; with MVSGI_METRICS_MASK_NONE bad = NB / (H * W)
 *   (:145-156, literally)
 *   ssim            in float64, the mask is not used (:59-60): R = max(maxP - minP, maxT - minT) over the frame
 *                   (MVSGI_METRICS_RANGE_FRAME) or the launch (MVSGI_METRICS_RANGE_BATCH: what one call of the reference on B frames
 *                   uses), c1 = (0.01 R)^2, c2 = (0.03 R)^2, g_u = exp(-(u / 1.5)^2 / 2), u = -5 .. 5, normalised to sum 1;
 *                   at every pixel whose 11 x 11 window lies inside the image mu_X = sum_uv g_u g_v X[i + u][j + v] for X in
 *                   {P, T, PP, TT, PT}; map = (2 mu_P mu_T + c1)(2 s_PT + c2) / ((mu_P^2 + mu_T^2 + c1)(s_P + s_T + c2)) with
 *                   s_P = mu_PP - mu_P^2, s_T = mu_TT - mu_T^2, s_PT = mu_PT - mu_P mu_T; ssim = the mean of the map over those
 *                   (H - 10)(W - 10) pixels (structural_similarity_index_measure with its defaults, whose reflect padding is cropped
 *                   off again before the mean); H < 11 or W < 11: NaN
 * out: [B + 1][9] float64, columns rmse, mae, bad, ssim, rmse_dist, mae_dist, bad_dist, ssim_dist, n.  Row B is the reference's
 * value for the batch as one call: sums and counts added over the frames (unmasked bad over H * W, as the reference divides),
 * ssim the mean of the frames' means.  Row b < B depends on frame b alone in MVSGI_METRICS_RANGE_FRAME.
 * ws: caller-owned device scratch of ws_bytes >= mvsgi_metrics_ws_bytes(B, H, W) bytes (0 = invalid dimensions), 8-byte aligned;
 * B < 65535. */
#define MVSGI_METRICS_MASK_NONE   0
#define MVSGI_METRICS_MASK_TENSOR 1
#define MVSGI_METRICS_MASK_RANGE  2
#define MVSGI_METRICS_RANGE_FRAME 0
#define MVSGI_METRICS_RANGE_BATCH 1
size_t mvsgi_metrics_ws_bytes(int B, int H, int W);
int mvsgi_metrics_f32(const float* preds, const float* target, const unsigned char* mask, int mask_kind, float lo, float hi,
                      float bf, float cmin, float cmax, float thresh, float thresh_dist, int range_scope, void* ws,
                      size_t ws_bytes, double* out, int B, int H, int W, mvsgi_stream_t stream);

/* ---- loss functions (csrc/losses.hip) -------------------------------------------------------------------------------------
 * dsta_mvs/support/loss_function/distance_loss.py: the forward values of VolumeCrossEntropy (:21-48), MaskedSmoothL1Loss (:59-70, the
 * shape[1] == 1 branch) and InBoundsBCEDistanceLoss (:86-105, likewise) for every frame of a batch and pooled, in one reduce and one
 * finalise launch, without atomics: the same inputs give the same bits.  No gradients.  fp32 without contraction per element; the
 * sums are float64, compensated (the sum of the fp32 addends to ~2^-100 relative, rounded once), the means float64.
 * labels [B][OH][OW] fp32: the true inverse distance L.  inv_list [D] fp32, D >= 2 (read for vol and true_cost only): list = bf / dist_list as the caller's fp32
 * division gives it, strictly decreasing (dist_list strictly increasing and positive; the caller checks, a zero bin width has no meaning).
 *   vol        x = clamp(L, list[D-1], list[0]) (torch.clamp: a NaN stays);  bin = clamp(D - #{d: list[d] < x} - 1, 0, D - 2)
 *              (len(list) - torch.bucketize(x, flipped list) - 1);  d = (x - list[bin]) / (list[bin+1] - list[bin]);
 *              t[bin] = 1 - d, t[bin+1] = d, t = 0 elsewhere;  per selected element (b, c, i, j) the addend
 *              (t - 1) * max(log1pf(-p), -100) - t * max(logf(p), -100)  (ATen's binary_cross_entropy);  vol = sum / n_vol (n_vol = 0: NaN).
 *              p_kind MVSGI_LOSSES_P_GIVEN: p = probs[b][c][i][j], probs [B][D][OH][OW] (the regressor's norm_costs, or any probabilities);
 *              MVSGI_LOSSES_P_FUSED: probs is the low-resolution cost volume [B][D][H][W] and p the soft-argmin's softmax at the
 *              output pixel, as mvsgi_confidence_f32 defines it: v_c the blend of mvsgi_softargmin_scaled_f32 (same coordinate rule,
 *              OH = floor(H * scale), OW = floor(W * scale), zero-weight-tap rule), m = max_c v_c, e_c = expf(-(m - v_c)), S = sum e_c in
 *              order of c, p_c = e_c / S; no [B][D][OH][OW] tensor is read or written.  MVSGI_LOSSES_P_NONE: no volume loss
 *              (columns vol and n_vol NaN); H, W and scale are read in the fused kind only.
 *              Selection: vol_kind MVSGI_LOSSES_VOL_NONE every element; _PIXEL vol_mask [B][OH][OW] bytes, a pixel counts D times;
 *              _VOLUME vol_mask [B][D][OH][OW] bytes.  A select: an unselected element never reaches the sum.
 *   true_cost  optional output [B][D][OH][OW] fp32: t for every element, selected or not; null: not written.
 *   smooth_l1  pred [B][OH][OW] fp32 (null: columns smooth_l1 and inbounds NaN): z = |pred - L|, addend z < 1 ? 0.5 * z * z : z - 0.5
 *              over the selected pixels, / n_px.  Selection: px_kind MVSGI_LOSSES_PX_NONE every pixel; _TENSOR px_mask [B][OH][OW]
 *              bytes; _LABEL_MAX L <= label_max (the training step masks labels above 191).
 *   inbounds   (inbounds != 0, else NaN) in(v) = v < near_inv && v > far_inv on the raw pred and L, near_inv = fl32(1 / near_dist_threshold),
 *              far_inv = fl32(1 / far_dist_threshold); BCELoss on {0, 1} values with its -100 clamp is 100 * #{in(pred) != in(L)} / n_px
 *              over the selected pixels.
 * out: [B + 1][5] float64, columns vol, smooth_l1, inbounds, n_vol, n_px.  Row b < B depends on frame b alone; row B: sums and
 * counts added over the frames in frame order (what one call of the reference's class on the batch computes).
 * ws: caller-owned device scratch of ws_bytes >= mvsgi_losses_ws_bytes(B, OH, OW) bytes (0 = invalid dimensions), 8-byte aligned;
 * B < 65535.  With ws and out supplied nothing is allocated and the call can be captured into a hipGraph. */
#define MVSGI_LOSSES_P_NONE       0
#define MVSGI_LOSSES_P_GIVEN      1
#define MVSGI_LOSSES_P_FUSED      2
#define MVSGI_LOSSES_VOL_NONE     0
#define MVSGI_LOSSES_VOL_PIXEL    1
#define MVSGI_LOSSES_VOL_VOLUME   2
#define MVSGI_LOSSES_PX_NONE      0
#define MVSGI_LOSSES_PX_TENSOR    1
#define MVSGI_LOSSES_PX_LABEL_MAX 2
size_t mvsgi_losses_ws_bytes(int B, int OH, int OW);
int mvsgi_losses_f32(const float* labels, const float* pred, const float* probs, int p_kind, const float* inv_list,
                     const unsigned char* vol_mask, int vol_kind, const unsigned char* px_mask, int px_kind, float label_max,
                     int inbounds, float near_inv, float far_inv, float* true_cost, void* ws, size_t ws_bytes, double* out,
                     int B, int D, int H, int W, double scale, int OH, int OW, mvsgi_stream_t stream);

/* ---- packed point cloud (csrc/cloud.hip) --------------------------------------------------------------------------------
 * The last stage behind the back-projection and the confidence maps: the prediction as a packed list of points, filtered and
 * compacted on the device.  Not part of the reference's interface; defined as a composition of operations this library already
 * has.  Per frame b, pixel (i, j) of the H x W map, linear index p = i * W + j (fp32, no contraction):
 *     d = bf / inv[b][i][j]                 the IEEE single division of mvsgi_reproject_f32
 *     xyz = rays[:, i, j] * d               the bits mvsgi_reproject_f32 writes to xyz[b][:, i, j]
 * keep(b, p) holds iff all of (a comparison with a NaN is false)
 *     1. i % sy == 0 && j % sx == 0
 *     2. mask != 0                          when a mask is given: uint8 [H][W] (mask_per_frame = 0) or [B][H][W] (1)
 *     3. d is finite && d_min <= d <= d_max (d_min > 0 drops inv = 0, negative, +-inf and NaN)
 *     4. lo[k] <= gate_k[b][i][j] <= hi[k]  for each of the n_gates <= 4 gate planes [B][H][W] fp32
 *     5. some camera n has valid[b][n][i][j] != 0          when require_colour
 * colour of a kept point: warped[b][n*][0 .. C-1][i][j], n* the lowest camera index with valid set; when no camera is valid every
 * channel is no_colour.  warped [B][N][C][H][W] fp32 and valid [B][N][H][W] uint8 as mvsgi_reproject_f32 writes them, both or
 * neither (NULL; N and C are then ignored and C counts as 0), 1 <= N <= mvsgi_sweep_max_cams(), 1 <= C <= 4.
 * attributes: A planes [B][H][W] fp32.  Record width R = 3 + C + A <= 16.
 *   device, out:  points [B][capacity][R] fp32, records [x, y, z, c_0 .., a_0 ..]; the kept points of frame b in ascending p;
 *                 counts [B][2] int32 = (written, kept), written = min(kept, capacity);
 *                 index [B][capacity] int32, the source p of each record, or NULL.
 *                 Rows >= written of points and index are not written; nothing but the outputs and ws is written.
 *   host:         gates [n_gates] and attrs [A]: tables of DEVICE pointers; gate_lo / gate_hi [n_gates] fp32.  They are read by the
 *                 call and travel in the kernels' arguments: no device copy, nothing to keep alive (as T_host of mvsgi_reproject_f32).
 *   ws:           caller-owned device scratch of ws_bytes >= mvsgi_cloud_ws_bytes(B, H, W) bytes (0 = invalid dimensions), 16-byte
 *                 aligned: one bit per pixel in 64-bit words (tiles of 1024 consecutive p, 16 words each), and per tile its number
 *                 of kept pixels and its offset in the frame's list.
 * Three launches (flags and tile counts; one exclusive scan per frame; scatter), no atomics, no waiting between workgroups, no host
 * synchronisation: the same inputs give the same bits.  The predicate is evaluated once; the scatter reads its bits.  Every device
 * pointer needs its element's alignment only (ws: 16 bytes).  H * W < 2^31, 1 <= B <= 65535, 1 <= capacity < 2^31, sy, sx >= 1. */
size_t mvsgi_cloud_ws_bytes(long long B, int H, int W);
int mvsgi_cloud_pack_f32(const float* inv, const float* rays, const unsigned char* mask, int mask_per_frame,
                         const float* const* gates_host, const float* gate_lo_host, const float* gate_hi_host, int n_gates,
                         const float* warped, const unsigned char* valid, int N, int C, int require_colour, float no_colour,
                         const float* const* attrs_host, int A, float* points, int* counts, int* index, long long capacity,
                         void* ws, size_t ws_bytes, long long B, int H, int W, int sy, int sx, float bf, float d_min, float d_max,
                         mvsgi_stream_t stream);

/* ---- photometric consistency of the prediction (csrc/photo.hip) ----------------------------------------------------------------
 * Do the cameras agree on the colour of the point a pixel's predicted distance puts in front of them?  The cost volume's own fusion
 * rule (SphericalSweepStdMasked, dsta_mvs/model/cost_volume_builder/spherical_sweep_avg.py:92-125: the masked variance over the
 * cameras that see a point), evaluated on the camera images at the predicted inverse distance.  Not part of the reference's
 * interface; defined as a composition of operations this library already has.  For frame b and pixel (i, j) of the H x W map, steps
 * 1-6 of mvsgi_reproject_f32 give valid_n and w_n[c] = warped[b][n][c][i][j] (invalid_value 0) for each camera n < N: the same
 * functions, so the same bits; warped is never stored, and the taps of an invalid camera are not fetched.  Then in fp32, no
 * contraction, each operation one IEEE operation, every sum over cameras or channels started at +0 and taken left to right from
 * index 0:
 *     1. seen_n = valid_n; with cam_masks (fp32 [N][1][Hr][Wr], the tensor sample_masks takes, the size of the images) additionally
 *        && (the mask of camera n sampled at the same grid by the same bilinear arithmetic) > 0      (:92-102, the 4-tap rule)
 *     2. cnt = sum_n float(seen_n);  ok = cnt > 1;  k = ok ? cnt : 1                                 (:106-111)
 *     3. avg_c = (sum_n w_n[c] * float(seen_n)) / k                                                  (:114)
 *     4. x_n = seen_n ? w_n[c] : avg_c;  var_c = ok ? (sum_n (x_n - avg_c) * (x_n - avg_c)) / k : 0  (:119-125)
 *     5. photo_var = (sum_c var_c) / float(C)
 *     6. photo_std = sqrt(photo_var)
 *     7. a pixel is scored when ok && mask != 0 (mask: uint8 [H][W] with mask_per_frame = 0, [B][H][W] with 1, NULL: every pixel)
 * Values of inv nobody should pass do what the chain does with them, there is no special case: 0 and NaN give coordinates no camera
 * accepts (cnt = 0, photo_var = 0, not scored); a negative value or inf is a finite point behind the rig camera or at its centre,
 * which another camera may see.  Occlusion is not reasoned about: a point hidden from one camera reads high.
 *   device, out:  n_views [B][H][W] uint8 = cnt;  photo_var, photo_std [B][H][W] fp32;  mean_colour [B][C][H][W] fp32 = avg_c (0
 *                 where cnt = 0); each may be NULL (not written); 16-byte aligned.
 *                 table [B + 1][14] float64, or NULL: columns n (scored pixels), mean_std = sum std / n, rms = sqrt(sum var / n),
 *                 bad = #{std > thresh} / n, coverage = n / #{mask != 0}, views_0 .. views_8 = the masked pixels with exactly k
 *                 seen cameras; mean_std, rms and bad are NaN where n = 0.  The sums are float64, compensated (the sum of the
 *                 fp32 addends to ~2^-100 relative, rounded once).  Row b < B depends on frame b alone; row B: sums and counts
 *                 added over the frames in frame order.
 *   device, in:   inv, rays, imgs (img_kind, C, Hr, Wr) as for mvsgi_reproject_f32, imgs required; inv and rays 16-byte and mask
 *                 4-byte aligned when W % 4 == 0.
 *   host:         T [N][16], cams [N][10] as for mvsgi_reproject_f32 (copied into the kernel's arguments by the call).
 *   ws:           caller-owned device scratch of ws_bytes >= mvsgi_photo_ws_bytes(B, H, W) bytes (0 = invalid dimensions), 8-byte
 *                 aligned; read with a table only (ws may be NULL without one, and the second launch is then skipped).
 * Two launches (reduce, grid (G, B) with G a function of (H, W) alone; finalise), no atomics, no host synchronisation, no
 * allocation: capturable, and the same inputs give the same bits.  1 <= N <= mvsgi_sweep_max_cams(); H * W < 2^31 - 2^18, B < 65535;
 * limits of the images as for mvsgi_resample_bilinear_*. */
size_t mvsgi_photo_ws_bytes(long long B, int H, int W);
int mvsgi_photo_consistency_f32(const float* inv, const float* rays, const void* imgs, int img_kind, const float* cam_masks,
                                const float* T_host, const float* cams_host, const unsigned char* mask, int mask_per_frame,
                                float thresh, unsigned char* n_views, float* photo_var, float* photo_std, float* mean_colour,
                                void* ws, size_t ws_bytes, double* table, long long B, int N, int C, int Hr, int Wr, int H, int W,
                                float bf, mvsgi_stream_t stream);
/* The same with one more input: cam_seen [B][N][H][W] bytes, or NULL.  Step 1 becomes seen_n = valid_n && (the camera-mask rule) &&
 * cam_seen[b][n][i][j] != 0: what mvsgi_visibility_f32 writes to `visible` makes the fusion rule skip the cameras a nearer surface hides
 * the point from.  4-byte aligned when W % 4 == 0.  With NULL this is mvsgi_photo_consistency_f32 (the same kernels, the same bits), and
 * so is an all-ones plane in its values. */
int mvsgi_photo_consistency_seen_f32(const float* inv, const float* rays, const void* imgs, int img_kind, const float* cam_masks,
                                     const float* T_host, const float* cams_host, const unsigned char* mask, int mask_per_frame,
                                     float thresh, unsigned char* n_views, float* photo_var, float* photo_std, float* mean_colour,
                                     void* ws, size_t ws_bytes, double* table, long long B, int N, int C, int Hr, int Wr, int H, int W,
                                     float bf, const unsigned char* cam_seen, mvsgi_stream_t stream);

/* ---- camera range images and visibility (csrc/visibility.hip) ---------------------------------------------------------------------
 * The predicted surface forward-rendered into each camera, the nearest point kept per cell of the camera's own Hz x Wz buffer (a
 * z-buffer), and per pixel and camera whether the pixel's own point is the one the camera sees there.  Not part of the reference's
 * interface; defined as a composition of operations this library already has.  All arithmetic is fp32, no contraction, one IEEE
 * operation per written operation.  For frame b, pixel (i, j) of the H x W map and camera n < N <= mvsgi_sweep_max_cams():
 *     1. steps 1-5 of mvsgi_reproject_f32 (the same functions, so the same bits): v = inv[b][i][j], d = bf / v, p = rays[:, i, j] * d,
 *        q = T_n p, (g, in_fov) the camera's projection of q, valid_n = in_fov && |gx| <= 1 && |gy| <= 1
 *     2. live = 0 < v <= FLT_MAX && d <= FLT_MAX   (a NaN, zero, negative or infinite v is not live, nor a v so small that d
 *        overflows; v = +inf would give d = 0, the rig camera's own centre)
 *     3. r2 = (qx * qx + qy * qy) + qz * qz    the squared range from camera n; no square root
 *     4. cell: cx = clamp(int(floorf(((gx + 1) * float(Wz)) * 0.5f)), 0, Wz - 1), cy likewise with gy and Hz
 *     5. splat, iff live && valid_n && mask != 0 (mask: uint8 [H][W] with mask_per_frame = 0, [B][H][W] with 1, NULL: every pixel):
 *        z2[b][n][cy][cx] = min(z2[b][n][cy][cx], r2), the buffer starting at +inf.  With footprint = 2 instead into the four cells
 *        (clamp(x0 + dx, 0, Wz - 1), clamp(y0 + dy, 0, Hz - 1)), dx, dy in {0, 1}, x0 = floorf(((gx + 1) * float(Wz) - 1) * 0.5f), y0
 *        likewise (cells that coincide after the clamp are harmless).  Longitude does not wrap: the footprint clamps at the edge.
 *     6. test, in a later launch and always at the cell of step 4: visible_n = live && valid_n && r2 <= z2[b][n][cy][cx] * k2, with
 *        k2 = fp32((1 + tol)^2) rounded once from double by the caller.  A pixel the mask excluded is not splatted but is tested.
 *     7. n_visible = sum_n visible_n
 *     8. range = sqrtf(z2) (+inf in an empty cell)
 * When a point is splatted r2 is >= +0 and not a NaN (a NaN q is not valid), so its bit pattern orders like an unsigned integer and
 * +inf is the fill value: the minimum is an atomic minimum on the unsigned pattern, independent of the order of arrival.  The same
 * inputs give the same bits in every run, and a captured launch replays the eager bits.  A cell holds the minimum over everything that
 * lands in it, so a slanted surface reads nearer than its own points: tol is the caller's answer.  An empty cell
 * occludes nothing.
 *   device:  inv, rays as for mvsgi_reproject_f32 (16-byte aligned when W % 4 == 0); mask 4-byte aligned when W % 4 == 0;
 *            z2 [B][N][Hz][Wz] fp32, 16-byte aligned: written by mvsgi_camera_range_f32 (every cell), read by mvsgi_visibility_f32;
 *            visible [B][N][H][W] uint8 (0 / 1), n_visible [B][H][W] uint8, range [B][N][Hz][Wz] fp32: each may be NULL (not all), 16-byte
 *            aligned.
 *   host:    T [N][16], cams [N][10] as for mvsgi_reproject_f32 (copied into the kernels' arguments by the call).
 * mvsgi_camera_range_f32: two launches (fill, splat); mvsgi_visibility_f32: one launch for visible / n_visible and one for range.  No
 * host synchronisation, no allocation: capturable.  H * W < 2^31, Hz * Wz < 2^31, Hz, Wz <= 2^24, 1 <= k2 < inf, footprint 1 or 2. */
int mvsgi_camera_range_f32(const float* inv, const float* rays, const float* T_host, const float* cams_host, const unsigned char* mask,
                           int mask_per_frame, int footprint, float* z2, long long B, int N, int H, int W, int Hz, int Wz, float bf,
                           mvsgi_stream_t stream);
int mvsgi_visibility_f32(const float* inv, const float* rays, const float* T_host, const float* cams_host, const float* z2, float k2,
                         unsigned char* visible, unsigned char* n_visible, float* range, long long B, int N, int H, int W, int Hz,
                         int Wz, float bf, mvsgi_stream_t stream);

/* ---- temporal fusion (csrc/temporal.hip) ------------------------------------------------------------------------------------------
 * The previous fused prediction of a sequence, warped to the rig's new pose and fused with the new measurement: a z-buffer that carries
 * its source pixel, then a per-pixel gated Kalman update.  Not part of the reference's interface; defined as a composition of
 * operations this library already has.  All arithmetic is fp32, no contraction, one IEEE operation per written operation; the steps
 * shared with mvsgi_reproject_f32 and mvsgi_camera_range_f32 are the same functions, so the same bits.  B independent sequences, one
 * step per call; frame b, H x W maps of the rig camera (an equirectangular panorama, rays as mvsgi_rays_panorama_f32 makes them).
 * Stage A, splat (mvsgi_temporal_splat_f32), source pixel (i, j), s = i * W + j:
 *     1. v = prev_inv[b][i][j], d = bf / v, p = rays[:, i, j] * d                      (steps 1, 2 of mvsgi_reproject_f32)
 *     2. live = prev_age[b][i][j] != 0 && 0 < v <= FLT_MAX && d <= FLT_MAX             (mvsgi_camera_range_f32's rule and the age)
 *     3. q = T_b p (rows 0..2 of T[b], the row rule of mvsgi_transform_points_f32); r2 = (qx * qx + qy * qy) + qz * qz; the point is
 *        rejected unless 0 < r2 <= FLT_MAX (a NaN compares false)
 *     4. (gx, gy) = the equirectangular projection of q (mvsgi_grid_equirect_f32); u = gx * au + bu, w = gy * av + bv, each a multiply
 *        then an add; cx = int(floorf(u)), cy = int(floorf(w)); with wrap != 0: cx += W when cx < 0, cx -= W when cx >= W, once each;
 *        rejected unless 0 <= cx < W && 0 <= cy < H (decided on the floats, so a NaN or a value no int holds is rejected too).
 *        au = pi * W / (long1 - long0), bu = -long0 * W / (long1 - long0), av = (pi / 2) * H / (lat1 - lat0),
 *        bv = (pi / 2 - lat0) * H / (lat1 - lat0) of the rig camera's ranges, float64 on the host, rounded once: the inverse of the
 *        panorama's ray table (lon = theta, lat = phi - pi / 2), so at T = identity a live pixel lands in its own cell.
 *     5. key = (uint64(bits(r2)) << 32) | uint32(s);  zkey[b][cy][cx] = min(zkey[b][cy][cx], key), the buffer starting at
 *        EMPTY = 0x7F800000FFFFFFFF (+inf over the largest index).  The nearest source wins a cell, on equal r2 the lower index.  r2 is
 *        positive and finite, so its pattern orders like an unsigned integer, and an integer minimum does not depend on the order of
 *        arrival: every run and every captured replay give the same bits.
 * Stage B, resolve and fuse (mvsgi_temporal_fuse_f32), target pixel t:
 *     1. key = zkey[b][t]; r2 = float(bits(key >> 32)); s = min(key & 0xffffffff, H * W - 1) (< H * W by construction, clamped all the same)
 *     2. warped_inv = bf / sqrtf(r2); ratio = warped_inv / prev_inv[b][s]; g = ratio * ratio; var_w = prev_var[b][s] * (g * g) + q_var
 *        (along the ray d inv' / d inv = (inv' / inv)^2; the cosine between the old and the new ray is dropped: an approximation)
 *     3. prior = key != EMPTY && 0 <= var_w <= FLT_MAX
 *     4. m = cur_inv[b][t]; sd = cur_std ? cur_std[b][t] : meas_std; var_m = sd * sd
 *     5. meas = 0 < m <= FLT_MAX && 0 < var_m <= FLT_MAX
 *     6. neither:            fused = m (as it is), var = +inf, age = 0
 *        prior only:         fused = warped_inv, var = var_w, age = prev_age[b][s]           (not confirmed: not incremented)
 *        meas only:          fused = m, var = var_m, age = 1
 *        both: e = m - warped_inv, S = var_w + var_m; they agree iff e * e <= gate2 * S, then K = var_w / S,
 *                            fused = warped_inv + K * e, var = var_w - K * var_w, age = min(prev_age[b][s] + 1, 255)
 *        both, disagreeing:  fused = m, var = var_m, age = 1                                 (the measurement restarts the pixel)
 *     7. optional: warped_inv (0 in an empty cell), warped_var = var_w (+inf in an empty cell), src = s as int32 (-1 in an empty cell;
 *        a source index above 2^31 - 1 reads negative)
 *   device:  prev_inv, prev_var, cur_inv, cur_std [B][H][W] fp32; prev_age, age [B][H][W] uint8; rays [3][H][W]; T [B][16] fp32 row-major
 *            4 x 4, READ FROM DEVICE MEMORY by the splat (it changes every step; a captured launch sees the value of the replay);
 *            zkey [B][H][W] uint64; fused, var, warped_inv, warped_var fp32, src int32 [B][H][W].  Everything 16-byte aligned.  The
 *            outputs of the fuse may each be NULL (not all); none may alias prev_* (stage B gathers the state at s).
 *   host:    bf; au, bu, av, bv, wrap as above; gate2 = fp32(gate^2) > 0, q_var >= 0, meas_std > 0 (read when cur_std is NULL).
 * mvsgi_temporal_splat_f32: two launches (fill, splat); mvsgi_temporal_fuse_f32: one.  No host synchronisation, no allocation:
 * capturable.  H * W < 2^32 and B * ceil(H * ceil(W / 4) / 256) < 2^31. */
int mvsgi_temporal_splat_f32(const float* prev_inv, const unsigned char* prev_age, const float* rays, const float* T,
                             unsigned long long* zkey, long long B, int H, int W, float bf, float au, float bu, float av, float bv,
                             int wrap, mvsgi_stream_t stream);
int mvsgi_temporal_fuse_f32(const unsigned long long* zkey, const float* prev_inv, const float* prev_var,
                            const unsigned char* prev_age, const float* cur_inv, const float* cur_std, float meas_std, float* fused,
                            float* var, unsigned char* age, float* warped_inv, float* warped_var, int* src, long long B, int H, int W,
                            float bf, float gate2, float q_var, mvsgi_stream_t stream);

/* ---- volumetric fusion (csrc/tsdf.hip) --------------------------------------------------------------------------------------------
 * The predictions of a sequence integrated into a world-fixed truncated signed distance volume that rolls with the rig, and that
 * volume ray-cast back into the rig's view.  Not part of the reference's interface; defined as a composition of operations this
 * library already has.  All arithmetic is fp32, no contraction, one IEEE operation per written operation; the row of a transform,
 * the equirectangular projection and the affine map into the panorama's cells are the functions mvsgi_temporal_splat_f32 uses.
 * State, per sequence b: vol [Nz][Ny][Nx][2] fp32, the pair (f, w) of a voxel: the truncated signed distance in units of trunc
 * (positive in front of the surface) and the accumulated weight.  The store is TOROIDAL: the voxel with world index i = (ix, iy, iz)
 * (integers of any sign; its centre is (i + 0.5) * vs) lives in slot i mod N per axis, the floored modulus; the volume covers
 * origin[b][a] <= i_a < origin[b][a] + N_a.  origin, origin_prev [B][3] int32 and the poses are DEVICE pointers, read by the
 * launches: a captured step follows a moving rig.  |i_a| < 2^23 is the caller's to keep (the origin is device data and not checked;
 * whatever it holds, no address outside the buffers is formed).
 * mvsgi_tsdf_integrate_f32, one launch, in place; slot s = (sx, sy, sz) of sequence b:
 *     1. i_a = origin_a + ((s_a - origin_a) mod N_a); fresh = some axis has i_a < origin_prev_a or i_a >= origin_prev_a + N_a (the
 *        slot scrolled in since the previous integrate: re-centring costs no pass of its own); (f, w) = fresh ? (1, 0) : vol[b][s]
 *     2. c_a = (float(i_a) + 0.5f) * vs; q = T_b c (T: world -> rig, rows 0..2, the row rule of mvsgi_transform_points_f32);
 *        r2 = (qx * qx + qy * qy) + qz * qz, rejected unless 0 < r2 <= FLT_MAX; r = sqrtf(r2), rejected unless r_min <= r <= r_max
 *     3. (gx, gy) = the equirectangular projection of q; u = gx * au + bu, v = gy * av + bv; floorf, the column wrapped once when
 *        wrap != 0; rejected outside the map, decided on the floats (step 4 of mvsgi_temporal_splat_f32: the same cell (cx, cy))
 *     4. m = inv[b][cy][cx]; rejected where mask is given and mask[b][cy][cx] == 0; d = bf / m; rejected unless
 *        0 < m <= FLT_MAX && d <= FLT_MAX
 *     5. sdf = d - r; rejected if sdf < -trunc (behind the surface: not observed); obs = fminf(sdf, trunc) / trunc
 *     6. w_obs = 1 without std; with std: sd = std[b][cy][cx] (in inv's unit), sig = sd * d / m (the standard deviation of the
 *        distance), w_obs = t2 / (t2 + sig * sig), t2 = fp32(trunc^2); rejected unless 0 < w_obs <= 1 (a NaN compares false)
 *     7. W = w + w_obs; f' = (f * w + obs * w_obs) / W; w' = fminf(W, w_max)
 *     8. vol[b][s] = (f', w'); a rejected voxel keeps the (f, w) of step 1, so a fresh rejected one is stored as (1, 0)
 *        optional: range[b][s] = r (0 where r2 was rejected), for the tests that bound the root
 *   host: vs > 0, trunc > 0, t2, w_max > 0, 0 <= r_min < r_max <= FLT_MAX, the affine map finite, wrap 0 / 1, every N_a >= 1,
 *         Nx * Ny * Nz < 2^31 (offsets are 64-bit), H * W < 2^31, B * ceil(Nx * Ny * Nz / 512) < 2^31; 16-byte alignment.
 * mvsgi_tsdf_raycast_f32, one launch; pixel (i, j) of sequence b, P_b the rig -> world pose:
 *     1. dir_a = fma(P[a][2], rz, fma(P[a][1], ry, P[a][0] * rx)) of rays[:, i, j] (the row rule without the translation);
 *        o_a = P[a][3]
 *     2. for k = 0 .. K - 1: t_k = t0 + float(k) * step; p_a = o_a + dir_a * t_k; g_a = floorf(p_a * inv_vs) (inv_vs = fp32(1 / vs),
 *        rounded once on the host); inside = every axis has origin_a <= g_a < origin_a + N_a, decided on the floats; (f_k, w_k) =
 *        the pair of slot g mod N; valid_k = inside && w_k >= w_min
 *     3. the first k >= 1 with valid_k && valid_{k-1} && f_{k-1} > 0 && f_k <= 0 ends the march: t* = t_{k-1} + step * (f_{k-1} /
 *        (f_{k-1} - f_k)); inv = bf / t*, weight = w_k, steps = k.  No crossing: inv = 0, weight = 0, steps = K.  A back-face
 *        crossing (f rising through 0) is ignored.  The fixed step is part of the definition.
 *   `origin` is the coverage of what the volume holds: origin_prev after an integrate.  inv, weight fp32 and steps int32 [B][H][W]
 *   may each be NULL, not all.  1 <= K <= 4096, inv_vs > 0, t0 >= 0, step > 0, w_min finite; rays [3][H][W]; 16-byte alignment.
 * No host synchronisation, no allocation: capturable.  No atomics: every slot and every pixel has one owner. */
int mvsgi_tsdf_integrate_f32(float* vol, const float* inv, const float* std, const unsigned char* mask, const float* T,
                             const int* origin, const int* origin_prev, float* range, long long B, int Nx, int Ny, int Nz, int H,
                             int W, float vs, float trunc, float t2, float w_max, float r_min, float r_max, float bf, float au,
                             float bu, float av, float bv, int wrap, mvsgi_stream_t stream);
int mvsgi_tsdf_raycast_f32(const float* vol, const float* rays, const float* P, const int* origin, float* inv, float* weight,
                           int* steps, long long B, int Nx, int Ny, int Nz, int H, int W, float inv_vs, float t0, float step, int K,
                           float w_min, float bf, mvsgi_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MVSGI_H */
