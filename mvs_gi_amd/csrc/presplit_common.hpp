// What the kernels on PRE-SPLIT activations share: K2g (csrc/conv3d_s2rs.hip) and K5 with its stride-2 layer (csrc/resblock2d_rs.hip)
// stage their windows with LDS-DMA copies and keep their weights in registers.  Defined once here: the activation, the split
// epilogue's half-trade, the window geometry with its DMA plan, the set-up of a persistent workgroup's walk, the tap of a lane's
// fragment and the weight packer (which csrc/conv3d_headsplit.hip's packer sits beside: another lane rule, the same split).
// Every form here leaves the kernels' assembly what it was (tools/isa_diff.py; DESIGN.md section 22 lists the forms that did not).
// Include inside the translation unit's anonymous namespace.
#pragma once

#include "split_fmt.hpp"

// LeakyReLU for slopes in [0, 1] as mul + max (plain asm max: __builtin_fmaxf first canonicalises an MFMA result with a third op)
__device__ __forceinline__ float lrelu(const float v, const float slope) {
    const float m = v * slope;
    float r;
    asm("v_max_f32 %0, %1, %2" : "=v"(r) : "v"(v), "v"(m));
    return r;
}

// The split epilogue of an MFMA result: lane (col, kg) holds channels 4 kg .. 4 kg + 3 of its voxel; hi | lo of the four, then
// lanes kg and kg ^ 1 trade halves: kg even ends up with hi, kg odd with lo of channels 8 (kg >> 1) .. + 7 -- one 16-byte chunk of
// the voxel's record [hi 0-7 | hi 8-15 | lo 0-7 | lo 8-15], at byte (kg & 1) * 32 + (kg >> 1) * 16.
template <bool F16>
__device__ __forceinline__ u32x4 ps_pack_split(const f32x4 v, float& satm) {
    u32x2 hi, lo;
    sf_split4<F16>(v, hi, lo, satm);
    const u32x2 sa = __builtin_amdgcn_permlane16_swap(hi[0], lo[0], false, false);
    const u32x2 sb = __builtin_amdgcn_permlane16_swap(hi[1], lo[1], false, false);
    return u32x4{sa[0], sb[0], sa[1], sb[1]};
}
// the bf16 split has no range to report
template <bool F16>
__device__ __forceinline__ u32x4 ps_pack_split(const f32x4 v) {
    static_assert(!F16, "the fp16 split keeps the lane's running maximum");
    float none = 0.f;
    return ps_pack_split<F16>(v, none);
}

// ---- windows ----
// A window is staged as two LDS regions, HI and LO (32 B per voxel each, the LO region REGION bytes behind), by DMA pieces of
// 32 voxels x 2 chunks of 16 B = 1 KiB: piece q of 2 PIECES, the four waves take q = wave + 4 m.  Lane l of a piece carries chunk
// l & 1 of LDS voxel 32 j + (l >> 1); its source offset within the window's descriptor is the plan.  Voxels past the window's last
// get an offset beyond num_records (zeros).  The source is a (2-D or 3-D) split-padded tensor of 64-byte records, Hp x Wp per plane.
template <int NPX_>
struct PsPieces {
    static constexpr int NPX = NPX_;                       // voxels of a window
    static constexpr int PIECES = (NPX + 31) / 32;         // DMA pieces per region
    static constexpr int DPW = 2 * PIECES / 4;             // pieces per wave (HI and LO regions)
    static constexpr int REGION = PIECES * 1024;           // HI region, the LO region right behind
    static constexpr int IMG = 2 * REGION;
    static_assert(2 * PIECES % 4 == 0, "whole pieces per wave");
};
// piece wave + 4 m of the window at LDS address `window`, from this lane's planned offset
__device__ __forceinline__ void ps_dma_piece(const __amdgpu_buffer_rsrc_t dsc, unsigned char* window, const int wave, const int m, const unsigned voff) {
    lds_dma16(dsc, window + (wave + 4 * m) * 1024, voff);
}
// Stride 1: LDS voxel v = window pixel (v / IW, v % IW).
template <int IH, int IW>
__device__ __forceinline__ unsigned ps_window_voff(const int q, const int lane, const int Wp) {
    constexpr int NPX = IH * IW, PIECES = PsPieces<NPX>::PIECES;
    const int region = q >= PIECES ? 1 : 0, j = q - region * PIECES;
    const int v = 32 * j + (lane >> 1), chunk = lane & 1;
    const int wy = v / IW, wx = v - wy * IW;
    return v < NPX ? (unsigned)((wy * Wp + wx) * 64 + region * 32 + chunk * 16) : 0xffffff00u;
}
// Stride 2: the window of IHt_ rows x 16 outputs (of PLANES input planes) is PLANES x IHt_ x 33 input voxels, and the plan
// DE-INTERLEAVES it on the way into LDS -- the 17 even columns, then the 16 odd columns of a row -- so that the 16 outputs of a tile
// read unit-stride voxels for every tap (kw = 0 | 2: even columns ow, ow + 1; kw = 1: odd column ow):
//   LDS voxel index = (plane * IHt + row) * 33 + (column odd ? 17 + column / 2 : column / 2)
template <int PLANES, int IHt_>
struct PsS2Window : PsPieces<PLANES * IHt_ * 33> {
    using PsPieces<PLANES * IHt_ * 33>::NPX;
    using PsPieces<PLANES * IHt_ * 33>::PIECES;
    static constexpr int TW = 16;                          // outputs per tile (one row)
    static constexpr int IW = 2 * TW + 1;                  // 33 input columns
    static constexpr int IHt = IHt_;                       // input rows
    static __device__ __forceinline__ unsigned voff(const int q, const int lane, const int Hp, const int Wp) {
        const int region = q >= PIECES ? 1 : 0, j = q - region * PIECES;
        const int v = 32 * j + (lane >> 1), chunk = lane & 1;
        const int pr = v / IW, e = v - pr * IW;               // (plane * IHt + row), slot in the row
        const int pl = PLANES == 1 ? 0 : pr / IHt, row = pr - pl * IHt;
        const int c = e <= TW ? 2 * e : 2 * (e - TW - 1) + 1;
        return v < NPX ? (unsigned)(((pl * Hp + row) * Wp + c) * 64 + region * 32 + chunk * 16) : 0xffffff00u;
    }
};

// LDS slot, within a row of window WIN, of input column 2 col + kw: what output COL reads under tap column KW.  (A macro: as a
// member function conv2d_s2rs_kernel comes out with another prologue.)
#define PS_S2_SLOT(WIN, KW, COL) (((KW) & 1) * (WIN::TW + 1) + (COL) + ((KW) >> 1))

// ---- the walk of a persistent workgroup ----
// Workgroup b of G walks N units, logical ids ID0 + k * STEP: XCD x walks a contiguous eighth of the units (xcd_remap; G is a
// multiple of 8, mvsgi::launch_persistent) -- or its one unit b when the grid covers every unit once (G == total, any G).
#define PS_WALK(TOTAL, N, ID0, STEP)                                                                                  \
    const int ps_total_ = (TOTAL), ps_g_ = gridDim.x;                                                                 \
    const int N = (ps_total_ - (int)blockIdx.x + ps_g_ - 1) / ps_g_;                                                  \
    const int ID0 = ps_g_ == ps_total_ ? (int)blockIdx.x : xcd_remap((int)blockIdx.x, ps_total_);                     \
    const int STEP = ps_g_ == ps_total_ ? 0 : ps_g_ >> 3;

// ---- fragments ----
// K of one MFMA = two taps x 16 channels: lane (col, kg) reads chunk kg & 1 (channels 8 (kg & 1) .. + 7) of the voxel under tap
// 2 p + (kg >> 1) of pair p.  An odd number of taps leaves the last pair's second slot without one: its weights are zeros, its
// lanes read the pair's first tap again.  (A macro of two statements: as a function of p, and as ONE nested conditional expression, the
// 2-D kernels come out with other prologues.)
#define PS_PAIR_TAP(T, P, KG, TAPS)                                                        \
    const int T##_a = 2 * (P), T##_b = 2 * (P) + 1 < (TAPS) ? 2 * (P) + 1 : 2 * (P);       \
    const int T = ((KG) >> 1) ? T##_b : T##_a;

// ---- weights ----
// [Cout 16 cts][Cin 16][TAPS] x scale[Cout] -> [cout tile cts][pairs][hi | lo][64 lanes][8 x 16 bit]
//   lane = (kg << 4) | i holds scale[co] * W[co = 16 ct + i][cin = (kg & 1) * 8 + j][tap = 2 p + (kg >> 1)]  (past the last tap: zeros)
// The BatchNorm scale is folded into the weights here (fp32 product, then hi | lo) and the shift is the accumulators' start
// value: the epilogues have no scale / shift arithmetic left.
template <int TAPS>
__global__ void ps_pack_weights_kernel(const float* __restrict__ w, const float* __restrict__ scale, bf16x8* __restrict__ wp, int cts, bool f16) {
    constexpr int PAIRS = (TAPS + 1) / 2;
    const int idx = blockIdx.x * 64 + threadIdx.x;
    if (idx >= cts * PAIRS * 64) return;
    const int lane = idx & 63, r = idx >> 6;
    const int p = r % PAIRS, ct = r / PAIRS;
    const int kg = lane >> 4, co = ct * 16 + (lane & 15), ci = (kg & 1) * 8, tap = 2 * p + (kg >> 1);
    u16x8 hi, lo;
    for (int j = 0; j < 8; ++j) {
        const float v = tap < TAPS ? w[((long long)co * 16 + ci + j) * TAPS + tap] * scale[co] : 0.f;
        unsigned short h_, l_;
        sf_split_weight(v, f16, h_, l_);
        hi[j] = h_;
        lo[j] = l_;
    }
    wp[((ct * PAIRS + p) * 2) * 64 + lane] = __builtin_bit_cast(bf16x8, hi);
    wp[((ct * PAIRS + p) * 2 + 1) * 64 + lane] = __builtin_bit_cast(bf16x8, lo);
}
