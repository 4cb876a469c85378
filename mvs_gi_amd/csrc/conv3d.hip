// K2: 3x3x3 convolution block for gfx950 -- conv3d(pad 1, stride 1|2) * scale + shift
// (+ residual) -> LeakyReLU, channels-last fp32.  Replaces BaseConvBlk3d.forward
// (dsta_mvs/model/common/common_modules.py:107-115) with eval-mode BatchNorm3d applied as
// the per-channel (scale, shift) of the epilogue.
//
// Two implementations behind one entry point:
//
//  * conv3d_mfma_kernel -- implicit GEMM on the exact-fp32 matrix instruction
//    v_mfma_f32_16x16x4_f32.  A workgroup owns a TD x TH x TW brick of output voxels and
//    a block of output channels; per 16-input-channel slice it stages the brick's halo
//    ((T-1)*stride+3 per axis) into LDS once and then runs the 27 taps as shifted LDS reads:
//         D[cout 16][voxel 16] += W[cout 16][k 4] * X[k 4][voxel 16]
//    A (weights) comes straight from HBM/L2 in a pre-packed, lane-ordered layout (one
//    coalesced 16-byte load per lane gives the 4 k-steps of a tap), B (activations) is one
//    ds_read_b128 per lane per tap (its 4 channels feed the same 4 k-steps), and the
//    accumulator tile leaves each lane holding 4 consecutive output channels of one voxel,
//    so the epilogue is a single 16-byte residual load and store per tile.
//    The MFMA result is bit-for-bit a k-ordered fmaf chain, i.e. plain fp32 arithmetic.
//
//  * conv3d_direct_kernel -- one thread per (voxel, group of CO output channels), any channel
//    counts; used for the Cout == 1 cost head (unet_regulator.py:61-68) and as the on-device
//    cross-check of the MFMA path.
#include "common.hpp"
#include "conv_common.hpp"
#include "conv3d_variants.hpp"
#ifdef MVSGI_STAMPS
#include <cstdio>
#include <cstdlib>
#endif

namespace {

// head layout (Cout == 1): [1][Cin][27] -> [27][Cin], so a tap's channels are contiguous and a
// wave-uniform 16-byte scalar load fetches four of them
__global__ void pack_head_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin) {
    const int idx = blockIdx.x * 256 + threadIdx.x;
    if (idx >= 27 * Cin) return;
    const int tap = idx / Cin, ci = idx % Cin;
    wp[idx] = w[ci * 27 + tap];
}

#include "conv3d_f32mfma.hpp"
#include "conv3d_bf16x3.hpp"

// ----------------------------------------------------------------------------------------
// cost head (Cout == 1, stride 1; unet_regulator.py:61-68), exact fp32 on the matrix cores.
//
// Cout == 1 has no output-channel dimension for an implicit GEMM, but the 27 TAPS can play that
// role:  P[t][u] = sum_c w[t][c] * x[u][c]  is a [27 -> 32] x [Cin] x [voxels] product, and
//        out[v]  = sum_t P[t][v + offset(t)]  is a sum of 27 shifted copies of it.
// A workgroup owns an 8 x 32 (h, w) window of one frame and MARCHES along D.  Per input plane p:
//   1. every wave multiplies its 32-voxel tiles of the 10 x 34 halo window by all taps with
//      v_mfma_f32_32x32x2_f32 (bit-for-bit fp32 FMAs).  The weights are the A operand (8 VGPRs hold
//      a 16-channel slice of all 27 taps), the activations go from global memory straight into
//      the B operand (lane = (voxel, channel half): two 16-byte loads, no LDS staging, every
//      input voxel fetched once per window);
//   2. P[27][window] goes to LDS (36 KB), and after one barrier thread (h, w) adds its 3 x 3 x 3
//      taps into THREE running outputs -- od = p-1 (kd = 2), p (kd = 1), p+1 (kd = 0) -- 27
//      conflict-free ds_read_b32 per output instead of the 108 ds_read_b128 of a brick-per-
//      workgroup FMA kernel, which was LDS-bound (and whose 432 scalar-loaded weights per slice
//      the compiler spilled).
// The loads of plane p+1 are in flight while plane p is reduced.
// ----------------------------------------------------------------------------------------

__global__ __launch_bounds__(256) void conv3d_head_kernel(ConvArgs a, int dchunk, int nd) {
    constexpr int TH = 8, TW = 32, ITH = TH + 2, ITW = TW + 2, PV = ITH * ITW;
    constexpr int NT = (PV + 31) / 32;               // 32-voxel tiles of the halo window (11)
    constexpr int TPW = (NT + 3) / 4;                // tiles per wave (3)
    constexpr int PSTR = 360;                        // row stride of P: rows 4 apart land 32 banks apart
    static_assert(NT * 32 <= PSTR, "P row too short");
    extern __shared__ __attribute__((aligned(16))) float pbuf[];     // [27][PSTR]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int n = lane & 31, h = lane >> 5;
    int t = xcd_remap((int)blockIdx.x, (int)gridDim.x);     // an XCD owns a contiguous run of windows: neighbours' halo rows / columns hit its L2
    const int tw_i = t % a.tiles_w;
    t /= a.tiles_w;
    const int th_i = t % a.tiles_h;
    t /= a.tiles_h;
    const int dc = t % nd;
    const int b = t / nd;
    const int oh0 = th_i * TH, ow0 = tw_i * TW;
    const int od_begin = dc * dchunk;
    const int od_end = od_begin + dchunk < a.Do ? od_begin + dchunk : a.Do;
    const int p0 = od_begin > 0 ? od_begin - 1 : 0;
    const int p1 = od_end < a.Din - 1 ? od_end : a.Din - 1;          // inclusive
    const int nchunks = a.Cin / 16;
    const int U = (p1 - p0 + 1) * nchunks;

    // this lane's voxel of each of the wave's tiles (the same for every plane)
    int goff[TPW];
    bool ok[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k) {
        const int T = wave + 4 * k, v = T * 32 + n;
        const int ih = v / ITW, iw = v - ih * ITW;
        const int gh = oh0 - 1 + ih, gw = ow0 - 1 + iw;
        ok[k] = T < NT && v < PV && gh >= 0 && gh < a.Hin && gw >= 0 && gw < a.Win;
        goff[k] = ok[k] ? (gh * a.Win + gw) * a.Cin + 8 * h : 0;
    }
    const long long plane_stride = (long long)a.Hin * a.Win * a.Cin;
    const float* xb = a.x + (long long)b * a.Din * plane_stride;
    // A operand: lane (row = tap n, k-half h) holds w[tap][16*cs + 8*h + j], j = 0..7; rows >= 27 are 0
    const float* wrow = reinterpret_cast<const float*>(a.wp) + (n < 27 ? n : 0) * a.Cin + 8 * h;
    f32x4 wa[2], xr[TPW][2];
#define MVSGI_HEAD_FETCH(P, CS)                                                                     \
    {                                                                                               \
        const float* src_ = xb + (long long)(P) * plane_stride + (CS) * 16;                         \
        _Pragma("unroll") for (int k = 0; k < TPW; ++k) {                                           \
            xr[k][0] = *reinterpret_cast<const f32x4*>(src_ + goff[k]);                             \
            xr[k][1] = *reinterpret_cast<const f32x4*>(src_ + goff[k] + 4);                         \
        }                                                                                           \
        wa[0] = *reinterpret_cast<const f32x4*>(wrow + (CS) * 16);                                  \
        wa[1] = *reinterpret_cast<const f32x4*>(wrow + (CS) * 16 + 4);                              \
    }
    MVSGI_HEAD_FETCH(p0, 0)

    const int h_ = tid / TW, w_ = tid % TW;
    const int oh = oh0 + h_, ow = ow0 + w_;
    const bool inside = oh < a.Ho && ow < a.Wo;
    const float sc = a.scale[0], sh = a.shift[0];
    float run[3] = {0.f, 0.f, 0.f};                   // outputs od = p-1, p, p+1 under construction
    f32x16 acc[TPW];
#pragma unroll
    for (int k = 0; k < TPW; ++k)
#pragma unroll
        for (int i = 0; i < 16; ++i) acc[k][i] = 0.f;

    int p = p0, cs = 0;
    // A finished output is stored at the START of the next step, ahead of that step's loads: loads and stores retire through
    // one in-order counter, so a store issued behind the loads a step waits for would put its own round trip on the path.
    float pend = 0.f;
    long long pend_vox = -1;
    for (int u = 0; u < U; ++u) {
        int ncs = cs + 1, np = p;
        if (ncs == nchunks) { ncs = 0; np = p + 1; }
        const f32x4 w0 = n < 27 ? wa[0] : f32x4{0.f, 0.f, 0.f, 0.f};
        const f32x4 w1 = n < 27 ? wa[1] : f32x4{0.f, 0.f, 0.f, 0.f};
        f32x4 cx[TPW][2];
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            cx[k][0] = ok[k] ? xr[k][0] : f32x4{0.f, 0.f, 0.f, 0.f};
            cx[k][1] = ok[k] ? xr[k][1] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        if (pend_vox >= 0) {
            a.y[pend_vox] = pend;
            pend_vox = -1;
        }
        {   // the next unit's operands, requested before this unit is multiplied (past the end: this unit again, unused);
            // unconditional, so that every wait behind it is counted exactly
            const int fp = u + 1 < U ? np : p, fcs = u + 1 < U ? ncs : cs;
            MVSGI_HEAD_FETCH(fp, fcs)
        }
#pragma unroll
        for (int k = 0; k < TPW; ++k) {
            if (wave + 4 * k < NT) {                 // wave-uniform
                const f32x4 x0 = cx[k][0];
                const f32x4 x1 = cx[k][1];
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(w0[j], x0[j], acc[k], 0, 0, 0);
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[k] = __builtin_amdgcn_mfma_f32_32x32x2f32(w1[j], x1[j], acc[k], 0, 0, 0);
            }
        }
        if (ncs == 0) {
            // P of plane p: lane (n, h) holds rows (i / 4) * 8 + 4 * h + i % 4 of voxel T * 32 + n
#pragma unroll
            for (int k = 0; k < TPW; ++k) {
                if (wave + 4 * k < NT) {
                    const int v = (wave + 4 * k) * 32 + n;
#pragma unroll
                    for (int i = 0; i < 16; ++i) {
                        const int row = (i / 4) * 8 + 4 * h + (i % 4);
                        if (row < 27) pbuf[row * PSTR + v] = acc[k][i];
                        acc[k][i] = 0.f;
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int k2 = 0; k2 < 9; ++k2) {
                const int vv = (h_ + k2 / 3) * ITW + (w_ + k2 % 3);
                run[0] += pbuf[(18 + k2) * PSTR + vv];      // kd = 2 -> od = p - 1
                run[1] += pbuf[(9 + k2) * PSTR + vv];       // kd = 1 -> od = p
                run[2] += pbuf[k2 * PSTR + vv];             // kd = 0 -> od = p + 1
            }
            const int od = p - 1;
            if (od >= od_begin && inside) {
                const long long vox = (((long long)b * a.Do + od) * a.Ho + oh) * a.Wo + ow;
                float r = run[0] * sc + sh;
                if (a.res) r += a.res[vox];
                pend = r > 0.f ? r : r * a.neg_slope;
                pend_vox = vox;
            }
            run[0] = run[1];
            run[1] = run[2];
            run[2] = 0.f;
            __syncthreads();                         // P consumed before the next plane overwrites it
        }
        p = np;
        cs = ncs;
    }
    if (pend_vox >= 0) a.y[pend_vox] = pend;
    if (p1 < od_end && inside) {                     // the last plane of the volume: no plane behind it
        const long long vox = (((long long)b * a.Do + p1) * a.Ho + oh) * a.Wo + ow;
        float r = run[0] * sc + sh;
        if (a.res) r += a.res[vox];
        a.y[vox] = r > 0.f ? r : r * a.neg_slope;
    }
#undef MVSGI_HEAD_FETCH
}

// ----------------------------------------------------------------------------------------
// direct convolution: thread = (voxel, CO consecutive couts); weights in PyTorch OIDHW order
// ----------------------------------------------------------------------------------------
template <int CO>
__global__ __launch_bounds__(256) void conv3d_direct_kernel(ConvArgs a) {
    const int groups = (a.Cout + CO - 1) / CO;
    const long long total = (long long)a.B * a.Do * a.Ho * a.Wo * groups;
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= total) return;
    const int cg = (int)(idx % groups);
    const long long vox = idx / groups;
    const int ow = (int)(vox % a.Wo);
    const int oh = (int)((vox / a.Wo) % a.Ho);
    const int od = (int)((vox / ((long long)a.Wo * a.Ho)) % a.Do);
    const int b = (int)(vox / ((long long)a.Wo * a.Ho * a.Do));
    const int co0 = cg * CO;
    float acc[CO];
#pragma unroll
    for (int o = 0; o < CO; ++o) acc[o] = 0.f;
    for (int kd = 0; kd < 3; ++kd) {
        const int id = od * a.stride - 1 + kd;
        if (id < 0 || id >= a.Din) continue;
        for (int kh = 0; kh < 3; ++kh) {
            const int ih = oh * a.stride - 1 + kh;
            if (ih < 0 || ih >= a.Hin) continue;
            for (int kw = 0; kw < 3; ++kw) {
                const int iw = ow * a.stride - 1 + kw;
                if (iw < 0 || iw >= a.Win) continue;
                const int tap = (kd * 3 + kh) * 3 + kw;
                const float* xp = a.x + ((((long long)b * a.Din + id) * a.Hin + ih) * a.Win + iw) * a.Cin;
                for (int ci = 0; ci < a.Cin; ++ci) {
                    const float xv = xp[ci];
#pragma unroll
                    for (int o = 0; o < CO; ++o) {
                        const int co = co0 + o;
                        if (co < a.Cout) acc[o] = fmaf(xv, a.w_oidhw[((long long)co * a.Cin + ci) * 27 + tap], acc[o]);
                    }
                }
            }
        }
    }
#pragma unroll
    for (int o = 0; o < CO; ++o) {
        const int co = co0 + o;
        if (co >= a.Cout) break;
        float r = acc[o] * a.scale[co] + a.shift[co];
        if (a.res) r += a.res[vox * a.Cout + co];
        r = r > 0.f ? r : r * a.neg_slope;
        a.y[vox * a.Cout + co] = r;
    }
}

int launch_head(ConvArgs a, hipStream_t st) {
    constexpr size_t lds_bytes = (size_t)27 * 360 * sizeof(float);      // P[27][PSTR]
    a.tiles_h = (int)mvsgi::cdiv(a.Ho, 8);
    a.tiles_w = (int)mvsgi::cdiv(a.Wo, 32);
    // split D only when the (frame, window) count alone cannot fill the chip (each chunk re-reads
    // its two boundary planes)
    const long long windows = (long long)a.B * a.tiles_h * a.tiles_w;
    long long nd = windows >= 1024 ? 1 : mvsgi::cdiv(1024, windows);
    if (nd > mvsgi::cdiv(a.Do, 2)) nd = mvsgi::cdiv(a.Do, 2);
    const int dchunk = (int)mvsgi::cdiv(a.Do, nd);
    nd = mvsgi::cdiv(a.Do, dchunk);
    a.tiles_d = (int)nd;
    const long long nt = windows * nd;
    MVSGI_REQUIRE(nt < (1ll << 31), "conv3d: too many tiles");
    MVSGI_REQUIRE((long long)a.Hin * a.Win * a.Cin < (1ll << 31), "conv3d(head): plane too large for 32-bit offsets");
    hipLaunchKernelGGL(conv3d_head_kernel, dim3((unsigned)nt), dim3(256), lds_bytes, st, a, dchunk, (int)nd);
    return mvsgi::check_launch("mvsgi_conv3d_f32(head)");
}

int launch_direct(const ConvArgs& a, hipStream_t st) {
    const long long vox = (long long)a.B * a.Do * a.Ho * a.Wo;
    if (a.Cout == 1) {
        hipLaunchKernelGGL((conv3d_direct_kernel<1>), dim3((unsigned)mvsgi::cdiv(vox, 256)), dim3(256), 0, st, a);
    } else {
        const long long total = vox * mvsgi::cdiv(a.Cout, 4);
        hipLaunchKernelGGL((conv3d_direct_kernel<4>), dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0, st, a);
    }
    return mvsgi::check_launch("mvsgi_conv3d_f32(direct)");
}

// 32x32x16 schedule: Cout % 32 == 0, stride 1, and enough bricks to fill the chip with its two brick shapes
bool v32_applies(const ConvArgs& a) {
    if (a.Cout % 32 || a.Cin % 16 || a.stride != 1) return false;
    const long long big = (long long)a.B * mvsgi::cdiv(a.Do, 4) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
    const long long mid = (long long)a.B * mvsgi::cdiv(a.Do, 2) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
    return a.Cout == 32 ? big >= 384 : mid * mvsgi::cdiv(a.Cout, 64) >= 384;
}

// variant of the fused upsample + conv (a holds the UPSAMPLED input size); V_COUNT when unsupported
int select_variant_up2(const ConvArgs& a, int w_layout) {
    if (w_layout == MVSGI_CONV_BF16X3_D32) {      // 32-channel slices: the sibling of the 2 x 4 x 16-brick variant, where that is the choice
        const int base = a.Cin % 32 ? V_COUNT : select_variant_up2(a, MVSGI_CONV_BF16X3);
        const bool d2 = a.Do == 2;
        if (base == B3U_N64) return d2 ? B3DU2_N64 : B3DU_N64;
        if (base == B3U_N96) return d2 ? B3DU2_N96 : B3DU_N96;
        mvsgi::fail("mvsgi_conv3d_up2_f32: the 32-channel-slice kernels do not apply to this problem (see mvsgi_conv3d_up2_d32_applies)");
        return V_COUNT;
    }
    const bool c16_layout = w_layout == MVSGI_CONV_BF16X3_C16;
    if (w_layout == MVSGI_CONV_BF16X3_V32) {
        if (!v32_applies(a) || !a.wp) { mvsgi::fail("mvsgi_conv3d_up2_f32: the 32x32x16 kernel does not apply to this problem"); return V_COUNT; }
        return a.Cout == 32 ? B3VU_N32 : B3VU_N64;
    }
    if (a.Cin % 16 || a.Cout % 16) {
        mvsgi::fail("mvsgi_conv3d_up2_f32: Cin, Cout must be multiples of 16 (got %d, %d)", a.Cin, a.Cout);
        return V_COUNT;
    }
    if (!a.wp) { mvsgi::fail("mvsgi_conv3d_up2_f32: needs w_packed (bf16x3 layout)"); return V_COUNT; }
    const int CT = a.Cout / 16;
    const long long big = (long long)a.B * mvsgi::cdiv(a.Do, 4) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
    const long long mid = (long long)a.B * mvsgi::cdiv(a.Do, 2) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
    if (CT == 1) return c16_layout ? B3PU_N16 : B3U_N16;
    if (CT == 2) {
        // 256-voxel bricks from 384 units on; below, whichever of the two brick sizes makes the cheaper rounds (a 256-voxel unit takes
        // ~1.6 x a 128-voxel one, a further round 0.85 of the first): 64 -> 32 onto [8,40,160] at one frame 24.2 -> 20.4 us (200 units
        // in one round against 400 in two)
        if (big >= 384) return B3U_N32;
        const long long cus = mvsgi::device_cus(), r32 = mvsgi::cdiv(big, cus), rm = mvsgi::cdiv(mid, cus);
        return 157 * (100 + 85 * (r32 - 1)) < 100 * (100 + 85 * (rm - 1)) ? B3U_N32 : B3U_N32_M;
    }
    if (CT == 3) return B3U_N48;
    if (CT % 6 == 0 && mid * (CT / 6) >= 384) return B3U_N96;
    // a launch that 64-voxel bricks x 32 couts cover in ONE round of the chip (an up block at one frame): waves as (voxel half, cout
    // tile), as B3_N32_TB below.  128 -> 64 onto [4,20,80] x 1 frame: 50 units of B3U_N64 30.2 us, 200 of these 17.2; 384 -> 192 onto
    // [2,10,40]: 77.6 -> 40.7; two frames 30.5 / 29.4, four 34.4 / 56.2)
    if (CT % 2 == 0 && (long long)a.B * mvsgi::cdiv(a.Do, 2) * mvsgi::cdiv(a.Ho, 2) * mvsgi::cdiv(a.Wo, 16) * (CT / 2) <= mvsgi::device_cus())
        return B3U_N32_TB;
    return B3U_N64;
}

int select_variant(const ConvArgs& a, int impl);

// MVSGI_CONV_BF16X3_D32: the 32-channel-slice sibling of the variant the split kernel would take for this problem (Cin % 32 == 0,
// stride 1, a launch large enough for one of the bricks of conv3d_b3d_variants.inc), or V_COUNT (no error text)
int d32_variant(const ConvArgs& a) {
    if (a.stride != 1 || a.Cin % 32 || a.Cout % 16) return V_COUNT;
    ConvArgs b = a;
    static const float dummy = 0.f;
    if (!b.wp) b.wp = reinterpret_cast<const f32x4*>(&dummy);      // (the query form has no weights)
    const bool d2 = a.Do == 2;      // a volume two planes deep: the depth-skip siblings
    switch (select_variant(b, MVSGI_CONV_BF16X3)) {
        case B3_N64: return d2 ? B3D2_N64 : B3D_N64;
        case B3_N64_H5: return d2 ? B3D2_N64_H5 : B3D_N64_H5;
        case B3_N64_W8: return d2 ? B3D2_N64_W8 : B3D_N64_W8;
        case B3_N96: return d2 ? B3D2_N96 : B3D_N96;
        case B3_N96_H5: return d2 ? B3D2_N96_H5 : B3D_N96_H5;
        case B3_N96_W8: return d2 ? B3D2_N96_W8 : B3D_N96_W8;
        case B3_N128_P: return B3D_N128_P;
        case B3_N128_PH5: return B3D_N128_PH5;
        case B3_N128_PW8: return B3D_N128_PW8;
        case B3_N192_PH5: return B3D_N192_PH5;
        case B3_N192_PW8: return B3D_N192_PW8;
        // (a volume two planes deep on the one-plane small-launch units: 18 of 27 slots; also instead of the 16-cout units with their
        // weight slice in LDS, which are tap-pair kernels: 128 -> 128 on one [2,10,40] frame 13.2 us)
        case B3_N16_TW: return d2 && a.Cout % 32 == 0 ? B3D2_N32_TB : V_COUNT;
        case B3_N32_TB: return d2 ? B3D2_N32_TB : B3D_N32_TB;
        case B3_N64_S: return d2 ? B3D2_N64_S : B3D_N64_S;
        default: return V_COUNT;
    }
}

// returns V_COUNT when the request cannot be served (error text already set)
int select_variant(const ConvArgs& a, int impl) {
    const bool mfma_ok = (a.Cin % 16 == 0) && (a.Cout % 16 == 0);
    const bool head_ok = (a.Cout == 1) && (a.Cin % 16 == 0) && (a.stride == 1);
    if (impl == MVSGI_CONV_BF16X3_C16) {
        if (a.Cout != 16 || a.Cin % 16 || a.stride != 1) {
            mvsgi::fail("mvsgi_conv3d_f32: the Cout == 16 plane kernel needs Cout == 16, Cin %% 16 == 0, stride 1 (got %d, %d, %d)",
                        a.Cout, a.Cin, a.stride);
            return V_COUNT;
        }
        if (!a.wp) { mvsgi::fail("mvsgi_conv3d_f32: tiled path needs w_packed"); return V_COUNT; }
        return B3P_N16;
    }
    if (impl == MVSGI_CONV_BF16X3_V32) {
        if (!v32_applies(a)) {
            mvsgi::fail("mvsgi_conv3d_f32: the 32x32x16 kernel does not apply to this problem (see mvsgi_conv3d_v32_applies)");
            return V_COUNT;
        }
        if (!a.wp) { mvsgi::fail("mvsgi_conv3d_f32: tiled path needs w_packed"); return V_COUNT; }
        return a.Cout == 32 ? B3V_N32 : B3V_N64;
    }
    if (impl == MVSGI_CONV_BF16X3_D32) {
        const int v = d32_variant(a);
        if (v == V_COUNT) mvsgi::fail("mvsgi_conv3d_f32: the 32-channel-slice kernels do not apply to this problem (see mvsgi_conv3d_d32_applies)");
        else if (!a.wp) { mvsgi::fail("mvsgi_conv3d_f32: tiled path needs w_packed"); return V_COUNT; }
        return v;
    }
    if (impl == MVSGI_CONV_BF16X3 && !mfma_ok) impl = MVSGI_CONV_AUTO;   // head / odd channels: exact paths
    if (impl == MVSGI_CONV_AUTO) impl = (mfma_ok || head_ok) ? MVSGI_CONV_MFMA : MVSGI_CONV_DIRECT;
    if (impl == MVSGI_CONV_DIRECT) {
        if (!a.w_oidhw) { mvsgi::fail("mvsgi_conv3d_f32: direct path needs w_oidhw"); return V_COUNT; }
        return a.Cout == 1 ? V_DIRECT1 : V_DIRECT4;
    }
    if (impl != MVSGI_CONV_MFMA && impl != MVSGI_CONV_BF16X3) {
        mvsgi::fail("mvsgi_conv3d_f32: unknown impl %d", impl);
        return V_COUNT;
    }
    if (!a.wp) { mvsgi::fail("mvsgi_conv3d_f32: tiled path needs w_packed"); return V_COUNT; }
    if (head_ok && impl == MVSGI_CONV_MFMA) return V_HEAD;
    if (!mfma_ok) {
        mvsgi::fail("mvsgi_conv3d_f32: MFMA path needs Cin, Cout multiples of 16 (got %d, %d)", a.Cin, a.Cout);
        return V_COUNT;
    }
    const int CT = a.Cout / 16;
    const long long vox = (long long)a.B * a.Do * a.Ho * a.Wo;
    if (impl == MVSGI_CONV_BF16X3) {
        if (a.stride == 2) {
            // as many couts per workgroup as divide the layer evenly and still leave a few units per CU: a stride-2 brick stages
            // 12 input voxels per output voxel and slice, once per cout block (96 -> 192 at 32 frames: 879 us in 64-cout units, 688 in
            // 192-cout units; 192 -> 384: 478 -> 352; 16 -> 96: 933 -> 744)
            const long long s2bricks = (long long)a.B * mvsgi::cdiv(a.Do, 2) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 8);
            // (Round 6: 2 x 2 x 16 bricks -- conflict-free stride-2 fragment reads: LDS conflict cycles -63 %, the layers' time
            // -1.5 % ... +7.7 % for 8 % more halo to stage -- measured equal or slower, profiles/r06_stride2_brick_shapes.txt)
            if (CT % 12 == 0 && s2bricks * (CT / 12) >= 512) return B3_S2_N192;
            if (CT % 8 == 0 && s2bricks * (CT / 8) >= 512) return B3_S2_N128;
            if (CT % 6 == 0 && s2bricks * (CT / 6) >= 512) return B3_S2_N96;
            // 32 couts per unit: waves as (voxel half, cout tile) -- 2 weight + 4 activation fragment reads per slot and wave instead of
            // 4 + 2 with all four waves on both cout tiles (4cam-32's first layer, 64 -> 32: 1362 -> 1221 us per 16 frames)
            // ... and for a launch they cover in one round of the chip where the 64-cout units leave most CUs idle (round 6, hipGraph
            // of 20 launches: 64 -> 128 from [4,20,80] at 1 / 2 / 4 frames 13.7 -> 10.8, 13.9 -> 11.2, 14.6 -> 12.8 us, at 8: 16.0 vs 21.4;
            // 32 -> 64 from [8,40,160] at one frame 10.0 -> 8.9, at two 10.9 vs 13.4)
            if (CT <= 3 || s2bricks * mvsgi::cdiv(CT, 2) <= mvsgi::device_cus()) return B3_S2_N32B;
            return B3_S2_N64;
        }
        // workgroups a 256-voxel (N <= 48) / 128-voxel (N >= 64) brick decomposition would give
        const long long big = (long long)a.B * mvsgi::cdiv(a.Do, 4) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
        const long long mid = (long long)a.B * mvsgi::cdiv(a.Do, 2) * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
        if (CT == 1) return B3_N16;
        if (CT == 2) return big >= 384 ? B3_N32 : B3_N32_TB;      // (B3_N32_S until round 6: see the small-launch rule below)
        if (CT == 3) return B3_N48;
        const bool h5ok = a.Ho % 5 == 0 && a.Ho % 4 != 0;
        // 10 x 8 bricks instead of 5 x 16 where they cover the plane exactly and the 16-wide ones pad it (round 6; 128 -> 128 on
        // [2,10,40] x 128 frames: 231 -> 203 us, x 64: 126 -> 114, x 32: 81 -> 76; same sums bit for bit)
        const bool w8 = a.Ho % 10 == 0 && a.Wo % 16 == 8;
        // one-plane volumes (the coarsest level of an 8-candidate regulator): bricks one plane thick -- a 2-plane brick would do
        // half of its MFMAs on padding.  All four consumer waves share the brick's voxel tiles and split the couts.
        if (a.Do == 1 && CT >= 8 && CT % 4 == 0) {
            const long long rows5 = (long long)a.B * (a.Ho / 5) * mvsgi::cdiv(a.Wo, 16);
            if (h5ok && CT % 12 == 0 && rows5 * (CT / 12) >= 384) return w8 ? B3_N192_PW8 : B3_N192_PH5;
            // (a launch of a few frames has too few of these units to fill the chip -- 384 -> 384 at one frame: 18 workgroups walking
            // 24 slices each -- and falls through to the small-launch rule below)
            if (h5ok && CT % 8 == 0 && rows5 * (CT / 8) >= mvsgi::device_cus() / 2) return w8 ? B3_N128_PW8 : B3_N128_PH5;
            if (CT % 8 == 0 && (long long)a.B * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16) * (CT / 8) >= 384) return B3_N128_P;
        }
        if (CT % 6 == 0 && h5ok &&
            (long long)a.B * mvsgi::cdiv(a.Do, 2) * (a.Ho / 5) * mvsgi::cdiv(a.Wo, 16) * (CT / 6) >= 384) return w8 ? B3_N96_W8 : B3_N96_H5;
        if (CT % 6 == 0 && mid * (CT / 6) >= 384) return B3_N96;
        const long long cus = mvsgi::device_cus();
        // A launch of a few rounds (2 ... 24 frames of the (16, 32) regulator's levels 1 and 2: under four rounds of the 128-voxel x
        // 64-cout units): a workgroup fills a CU, the launch runs in rounds of one unit per CU, and WHICH unit shape puts the launch
        // into the fewest, fullest rounds changes with every frame count -- the variant of the lowest estimated time instead of unit
        // thresholds.  A unit of Cin / 16 slices takes a + b * slices; a further round of a launch 0.85 of its first (measured per
        // launch, hipGraph of 20, profiles/r06_mid_batch_units_probe.txt; us):
        //   64 -> 64 [4,20,80]   x 3: 23.1 (TB) / 23.7 (64_S) / 19.0 (N64) / 22.5 (N64_H5);  x 4: 29.8 / 24.3 / 19.8 / 22.9;
        //                        x 6: 39.2 / 35.2 / 34.7 / 24.8;  x 12: 73.7 / 55.7 / 50.9 / 45.6
        //   128 -> 128 [2,10,40] x 4: 25.9 / 21.1 / 29.3 / 36.7;  x 8: 37.7 / 38.6 / 29.5 / 36.7;  x 16: 63.9 / 57.3 / 56.8 / 37.8
        // (the rules below picked 64_S, 64_S, 64_S, N64 and 64_S, TB, 64_S there).  CT % 6 == 0 layers keep their 96-cout rules.
        if (CT % 4 == 0 && CT % 6 != 0 && mid * (CT / 4) < 4 * cus) {
            const long long tiny = (long long)a.B * a.Do * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
            if (tiny * CT <= cus) return B3_N16_TW;             // one round of 16-cout units with the weight slice in LDS (below)
            const long long slices = a.Cin / 16;
            struct Cand { int v; long long units, a_ns, b_ns; };
            const Cand cand[] = {
                {B3_N32_TB, tiny * (CT / 2), 5700, 1000},
                {B3_N64_S, tiny * (CT / 4), 6600, 1700},
                {B3_N64, mid * (CT / 4), 8700, 2600},
                {w8 ? B3_N64_W8 : B3_N64_H5, a.Ho % 5 ? 0 : (long long)a.B * mvsgi::cdiv(a.Do, 2) * (CT / 4) *
                                                 (w8 ? (a.Ho / 10) * (a.Wo / 8) : (a.Ho / 5) * mvsgi::cdiv(a.Wo, 16)), 8400, 3500},
            };
            int best = B3_N64;
            long long best_cost = -1;
            for (const Cand& c : cand) {
                if (c.units <= 0) continue;
                const long long rounds = mvsgi::cdiv(c.units, cus);
                const long long cost = (c.a_ns + c.b_ns * slices) * (100 + 85 * (rounds - 1));
                if (best_cost < 0 || cost < best_cost) { best_cost = cost; best = c.v; }
            }
            return best;
        }
        // planes whose height is a multiple of 5 but not of 4 (the 10 x 40 planes of UNet level 2): 2 x 5 x 16 bricks cover them
        // exactly where 2 x 4 x 16 ones pad 10 rows to 12 (17 % of the MFMAs) and stage 7 % more halo per voxel
        if (h5ok && (long long)a.B * mvsgi::cdiv(a.Do, 2) * (a.Ho / 5) * mvsgi::cdiv(a.Wo, 16) * mvsgi::cdiv(CT, 4) >= 384)
            return w8 ? B3_N64_W8 : B3_N64_H5;
        if (mid * mvsgi::cdiv(CT, 4) >= 384) return B3_N64;
        // a few frames (latency path): 64-voxel bricks.  A workgroup of this kernel fills a CU (8 waves x 256 registers), so a launch
        // runs in rounds of one unit per CU and a round costs its unit's Cin / 16 slices end to end: the couts per unit are the
        // FEWEST that still put every unit into the first round.  Measured per launch (MI355X, hipGraph replay),
        // 16 / 32 / 64 couts per unit: 64 -> 64 [4,20,80] x 1 frame 14.8 / 12.2 / 12.4 us, x 2 frames 25.5 / 20.1 / 12.8;
        // 128 -> 128 [2,10,40] x 1: 13.2 / 18.9 / 20.0, x 2: 23.1 / 18.8 / 19.9, x 4: 32.6 / 34.5 / 20.2 -- round 3's rule picked
        // the variant with AT LEAST 256 units instead (x 4: 35.4 us).  The 16-cout units take their weight slice through LDS
        // (conv3d_bf16x3.hpp, WLDS: the four consumer waves share it; 13.2 -> 12.7 us).
        // Round 6: the 32-cout units as (voxel half, cout tile) waves (B3_N32_TB) instead of four waves on both cout tiles (B3_N32_T):
        // in-kernel stamps of the latter (tools/stamp_probe.py) showed a slice's 84 MFMAs per wave (1344 cycles) taking 4200 -- each
        // of the four waves fetching the SAME 4 weight fragments per slot, 16 KiB per slot and CU through a vector-memory path that
        // returns 64 B per clock.  Two waves per cout tile halve that (8 KiB of weights, 16 KiB of LDS reads per slot: balanced):
        // 64 -> 64 x 1 frame 12.5 -> 9.7 us, x 2: 20.7 -> 15.4; 128 -> 128 x 2: 19.4 -> 13.9, x 8: 50.5 -> 34.9 (N64_S: 36.8).  It takes
        // a launch whenever its rounds cost less than the 64-cout units' (a round of it ~ 0.7 of theirs).
        const long long tiny = (long long)a.B * a.Do * mvsgi::cdiv(a.Ho, 4) * mvsgi::cdiv(a.Wo, 16);
        if (tiny * CT <= cus) return B3_N16_TW;                 // (128 -> 128 [2,10,40] x 1 frame: 13.2 us against B3_N32_TB's 13.7)
        const long long rounds32 = mvsgi::cdiv(tiny * mvsgi::cdiv(CT, 2), cus), rounds64 = mvsgi::cdiv(tiny * mvsgi::cdiv(CT, 4), cus);
        return 2 * rounds32 <= 3 * rounds64 ? B3_N32_TB : B3_N64_S;
    }
    if (a.stride == 1) {
        if (CT == 1) return V_S1_N16_B256;
        if (CT <= 3) return vox >= 256ll * 512 ? V_S1_N32_B256 : V_S1_N32_B64;
        return vox * CT >= 128ll * 4 * 1024 ? V_S1_N64_B128 : V_S1_N64_B64;
    }
    return CT <= 3 ? V_S2_N32_B64 : V_S2_N64_B64;
}

int launch_variant(int v, const ConvArgs& a, hipStream_t st) {
    if (a.f16) return mvsgi::conv3d_launch_b3_f16(v, &a, st);      // the fp16 split: the same variants, instantiated in conv3d_f16.hip
    switch (v) {
        case V_DIRECT1:
        case V_DIRECT4: return launch_direct(a, st);
        case V_HEAD: return launch_head(a, st);
#define MVSGI_MFMA(V, ...) case V: return launch_mfma<__VA_ARGS__>(a, st);
#define MVSGI_B3(V, K, ...) case V: return MVSGI_B3_LAUNCH##K(false, __VA_ARGS__)(a, st);
#include "conv3d_variants.inc"
#undef MVSGI_MFMA
#undef MVSGI_B3
    }
    return mvsgi::fail("mvsgi_conv3d_f32: bad variant %d", v);
}

int fill_args(ConvArgs& a, const float* x, const float* w_oidhw, const float* w_packed, const float* scale,
              const float* shift, const float* res, float* y, int B, int Cin, int Din, int Hin, int Win, int Cout,
              int stride, float neg_slope) {
    MVSGI_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && Din > 0 && Hin > 0 && Win > 0, "mvsgi_conv3d_f32: bad dims");
    MVSGI_REQUIRE(stride == 1 || stride == 2, "mvsgi_conv3d_f32: stride %d not in {1, 2}", stride);
    a.x = x;
    a.w_oidhw = w_oidhw;
    a.wp = reinterpret_cast<const f32x4*>(w_packed);
    a.scale = scale;
    a.shift = shift;
    a.res = res;
    a.y = y;
    a.B = B;
    a.Cin = Cin;
    a.Din = Din;
    a.Hin = Hin;
    a.Win = Win;
    a.Cout = Cout;
    a.stride = stride;
    a.neg_slope = neg_slope;
    a.Do = (Din - 1) / stride + 1;   // k=3, pad=1
    a.Ho = (Hin - 1) / stride + 1;
    a.Wo = (Win - 1) / stride + 1;
    return 0;
}

// MVSGI_CONV_F16 OR-ed into a split-kernel selector (MVSGI_CONV_BF16X3 / _C16 / _V32): strips the flag and records it in the
// launch arguments; any other selector with the flag is an error
int split_flag(ConvArgs& a, int& impl, const char* who) {
    a.f16 = (impl & MVSGI_CONV_F16) != 0;
    impl &= ~MVSGI_CONV_F16;
    MVSGI_REQUIRE(!a.f16 || impl == MVSGI_CONV_BF16X3 || impl == MVSGI_CONV_BF16X3_C16 || impl == MVSGI_CONV_BF16X3_V32 || impl == MVSGI_CONV_BF16X3_D32,
                  "%s: MVSGI_CONV_F16 goes with MVSGI_CONV_BF16X3 / _C16 / _V32 (got %d)", who, impl);
    MVSGI_REQUIRE(!a.f16 || (a.Cin % 16 == 0 && a.Cout % 16 == 0), "%s: the fp16 split needs Cin, Cout multiples of 16 (got %d, %d)", who, a.Cin, a.Cout);
    return 0;
}

// the demangled name of the kernel a variant launches, as rocprofv3 prints it (the bench and the tests match substrings of it)
const char* variant_name(int v, const ConvArgs& a) {
    switch (v) {
        case V_DIRECT1: return "conv3d_direct_kernel<1>";
        case V_DIRECT4: return "conv3d_direct_kernel<4>";
        case V_HEAD: return "conv3d_head_kernel";
#define MVSGI_MFMA(V, ...) case V: return "conv3d_mfma_kernel<" #__VA_ARGS__ ">";
#define MVSGI_B3(V, K, ...) case V: return a.f16 ? "conv3d_f16x3" #K "<" #__VA_ARGS__ ">" : "conv3d_bf16x3" #K "<" #__VA_ARGS__ ">";
#include "conv3d_variants.inc"
#undef MVSGI_MFMA
#undef MVSGI_B3
    }
    return nullptr;
}

}  // namespace

extern "C" size_t mvsgi_conv3d_packed_weight_floats(int Cout, int Cin) {
    return (size_t)27 * (size_t)Cout * (size_t)Cin;
}

extern "C" size_t mvsgi_conv3d_packed_weight_bytes_bf16x3(int Cout, int Cin) {
    return (size_t)(Cin / 16) * pairs_of(3) * (size_t)(Cout / 16) * 2 * 64 * 16;
}

extern "C" int mvsgi_conv3d_pack_weights_bf16x3(const float* w_oidhw, void* w_packed, int Cout, int Cin,
                                                mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed, "mvsgi_conv3d_pack_weights_bf16x3: null pointer");
    MVSGI_REQUIRE(Cout > 0 && Cin > 0 && Cout % 16 == 0 && Cin % 16 == 0,
                  "mvsgi_conv3d_pack_weights_bf16x3: Cout=%d Cin=%d must be positive multiples of 16", Cout, Cin);
    const long long total = (long long)(Cin / 16) * pairs_of(3) * (Cout / 16) * 64;
    hipLaunchKernelGGL(pack_weights_bf16x3_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0,
                       mvsgi::as_stream(stream), w_oidhw, reinterpret_cast<bf16x8*>(w_packed), Cout, Cin, 27, false);
    return mvsgi::check_launch("mvsgi_conv3d_pack_weights_bf16x3");
}

// weights of a split kernel in either split: layout = MVSGI_CONV_BF16X3 | _C16 | _V32, optionally | MVSGI_CONV_F16 (sizes as the bf16
// packers': mvsgi_conv3d_packed_weight_bytes_bf16x3 / _c16 / _v32)
extern "C" int mvsgi_conv3d_pack_weights_split(const float* w_oidhw, void* w_packed, int Cout, int Cin, int layout,
                                               mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed, "mvsgi_conv3d_pack_weights_split: null pointer");
    const bool f16 = (layout & MVSGI_CONV_F16) != 0;
    layout &= ~MVSGI_CONV_F16;
    MVSGI_REQUIRE(Cout > 0 && Cin > 0 && Cout % 16 == 0 && Cin % 16 == 0,
                  "mvsgi_conv3d_pack_weights_split: Cout=%d Cin=%d must be positive multiples of 16", Cout, Cin);
    bf16x8* wp = reinterpret_cast<bf16x8*>(w_packed);
    if (layout == MVSGI_CONV_BF16X3) {
        const long long total = (long long)(Cin / 16) * pairs_of(3) * (Cout / 16) * 64;
        hipLaunchKernelGGL(pack_weights_bf16x3_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0, mvsgi::as_stream(stream),
                           w_oidhw, wp, Cout, Cin, 27, f16);
    } else if (layout == MVSGI_CONV_BF16X3_C16) {
        MVSGI_REQUIRE(Cout == 16, "mvsgi_conv3d_pack_weights_split: the plane layout is for Cout == 16 (got %d)", Cout);
        const int total = (Cin / 16) * 5 * 3 * 64;
        hipLaunchKernelGGL(pack_weights_bf16x3_c16_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0, mvsgi::as_stream(stream),
                           w_oidhw, wp, Cin, f16);
    } else if (layout == MVSGI_CONV_BF16X3_V32) {
        MVSGI_REQUIRE(Cout % 32 == 0, "mvsgi_conv3d_pack_weights_split: the 32x32x16 layout needs Cout %% 32 == 0 (got %d)", Cout);
        const long long total = (long long)(Cin / 16) * (Cout / 32) * 27 * 64;
        hipLaunchKernelGGL(pack_weights_bf16x3_v32_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0, mvsgi::as_stream(stream),
                           w_oidhw, wp, Cout, Cin, f16);
    } else if (layout == MVSGI_CONV_BF16X3_D32) {
        MVSGI_REQUIRE(Cin % 32 == 0, "mvsgi_conv3d_pack_weights_split: the 32-channel-slice layout needs Cin %% 32 == 0 (got %d)", Cin);
        const long long total = (long long)(Cin / 32) * (Cout / 16) * 27 * 64;
        // the layout fills 27 of the 28 k-steps the buffer is sized for (mvsgi_conv3d_packed_weight_bytes_bf16x3): the rest is zeroed,
        // so that every byte of the caller's buffer is defined by the weights alone
        const size_t used = (size_t)total * 2 * sizeof(bf16x8), all = mvsgi_conv3d_packed_weight_bytes_bf16x3(Cout, Cin);
        MVSGI_REQUIRE(used <= all && hipMemsetAsync(reinterpret_cast<char*>(w_packed) + used, 0, all - used, mvsgi::as_stream(stream)) == hipSuccess,
                      "mvsgi_conv3d_pack_weights_split: clearing the unused tail of the 32-channel-slice layout failed");
        hipLaunchKernelGGL(pack_weights_bf16x3_d32_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0, mvsgi::as_stream(stream),
                           w_oidhw, wp, Cout, Cin, f16);
    } else {
        return mvsgi::fail("mvsgi_conv3d_pack_weights_split: layout %d is not a split-kernel layout", layout);
    }
    return mvsgi::check_launch("mvsgi_conv3d_pack_weights_split");
}

extern "C" size_t mvsgi_conv3d_packed_weight_bytes_bf16x3_v32(int Cout, int Cin) {
    return (size_t)(Cin / 16) * (Cout / 32) * 27 * 2 * 64 * 16;
}

extern "C" int mvsgi_conv3d_pack_weights_bf16x3_v32(const float* w_oidhw, void* w_packed, int Cout, int Cin,
                                                    mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed, "mvsgi_conv3d_pack_weights_bf16x3_v32: null pointer");
    MVSGI_REQUIRE(Cout > 0 && Cin > 0 && Cout % 32 == 0 && Cin % 16 == 0,
                  "mvsgi_conv3d_pack_weights_bf16x3_v32: Cout=%d must be a multiple of 32, Cin=%d of 16", Cout, Cin);
    const long long total = (long long)(Cin / 16) * (Cout / 32) * 27 * 64;
    hipLaunchKernelGGL(pack_weights_bf16x3_v32_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0,
                       mvsgi::as_stream(stream), w_oidhw, reinterpret_cast<bf16x8*>(w_packed), Cout, Cin, false);
    return mvsgi::check_launch("mvsgi_conv3d_pack_weights_bf16x3_v32");
}

// 1 when mvsgi_conv3d_f32 accepts MVSGI_CONV_BF16X3_D32 for this problem (weights packed with layout MVSGI_CONV_BF16X3_D32, sized
// by mvsgi_conv3d_packed_weight_bytes_bf16x3: 27 fragments per 32 channels where the tap-pair layout has 28)
extern "C" int mvsgi_conv3d_d32_applies(int B, int Cin, int Din, int Hin, int Win, int Cout, int stride) {
    ConvArgs a{};
    static const float dummy = 0.f;
    if (fill_args(a, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, B, Cin, Din, Hin, Win, Cout, stride, 1.f))
        return 0;
    return d32_variant(a) != V_COUNT ? 1 : 0;
}

// 1 when mvsgi_conv3d_f32 / mvsgi_conv3d_up2_f32 (pass the UPSAMPLED input size) accept MVSGI_CONV_BF16X3_V32 for this problem
extern "C" int mvsgi_conv3d_v32_applies(int B, int Cin, int Din, int Hin, int Win, int Cout, int stride) {
    ConvArgs a{};
    static const float dummy = 0.f;
    if (fill_args(a, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, B, Cin, Din, Hin, Win, Cout, stride, 1.f))
        return 0;
    return v32_applies(a) ? 1 : 0;
}

extern "C" size_t mvsgi_conv3d_packed_weight_bytes_bf16x3_c16(int Cin) { return (size_t)(Cin / 16) * 5 * 3 * 2 * 64 * 16; }

extern "C" int mvsgi_conv3d_pack_weights_bf16x3_c16(const float* w_oidhw, void* w_packed, int Cin, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed, "mvsgi_conv3d_pack_weights_bf16x3_c16: null pointer");
    MVSGI_REQUIRE(Cin > 0 && Cin % 16 == 0, "mvsgi_conv3d_pack_weights_bf16x3_c16: Cin=%d must be a positive multiple of 16", Cin);
    const int total = (Cin / 16) * 5 * 3 * 64;
    hipLaunchKernelGGL(pack_weights_bf16x3_c16_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0,
                       mvsgi::as_stream(stream), w_oidhw, reinterpret_cast<bf16x8*>(w_packed), Cin, false);
    return mvsgi::check_launch("mvsgi_conv3d_pack_weights_bf16x3_c16");
}

extern "C" int mvsgi_conv3d_pack_weights_f32(const float* w_oidhw, float* w_packed, int Cout, int Cin,
                                             mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed, "mvsgi_conv3d_pack_weights_f32: null pointer");
    if (Cout == 1 && Cin > 0 && Cin % 16 == 0) {   // cost head: [27][Cin]
        hipLaunchKernelGGL(pack_head_weights_kernel, dim3((unsigned)mvsgi::cdiv(27 * Cin, 256)), dim3(256), 0,
                           mvsgi::as_stream(stream), w_oidhw, w_packed, Cin);
        return mvsgi::check_launch("mvsgi_conv3d_pack_weights_f32");
    }
    MVSGI_REQUIRE(Cout > 0 && Cin > 0 && Cout % 16 == 0 && Cin % 16 == 0,
                  "mvsgi_conv3d_pack_weights_f32: Cout=%d Cin=%d must be positive multiples of 16 (or Cout == 1)",
                  Cout, Cin);
    const long long total = (long long)(Cin / 16) * 27 * (Cout / 16) * 64;
    hipLaunchKernelGGL(pack_weights_kernel, dim3((unsigned)mvsgi::cdiv(total, 256)), dim3(256), 0,
                       mvsgi::as_stream(stream), w_oidhw, reinterpret_cast<f32x4*>(w_packed), Cout, Cin, 27);
    return mvsgi::check_launch("mvsgi_conv3d_pack_weights_f32");
}

extern "C" int mvsgi_conv3d_f32(const float* x, const float* w_oidhw, const float* w_packed, const float* scale,
                                const float* shift, const float* res, float* y, int B, int Cin, int Din, int Hin,
                                int Win, int Cout, int stride, float neg_slope, int impl, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(x && y && scale && shift, "mvsgi_conv3d_f32: null pointer");
    ConvArgs a{};
    if (fill_args(a, x, w_oidhw, w_packed, scale, shift, res, y, B, Cin, Din, Hin, Win, Cout, stride, neg_slope))
        return 1;
    if (split_flag(a, impl, "mvsgi_conv3d_f32")) return 1;
    const int v = select_variant(a, impl);
    if (v == V_COUNT) return 1;
    return launch_variant(v, a, mvsgi::as_stream(stream));
}

// the same block with the output in the split-padded format of conv3d_rs.hip (y_split zero-bordered, interior written):
// the hand-over from a streaming split-bf16 layer to the register-stationary layers
extern "C" int mvsgi_conv3d_f32_out_split_fmt(const float* x, const float* w_packed_b3, const float* scale, const float* shift,
                                              const float* res, void* y_split, int B, int Cin, int Din, int Hin, int Win, int Cout,
                                              int stride, float neg_slope, int fmt, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(fmt == 0 || fmt == MVSGI_SPLIT_F16, "mvsgi_conv3d_f32_out_split: fmt %d not in {0, MVSGI_SPLIT_F16}", fmt);
    MVSGI_REQUIRE(x && y_split && scale && shift && w_packed_b3, "mvsgi_conv3d_f32_out_split: null pointer");
    MVSGI_REQUIRE(Cin % 16 == 0 && Cout % 16 == 0, "mvsgi_conv3d_f32_out_split: Cin, Cout must be multiples of 16");
    ConvArgs a{};
    if (fill_args(a, x, nullptr, w_packed_b3, scale, shift, res, reinterpret_cast<float*>(y_split), B, Cin, Din, Hin, Win, Cout,
                  stride, neg_slope))
        return 1;
    a.y_split = static_cast<unsigned char*>(y_split);
    a.f16 = fmt != 0;      // weights (w_packed_b3 packed with MVSGI_CONV_F16) and the split-padded output in the fp16 split
    const int v = select_variant(a, MVSGI_CONV_BF16X3);
    if (v == V_COUNT) return 1;
    return launch_variant(v, a, mvsgi::as_stream(stream));
}
extern "C" int mvsgi_conv3d_f32_out_split(const float* x, const float* w_packed_b3, const float* scale, const float* shift,
                                          const float* res, void* y_split, int B, int Cin, int Din, int Hin, int Win, int Cout,
                                          int stride, float neg_slope, mvsgi_stream_t stream) {
    return mvsgi_conv3d_f32_out_split_fmt(x, w_packed_b3, scale, shift, res, y_split, B, Cin, Din, Hin, Win, Cout, stride, neg_slope, 0, stream);
}

extern "C" const char* mvsgi_conv3d_variant_f32(int B, int Cin, int Din, int Hin, int Win, int Cout, int stride,
                                                int impl) {
    ConvArgs a{};
    static const float dummy = 0.f;
    if (fill_args(a, &dummy, &dummy, &dummy, &dummy, &dummy, nullptr, nullptr, B, Cin, Din, Hin, Win, Cout, stride,
                  1.f))
        return nullptr;
    if (split_flag(a, impl, "mvsgi_conv3d_variant_f32")) return nullptr;
    const int v = select_variant(a, impl);
    return variant_name(v, a);
}

// ResizeConv3d (common_modules.py:332-355) in one launch: trilinear x2 upsample (align_corners=False) of
// x [B][Dl][Hl][Wl][Cin] fused into the producers of the split-bf16 convolution at (2Dl, 2Hl, 2Wl);
// y / res [B][2Dl][2Hl][2Wl][Cout].  w_packed is the bf16x3 layout.
extern "C" int mvsgi_conv3d_up2_f32(const float* x, const void* w_packed, int w_layout, const float* scale,
                                    const float* shift, const float* res, float* y, int B, int Cin, int Dl, int Hl,
                                    int Wl, int Cout, float neg_slope, mvsgi_stream_t stream) {
    const bool f16 = (w_layout & MVSGI_CONV_F16) != 0;
    w_layout &= ~MVSGI_CONV_F16;
    MVSGI_REQUIRE(w_layout == MVSGI_CONV_BF16X3 || (w_layout == MVSGI_CONV_BF16X3_C16 && Cout == 16) ||
                      (w_layout == MVSGI_CONV_BF16X3_V32 && Cout % 32 == 0) || (w_layout == MVSGI_CONV_BF16X3_D32 && Cin % 32 == 0),
                  "mvsgi_conv3d_up2_f32: w_layout %d not valid for Cout %d", w_layout, Cout);
    MVSGI_REQUIRE(x && y && scale && shift && w_packed, "mvsgi_conv3d_up2_f32: null pointer");
    MVSGI_REQUIRE(Dl > 0 && Hl > 0 && Wl > 0 && Dl < (1 << 20) && Hl < (1 << 20) && Wl < (1 << 20),
                  "mvsgi_conv3d_up2_f32: bad dims");
    ConvArgs a{};
    if (fill_args(a, x, nullptr, static_cast<const float*>(w_packed), scale, shift, res, y, B, Cin, 2 * Dl, 2 * Hl,
                  2 * Wl, Cout, 1, neg_slope))
        return 1;
    a.f16 = f16;
    const int v = select_variant_up2(a, w_layout);
    if (v == V_COUNT) return 1;
    return launch_variant(v, a, mvsgi::as_stream(stream));
}

// mvsgi_conv3d_up2_f32 with the output in the split-padded format (the input of the polyphase out_costs.0, csrc/conv3d_up2poly.hip)
extern "C" int mvsgi_conv3d_up2_f32_out_split(const float* x, const void* w_packed, int w_layout, const float* scale, const float* shift,
                                              const float* res, void* y_split, int B, int Cin, int Dl, int Hl, int Wl, int Cout,
                                              float neg_slope, mvsgi_stream_t stream) {
    const bool f16 = (w_layout & MVSGI_CONV_F16) != 0;      // the fp16 split: y_split then holds fp16 pairs (read by mvsgi_conv3d_head_split_f16)
    w_layout &= ~MVSGI_CONV_F16;
    MVSGI_REQUIRE(w_layout == MVSGI_CONV_BF16X3 || (w_layout == MVSGI_CONV_BF16X3_C16 && Cout == 16),
                  "mvsgi_conv3d_up2_f32_out_split: w_layout %d not valid for Cout %d", w_layout, Cout);
    MVSGI_REQUIRE(x && y_split && scale && shift && w_packed, "mvsgi_conv3d_up2_f32_out_split: null pointer");
    MVSGI_REQUIRE(Dl > 0 && Hl > 0 && Wl > 0 && Dl < (1 << 20) && Hl < (1 << 20) && Wl < (1 << 20),
                  "mvsgi_conv3d_up2_f32_out_split: bad dims");
    ConvArgs a{};
    if (fill_args(a, x, nullptr, static_cast<const float*>(w_packed), scale, shift, res, reinterpret_cast<float*>(y_split), B, Cin,
                  2 * Dl, 2 * Hl, 2 * Wl, Cout, 1, neg_slope))
        return 1;
    a.y_split = static_cast<unsigned char*>(y_split);
    a.f16 = f16;
    const int v = select_variant_up2(a, w_layout);
    if (v == V_COUNT) return 1;
    return launch_variant(v, a, mvsgi::as_stream(stream));
}

// 1 when mvsgi_conv3d_up2_f32 accepts w_layout = MVSGI_CONV_BF16X3_D32 [| MVSGI_CONV_F16] for this problem (low-resolution sizes)
extern "C" int mvsgi_conv3d_up2_d32_applies(int B, int Cin, int Dl, int Hl, int Wl, int Cout) {
    ConvArgs a{};
    static const float dummy = 0.f;
    if (Cin % 32 || Cout % 16 || Dl <= 0 || Hl <= 0 || Wl <= 0 ||
        fill_args(a, &dummy, nullptr, &dummy, &dummy, &dummy, nullptr, nullptr, B, Cin, 2 * Dl, 2 * Hl, 2 * Wl, Cout, 1, 1.f))
        return 0;
    const int base = select_variant_up2(a, MVSGI_CONV_BF16X3);
    return (base == B3U_N64 || base == B3U_N96) ? 1 : 0;
}

extern "C" const char* mvsgi_conv3d_up2_variant_f32(int B, int Cin, int Dl, int Hl, int Wl, int Cout, int w_layout) {
    ConvArgs a{};
    static const float dummy = 0.f;
    if (fill_args(a, &dummy, nullptr, &dummy, &dummy, &dummy, nullptr, nullptr, B, Cin, 2 * Dl, 2 * Hl, 2 * Wl, Cout, 1,
                  1.f))
        return nullptr;
    a.f16 = (w_layout & MVSGI_CONV_F16) != 0;
    const int v = select_variant_up2(a, w_layout & ~MVSGI_CONV_F16);
    return variant_name(v, a);
}
