// K2w: Winograd F(2x2, 3x3) over (H, W), direct over D, for the 32 -> 32 residual convolutions of UNet level 0
// (BaseConvBlk3d.forward, dsta_mvs/model/common/common_modules.py:107-115, as used by ResConvBlk3d :231-244) in the fp16 split.
//
// Why.  conv3d_rs32_kernel sits at the matrix rate the board's power cap allows: the only lever left on these
// layers is fewer MFMAs.  With 2x2 output tiles in the plane, y = A^T [ sum_kd U_kd (.) V_(d + kd - 1) ] A,  U = G g G^T (4 x 4 per
// (cout, cin, kd)),  V = B^T x B (4 x 4 per (tile, cin, plane)), and the 16 element-wise products are 16 independent
// [32 couts x 32 cins] x [32 cins x tiles] GEMMs: 16 x 3 "taps" per 4 output voxels instead of 27 per voxel -- 2.25 x fewer MFMAs.
// In the fp16 split (x = hi + lo, 11 + 11 bits; the TRANSFORMED operands are split) the result is still ~25 x closer to the
// reference than the direct convolution in the bf16 split (tools/winograd_split_emulation.py).
//
// Shape of the kernel.  A workgroup is 4 waves, one per SIMD; wave `a` owns row a of the 4 x 4 transform space: its 4 (b) x 3 (kd) x
// 2 (cout tiles) x (hi, lo) weight fragments = 192 registers stay in the accumulator half of the register file for the whole launch.
// A unit is 16 tiles in a row (2 output rows x 32 columns) marched through all D (8 or 16) planes: per plane a lane (tile n, channel
// group kg) reads the two patch rows its wave's `a` needs (B^T has two non-zeros per row) from the plane's LDS image (every global read
// is an LDS-DMA request, three planes ahead), transforms 8 channels in registers straight into the MFMA's B-operand layout (no LDS
// round trip for V) piece by piece behind the MFMAs, and issues 72 MFMAs: plane p adds U_kd V_p to the open output planes
// p + 1 - kd.  A finished output plane leaves through A^T: the (b) half inside the wave, the (a) half across the waves through a
// 16 KiB LDS exchange, after which wave (pa, q) owns output voxel (2 r + pa, 2 n + q) of every tile: scale / shift, residual,
// LeakyReLU, (split,) store.  Tensors are padded (conv3d_rs.hip's geometry: the zero border is the convolution's padding) and hold
// either fp16 pairs (split-padded) or plain fp32 records ("fp32-padded": what the layers of a chain hand to each other).
// DESIGN.md section 2, K2w, has the measurements and what it took to make hipcc emit it.
#include "common.hpp"

#include <cstring>
#ifdef MVSGI_WINO_STAMPS
#include <cstdio>
#include <cstdlib>
#endif

namespace {

#include "split_fmt.hpp"

struct WinoArgs {
    const unsigned char* x;    // padded [B][D+2][H+2][W+2][32 x 4 bytes]: fp16 pairs (split-padded) or plain fp32 (A32)
    unsigned char* y;          // the same geometry and format, or a plain fp32 [B][D][H][W][32] tensor (OUT32)
    const unsigned char* res;  // residual in x's format or nullptr
    const u32x4* wp;           // [a 4][b 4][kd 3][cout tile 2][hi | lo][64 lanes] 16-byte fragments
    const float* scale;        // (carries the inverse of the weights' pre-scaling)
    const float* shift;
    int B, D, H, W;
    float neg_slope;
    int tiles_h, groups_w, total_units;
    unsigned long long* dbg;   // -DMVSGI_WINO_STAMPS builds (ABL = 16): per wave of workgroup 0, cycles per step section
    unsigned* sat;             // the range report's words (csrc/api.cpp)
};

#include "conv3d_wino_common.hpp"

constexpr float kWinoActMax = 16376.f;     // fp32-padded activations are written clamped to this: the transform's sums of four stay inside fp16's range

namespace wn {
using namespace wino;
constexpr int NBUF = 4;                           // plane images: the staging stream runs three planes ahead of the arithmetic
constexpr int ZB = NBUF * PLANE_LDS;              // the exchange: 2 x [a 4][q 2][cout tile 2][64 lanes][16 B]
constexpr int RB = ZB + 2 * 16384;                // the residual ring
constexpr int DUMMY = RB + NRES * RES_LDS;        // where the staging requests that have no piece land (zeros)
constexpr int LDS_BYTES = DUMMY + 1024;           // 160,768
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
}  // namespace wn

// OUT32: the output is a plain fp32 channels-last tensor [B][D][H][W][32] (the hand-over to a kernel that stages fp32)
// ABL: 0, or 16 = the section stamps of a -DMVSGI_WINO_STAMPS build
// A32: activations (input, residual, padded output) are "fp32-padded" -- the split-padded geometry with plain fp32 records
//      [B][D+2][H+2][W+2][32 floats], zero border -- instead of fp16 pairs: the hand-over BETWEEN Winograd layers (their operands are
//      split after the transform anyway: no join in front of it, no split behind the epilogue: ~90 of ~420 vector instructions a step)
template <int ABL, bool RES, bool OUT32, int DEPTH, bool A32>
__global__ __launch_bounds__(256, 1) void conv3d_wino32_kernel(WinoArgs a) {
    using namespace wn;
    static_assert(DEPTH % NBUF == 0 && DEPTH % 2 == 0, "image / V pair phases of the unrolled unit");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    WN_LANE()
    const int Hp = a.H + 2, Wp = a.W + 2;
    const long long plane_bytes = (long long)Hp * Wp * 128;
    const long long frame_bytes = (a.D + 2) * plane_bytes;
    const long long total_bytes = frame_bytes * a.B;
    WN_ROLE()

    WN_WEIGHTS(wv)
    const f32x4 esc_[2] = {*reinterpret_cast<const f32x4*>(a.scale + kg * 4), *reinterpret_cast<const f32x4*>(a.scale + 16 + kg * 4)};
    const f32x4 esh_[2] = {*reinterpret_cast<const f32x4*>(a.shift + kg * 4), *reinterpret_cast<const f32x4*>(a.shift + 16 + kg * 4)};
    __builtin_amdgcn_sched_barrier(0);

    const int lane_out = (2 * n) * 128 + (kg >> 1) * 16 + (kg & 1) * 8;       // this lane's 8-byte hi piece of an output voxel's slice 0
    const int lane_out32 = (2 * n) * 128 + kg * 16;                           // (fp32 output: its 16 bytes = couts 4 kg .. 4 kg + 3 of the voxel's first 16)
    const long long oplane_bytes = (long long)a.H * a.W * 128;
    const int rd0 = WN_FRAG_RD(i0);
    const int rd1 = WN_FRAG_RD(i1);
    WN_PLANE_PLAN(A32)
    unsigned rvoff[RDPW];
#pragma unroll
    for (int k = 0; k < RDPW; ++k) {
        WN_RES_SLOT(k)
        rvoff[k] = (vox < 64 && piece < 8) ? (unsigned)(((vox >> 5) * Wp + (vox & 31)) * 128 + piece * 16) : NOREC;
    }
    // the epilogue's residual reads: voxel (row pa, column 2 n + q), this lane's 8 bytes of slice 0's hi piece
    const int rrd = A32 ? ((pa * 32 + 2 * n + q) * RPITCH + kg) * 16                      // (fp32 records: 16 bytes = couts 4 kg .. 4 kg + 3 of a cout tile)
                        : ((pa * 32 + 2 * n + q) * RPITCH + (kg >> 1)) * 16 + (kg & 1) * 8;

    f32x4 Y[3][4][2];
    u32x4 vh[2][4], vl[2][4];      // V of the plane being multiplied | of the next one (written while the first is read)
    u32x4 raw[2][4][2];            // [patch row i0 | i1][column][hi | lo] of the plane being transformed
    float T[2][4];                 // h-pass of one channel pair: [lo | hi half][column]

    const int G = gridDim.x;
    // The walk: side by side through this XCD's share of the unit space (ids ubase + k * ustep), or blockIdx + k * G
    const int T_ = a.total_units;
    int ubase = (int)blockIdx.x, ustep = G, nmine = (T_ - (int)blockIdx.x + G - 1) / G;
    if ((G & 7) == 0 && T_ >= G) {
        const int x = (int)blockIdx.x & 7, i = (int)blockIdx.x >> 3;
        int lo, cnt;
        wino_xcd_share(T_, x, lo, cnt);
        ustep = G >> 3;
        ubase = lo + i;
        nmine = i < cnt ? (lo + cnt - ubase + ustep - 1) / ustep : 0;
    }
    if (nmine == 0) return;         // (the whole workgroup, before anything was requested)

// Staging: input plane (P + 3) of the plane stream -- of this unit, or of the next one from P = D - 3 on -- goes to image (P + 3) % 4
// (D % 4 == 0: the images keep their phase over units); the residual records of plane P to image `ri` of a ring of three.
#define WN_DMA_ISSUE(P3, K0, K1)                                                                            \
    _Pragma("unroll") for (int k_ = (K0); k_ < (K1); ++k_)                                                  \
        LDS_DMA16((P3) < DEPTH ? dsc : dsc_next, lds + (wv + 4 * k_ < NDMA ? ((P3) % NBUF) * PLANE_LDS + (wv + 4 * k_) * 1024 : DUMMY), \
                  voff[k_], (unsigned)(((P3) % DEPTH + 1) * plane_bytes), 0);
#define WN_RES_DMA(IMG, OPLANE)                                                                             \
    {                                                                                                       \
        const unsigned so_ = (unsigned)(((OPLANE) + 1) * plane_bytes);                                      \
        _Pragma("unroll") for (int k_ = 0; k_ < RDPW; ++k_)                                                 \
            LDS_DMA16(rdsc, lds + RB + (IMG) * RES_LDS + (wv + 4 * k_) * 1024, rvoff[k_], so_, 0);          \
    }
// One piece of the transform raw -> V[VN]: the h-pass of fp32 records is one fma per channel; on fp16 pairs the w-pass's sums are
// clamped to fp16's range; piece 17 carries the step's staging requests (WN_DPIECE)
#define WN_TPIECE(M, VN)                                                                                    \
    {                                                                                                       \
        constexpr int d_ = (M) / 18, r_ = (M) % 18;                                                         \
        if constexpr (r_ < 8) {                                                                             \
            constexpr int j_ = r_ >> 1;                                                                     \
            if constexpr (A32) {    /* channel 2 d_ + (r_ & 1) of the lane's eight: one fma */            \
                constexpr int e_ = (d_ & 1) * 2 + (r_ & 1);                                                 \
                T[r_ & 1][j_] = __builtin_fmaf(__builtin_bit_cast(float, raw[1][j_][d_ >> 1][e_] | 0u), sgn, \
                                               __builtin_bit_cast(float, raw[0][j_][d_ >> 1][e_] | 0u));    \
            } else {                                                                                        \
                WN_HPASS(r_, j_, d_)                                                                        \
            }                                                                                               \
        } else if constexpr (r_ < 16) {                                                                     \
            constexpr int b_ = (r_ - 8) >> 1;                                                               \
            if constexpr (((r_ - 8) & 1) == 0) {                                                            \
                WN_WPASS(b_)                                                                                \
                if constexpr (!A32) {                       /* (fp32-padded records arrive clamped to +-16376: their sums of four cannot leave fp16's range) */ \
                    X0 = sf_clamp<true>(X0);                                                                \
                    X1 = sf_clamp<true>(X1);                                                                \
                    satm = sf_sat_acc(satm, X0, X1);        /* range report: a sum of four left fp16's range */ \
                }                                                                                           \
                if constexpr (b_ > 0) { WN_SPLIT_LO(VN, b_ - 1, d_) }                                       \
            } else {                                                                                        \
                WN_SPLIT_HI(VN, b_, d_)                                                                     \
            }                                                                                               \
        } else if constexpr (r_ == 16) {                                                                    \
            WN_SPLIT_LO(VN, 3, d_)                                                                          \
        }                                                                                                   \
    }
#define WN_DPIECE(M, P)                                                                                     \
    if constexpr ((M) == 17) { if constexpr (RES) { WN_RES_DMA(ri, P) } }                                   \
    else if constexpr ((M) == 35) { WN_DMA_ISSUE((P) + 3, 0, 2) }                                           \
    else if constexpr ((M) == 53) { WN_DMA_ISSUE((P) + 3, 2, 4) }                                           \
    else if constexpr ((M) == 71) { WN_DMA_ISSUE((P) + 3, 4, 6) }
#define WN_STAMP(K)                                                                                         \
    if constexpr (ABL & 16) {                                                                               \
        unsigned long long t_;                                                                              \
        asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t_)::"memory");                         \
        tsum[K] += t_ - tlast;                                                                              \
        tlast = t_;                                                                                         \
    }
// the exchange's sums and the residual of this wave's output voxel of every tile
#define WN_EPI_READS(ZIMG)                                                                                  \
    WN_EXCHANGE_READS(ZIMG)                                                                                 \
    u32x2 rh_[2] = {u32x2{0u, 0u}, u32x2{0u, 0u}}, rl_[2] = {u32x2{0u, 0u}, u32x2{0u, 0u}};                 \
    f32x4 rf_[2] = {f32x4{0.f, 0.f, 0.f, 0.f}, f32x4{0.f, 0.f, 0.f, 0.f}};                                 \
    if constexpr (RES) {                                                                                    \
        _Pragma("unroll") for (int c_ = 0; c_ < 2; ++c_) {                                                  \
            if constexpr (A32) {                                                                            \
                rf_[c_] = *reinterpret_cast<const f32x4*>(rim_ + rrd + c_ * 64);                            \
            } else {                                                                                        \
                rh_[c_] = *reinterpret_cast<const u32x2*>(rim_ + rrd + c_ * 64);                            \
                rl_[c_] = *reinterpret_cast<const u32x2*>(rim_ + rrd + c_ * 64 + 32);                       \
            }                                                                                               \
        }                                                                                                   \
    }
#define WN_EPILOGUE(O)                                                                                      \
    _Pragma("unroll") for (int c_ = 0; c_ < 2; ++c_) {                                                      \
        f32x4 t_ = zz_[c_][0] + osg * (zz_[c_][1] + zz_[c_][2]);                                            \
        t_ = t_ * esc_[c_] + esh_[c_];                                                                      \
        if constexpr (RES && A32) {                                                                         \
            t_ = t_ + rf_[c_];                                                                              \
        } else if constexpr (RES) {                                                                         \
            t_[0] = mix_add_lo(rl_[c_][0], mix_add_lo(rh_[c_][0], t_[0]));                                  \
            t_[1] = mix_add_hi(rl_[c_][0], mix_add_hi(rh_[c_][0], t_[1]));                                  \
            t_[2] = mix_add_lo(rl_[c_][1], mix_add_lo(rh_[c_][1], t_[2]));                                  \
            t_[3] = mix_add_hi(rl_[c_][1], mix_add_hi(rh_[c_][1], t_[3]));                                  \
        }                                                                                                   \
        if constexpr (A32 && !OUT32) {      /* LeakyReLU, THEN the fp32-padded format's range (clamping inside the activation's med3 let \
                                               t * neg_slope > 16376 through: any t > 16376 at slope 1, t > 1.6e6 at 0.01) + the range report */ \
            _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_)                                                \
                t_[e_] = __builtin_amdgcn_fmed3f(__builtin_fmaxf(t_[e_], t_[e_] * a.neg_slope), -kWinoActMax, kWinoActMax); \
            satm = sf_sat_acc(sf_sat_acc(satm, t_[0], t_[1]), t_[2], t_[3]);                                \
        } else {                                                                                            \
            _Pragma("unroll") for (int e_ = 0; e_ < 4; ++e_) t_[e_] = __builtin_fmaxf(t_[e_], t_[e_] * a.neg_slope); \
        }                                                                                                   \
        if constexpr (OUT32) {                                                                              \
            *reinterpret_cast<f32x4*>(yb + (long long)(O) * oplane_bytes + lane_out32 + c_ * 64) = t_;      \
        } else if constexpr (A32) {                                                                         \
            *reinterpret_cast<f32x4*>(yb + (long long)((O) + 1) * plane_bytes + lane_out32 + c_ * 64) = t_; \
        } else {                                                                                            \
            unsigned h0_, l0_, h1_, l1_;                                                                    \
            split_pair(t_[0], t_[1], h0_, l0_, satm);                                                       \
            split_pair(t_[2], t_[3], h1_, l1_, satm);                                                       \
            unsigned char* q_ = yb + (long long)((O) + 1) * plane_bytes + lane_out + c_ * 64;               \
            *reinterpret_cast<u32x2*>(q_) = u32x2{h0_, h1_};                                                \
            *reinterpret_cast<u32x2*>(q_ + 32) = u32x2{l0_, l1_};                                           \
        }                                                                                                   \
    }
// one MFMA and the pieces that ride behind it
#define WN_SLOT(M, P, SI, SM, SF, VB)                                                                       \
    {                                                                                                       \
        WN_SLOT_MFMA(M, P, SI, SM, SF, VB)                                                                  \
        WN_TPIECE(M, (VB) ^ 1)                                                                              \
        WN_DPIECE(M, P)                                                                                     \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
    }

// One plane step, P = 0 .. D - 1.  V of plane P in vh / vl[VB]; raw holds the NEXT plane of the stream (the next unit's first after
// P = D - 1), whose V goes to vh / vl[VB ^ 1] piece by piece behind this plane's MFMAs.  Slot SF gets its last contribution: it leaves
// through the exchange at the end of the step.
#define WN_STEP(P, SI, SM, SF, VB)                                                                          \
    {                                                                                                       \
        WN_STAMP(0)                                                                                         \
        /* every global read of the kernel is an LDS-DMA request waited for by hand (hipcc's vmcnt bookkeeping does not count them: \
           its own waits for ordinary loads would drain the stream).  Per step, in this order: the residual records of plane P (for the \
           epilogue ONE step later -- the next step's, or the unit's closing one), then the input plane three steps ahead */ \
        unsigned char* rim_ = lds + RB + rprev * RES_LDS;                                                   \
        asm volatile("s_nop 1");                                                                            \
        {                                                                                                   \
            float X0 = 0.f, X1 = 0.f, L0 = 0.f, L1 = 0.f;                                                   \
            WN_REP72(WN_SLOT, P, SI, SM, SF, VB)                                                            \
        }                                                                                                   \
        WN_PAD()                                                                                            \
        WN_STAMP(2)                                                                                         \
        if constexpr ((P) > 0) { WN_OUT_WRITE(SF, ((P) - 1) & 1) }                                          \
        /* everything older than this step's requests has landed: the residual asked for a step ago, the image of the plane after the next */ \
        if constexpr (RES) asm volatile("s_waitcnt vmcnt(9) lgkmcnt(0)" ::: "memory");                      \
        else asm volatile("s_waitcnt vmcnt(6) lgkmcnt(0)" ::: "memory");                                    \
        WN_STAMP(3)                                                                                         \
        __builtin_amdgcn_s_barrier();                                                                       \
        WN_STAMP(4)                                                                                         \
        if constexpr ((P) > 0) {                                                                            \
            WN_EPI_READS(((P) - 1) & 1)                                                                     \
            WN_EPILOGUE((P) - 1)                                                                            \
        }                                                                                                   \
        __builtin_amdgcn_sched_barrier(0);                                                                  \
        WN_READ(((P) + 2) % NBUF)                       /* the plane after the next: its latency under the next step's start */ \
        WN_STAMP(5)                                                                                         \
        rprev = ri;                                                                                         \
        ri = ri == NRES - 1 ? 0 : ri + 1;                                                                   \
    }
// the unit's last output plane (its slot got the last contribution in step D - 1: plane D is the zero border)
#define WN_FINISH(SF)                                                                                       \
    {                                                                                                       \
        unsigned char* rim_ = lds + RB + rprev * RES_LDS;                                                   \
        WN_OUT_WRITE(SF, (DEPTH - 1) & 1)                                                                   \
        /* its residual was requested in the step before, in front of that step's input plane (6 requests) and output stores (4, or 2 fp32) */ \
        if constexpr (OUT32 || A32) asm volatile("s_waitcnt vmcnt(8) lgkmcnt(0)" ::: "memory");             \
        else asm volatile("s_waitcnt vmcnt(10) lgkmcnt(0)" ::: "memory");                                   \
        __builtin_amdgcn_s_barrier();                                                                       \
        WN_EPI_READS((DEPTH - 1) & 1)                                                                       \
        WN_EPILOGUE(DEPTH - 1)                                                                              \
    }


    unsigned long long tsum[8] = {0, 0, 0, 0, 0, 0, 0, 0}, tlast = 0;
    if constexpr (ABL & 16) asm volatile("s_memtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(tlast)::"memory");
    int ri = 0, rprev = 0;                             // residual image to request into / requested a step ago
    float satm = 0.f;                                  // running maximum |clamped value| (range report, csrc/split_fmt.hpp)
    auto dsc = WN_DESC(ubase, true);
    auto dsc_next = dsc;
    // the first three planes of the stream; V of the first; raw of the second
    WN_DMA_ISSUE(0, 0, DPW)
    WN_DMA_ISSUE(1, 0, DPW)
    WN_DMA_ISSUE(2, 0, DPW)
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();
    WN_READ(0)
    {
        float X0 = 0.f, X1 = 0.f, L0 = 0.f, L1 = 0.f;
        WN_REP72(WN_TPIECE, 0)
    }
    WN_READ(1)
    for (int k = 0; k < nmine; ++k) {
        const int u = ubase + k * ustep;
        const int c = u % a.groups_w;
        const int t = u / a.groups_w;
        const int r = t % a.tiles_h;
        const int b = t / a.tiles_h;
        // this wave's output voxel origin (padded row 2 r + pa + 1, column 32 c + q + 1)
        unsigned char* yb = OUT32 ? a.y + b * (a.D * oplane_bytes) + ((long long)(2 * r + pa) * a.W + 32 * c + q) * 128
                                  : a.y + b * frame_bytes + ((long long)(2 * r + pa + 1) * Wp + 32 * c + q + 1) * 128;
        const long long roff = b * frame_bytes + ((long long)(2 * r + 1) * Wp + 32 * c + 1) * 128;      // the unit's output rows in the residual tensor
        const long long rleft = total_bytes - roff;
        const auto rdsc = window_desc((RES ? a.res : a.x) + roff, 0, rleft);
        dsc_next = WN_DESC(u + ustep, k + 1 < nmine);
        WN_STEPP(WN_STEP, 0) WN_STEPP(WN_STEP, 1) WN_STEPP(WN_STEP, 2) WN_STEPP(WN_STEP, 3) WN_STEPP(WN_STEP, 4) WN_STEPP(WN_STEP, 5) WN_STEPP(WN_STEP, 6) WN_STEPP(WN_STEP, 7)
        if constexpr (DEPTH == 16) {
            WN_STEPP(WN_STEP, 8) WN_STEPP(WN_STEP, 9) WN_STEPP(WN_STEP, 10) WN_STEPP(WN_STEP, 11) WN_STEPP(WN_STEP, 12) WN_STEPP(WN_STEP, 13) WN_STEPP(WN_STEP, 14) WN_STEPP(WN_STEP, 15)
        }
        WN_FINISH((DEPTH - 1) % 3)
        dsc = dsc_next;
    }
    // fp32-padded records are clamped to +-16376 where they are written; on fp16 pairs the transform's sums and the output to +-65504
    if constexpr (!(A32 && OUT32)) sf_sat_report(a.sat, kSatWino, satm, A32 ? kWinoActMax : kF16Max);
    if constexpr (ABL & 16) {
        if (blockIdx.x == 0 && lane == 0 && a.dbg)
            for (int k = 0; k < 8; ++k) a.dbg[wv * 8 + k] = tsum[k];
    }
}

template <int ABL, bool RES, bool OUT32, int DEPTH, bool A32>
int wino_launch5(const WinoArgs& a, long long units, hipStream_t st) {
    static mvsgi::PersistentGeom geo_cache[mvsgi::kMaxDevices] = {};
    mvsgi::PersistentGeom geo;
    if (mvsgi::persistent_geometry(conv3d_wino32_kernel<ABL, RES, OUT32, DEPTH, A32>, 256, wn::LDS_BYTES, 1, geo_cache, "conv3d(winograd)", geo)) return 1;
    const unsigned grid = (unsigned)(units < geo.cus ? units : geo.cus);
    hipLaunchKernelGGL((conv3d_wino32_kernel<ABL, RES, OUT32, DEPTH, A32>), dim3(grid), dim3(256), wn::LDS_BYTES, st, a);
    return 0;
}
template <int ABL, int DEPTH, bool A32>
int wino_launch3(const WinoArgs& a, long long units, bool out32, hipStream_t st) {
    if (out32) return a.res ? wino_launch5<ABL, true, true, DEPTH, A32>(a, units, st) : wino_launch5<ABL, false, true, DEPTH, A32>(a, units, st);
    return a.res ? wino_launch5<ABL, true, false, DEPTH, A32>(a, units, st) : wino_launch5<ABL, false, false, DEPTH, A32>(a, units, st);
}
template <int ABL>
int wino_launch(const WinoArgs& a, long long units, bool out32, bool act32, hipStream_t st) {
    if (act32) return a.D == 16 ? wino_launch3<ABL, 16, true>(a, units, out32, st) : wino_launch3<ABL, 8, true>(a, units, out32, st);
    return a.D == 16 ? wino_launch3<ABL, 16, false>(a, units, out32, st) : wino_launch3<ABL, 8, false>(a, units, out32, st);
}

// [32][32][27] -> the packed weights (conv3d_wino_common.hpp, in fp32 arithmetic); unscale[cout] = 2^-k.
// One workgroup per cout: thread (ci = t & 31, group = t >> 5) computes 6 of the 48 (a, b, kd).
__global__ __launch_bounds__(256) void wino_pack_weights_kernel(const float* __restrict__ w, unsigned short* __restrict__ wp, float* __restrict__ unscale) {
    __shared__ float red[256];
    const int co = blockIdx.x, t = threadIdx.x, ci = t & 31, grp = t >> 5;
    constexpr float Gm[4][3] = WINO_G;
    const float* g = w + ((long long)co * 32 + ci) * 27;
    float u[6], amax = 0.f;
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int e = grp * 6 + i, kd = e % 3, ab = e / 3, a_ = ab >> 2, b_ = ab & 3;
        float acc = 0.f;
        for (int kh = 0; kh < 3; ++kh)
            for (int kw = 0; kw < 3; ++kw) acc += Gm[a_][kh] * Gm[b_][kw] * g[kd * 9 + kh * 3 + kw];
        u[i] = acc;
        amax = fmaxf(amax, fabsf(acc));
    }
    red[t] = amax;
    __syncthreads();
    for (int sft = 128; sft > 0; sft >>= 1) {
        if (t < sft) red[t] = fmaxf(red[t], red[t + sft]);
        __syncthreads();
    }
    amax = red[0];
    int k = 0;
    if (amax > 0.f) {
        int e;
        const float m = frexpf(amax, &e);
        k = wino_prescale_exp(m, e);
    }
    const float up = ldexpf(1.f, k);
    if (t == 0) unscale[co] = ldexpf(1.f, -k);
#pragma unroll
    for (int i = 0; i < 6; ++i) {
        const int e = grp * 6 + i, kd = e % 3, ab = e / 3;
        unsigned short hi, lo;
        sf_split_weight(u[i] * up, true, hi, lo);
        wino_weight_store(wp, ab, kd, co, ci, hi, lo);
    }
}

}  // namespace

extern "C" {

size_t mvsgi_conv3d_wino32_packed_weight_bytes(void) { return (size_t)4 * 4 * 3 * 2 * 2 * 64 * 16; }

int mvsgi_conv3d_wino32_applies(int Cin, int Cout, int D, int H, int W, int stride, float neg_slope) {
    return Cin == 32 && Cout == 32 && stride == 1 && (D == 8 || D == 16) && H > 0 && W > 0 && H % 2 == 0 && W % 32 == 0 && neg_slope >= 0.f && neg_slope <= 1.f &&
           (long long)(D + 2) * (H + 2) * (W + 2) * 128 < (1ll << 31);
}

int mvsgi_conv3d_wino32_pack_weights(const float* w_oidhw, void* w_packed, float* unscale, void* stream) {
    MVSGI_REQUIRE(w_oidhw && w_packed && unscale, "mvsgi_conv3d_wino32_pack_weights: null pointer");
    hipLaunchKernelGGL(wino_pack_weights_kernel, dim3(32), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), w_oidhw,
                       reinterpret_cast<unsigned short*>(w_packed), unscale);
    return mvsgi::check_launch("mvsgi_conv3d_wino32_pack_weights");
}

int mvsgi_conv3d_wino32_f16(const void* x_split, const void* w_packed, const float* scale, const float* shift, const void* res_split,
                            void* y, int y_is_f32, int act_f32p, int B, int D, int H, int W, float neg_slope, void* stream) {
    MVSGI_REQUIRE(x_split && w_packed && scale && shift && y, "mvsgi_conv3d_wino32_f16: null pointer");
    MVSGI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mvsgi_conv3d_wino32_f16: bad dims");
    MVSGI_REQUIRE((D == 8 || D == 16) && H % 2 == 0 && W % 32 == 0,
                  "mvsgi_conv3d_wino32_f16: needs D == 8 or 16, H %% 2 == 0 and W %% 32 == 0 (got %d, %d, %d)", D, H, W);
    MVSGI_REQUIRE(neg_slope >= 0.f && neg_slope <= 1.f, "mvsgi_conv3d_wino32_f16: neg_slope outside [0, 1]");
    MVSGI_REQUIRE((long long)B * (D + 2) * (H + 2) * (W + 2) * 128 < (1ll << 40), "mvsgi_conv3d_wino32_f16: tensor too large");
    MVSGI_REQUIRE((long long)(D + 2) * (H + 2) * (W + 2) * 128 < (1ll << 31), "mvsgi_conv3d_wino32_f16: frame too large for 32-bit plane offsets");
    WinoArgs a;
    memset(&a, 0, sizeof(a));
    a.x = reinterpret_cast<const unsigned char*>(x_split);
    a.y = reinterpret_cast<unsigned char*>(y);
    a.res = reinterpret_cast<const unsigned char*>(res_split);
    a.wp = reinterpret_cast<const u32x4*>(w_packed);
    a.scale = scale;
    a.shift = shift;
    a.B = B; a.D = D; a.H = H; a.W = W;
    a.neg_slope = neg_slope;
    a.tiles_h = H / 2;
    a.groups_w = W / 32;
    const long long units = (long long)B * a.tiles_h * a.groups_w;
    MVSGI_REQUIRE(units < (1ll << 31), "mvsgi_conv3d_wino32_f16: too many units");
    a.total_units = (int)units;
    MVSGI_SAT_WORDS(sat_words_);
    a.sat = sat_words_;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
#ifdef MVSGI_WINO_STAMPS      // diagnostic build: cycles per step section of workgroup 0 (tools/wino_probe.py)
    if (getenv("MVSGI_WINO_STAMP")) {
        static unsigned long long* dbg = nullptr;
        if (!dbg) (void)hipMalloc(&dbg, 32 * 8);
        a.dbg = dbg;
        if (wino_launch<16>(a, units, y_is_f32 != 0, act_f32p != 0, st)) return 1;
        (void)hipDeviceSynchronize();
        unsigned long long h[32];
        (void)hipMemcpy(h, dbg, sizeof(h), hipMemcpyDeviceToHost);
        for (int w = 0; w < 4; ++w) {
            fprintf(stderr, "wave %d:", w);
            for (int k = 0; k < 7; ++k) fprintf(stderr, " %llu", h[w * 8 + k]);
            fprintf(stderr, "\n");
        }
        return mvsgi::check_launch("mvsgi_conv3d_wino32_f16");
    }
#endif
    if (wino_launch<0>(a, units, y_is_f32 != 0, act_f32p != 0, st)) return 1;
    return mvsgi::check_launch("mvsgi_conv3d_wino32_f16");
}

}  // extern "C"
