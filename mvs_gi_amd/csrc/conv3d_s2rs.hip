// K2g: the regulator's first stride-2 convolution (UNetDownBlk.first of level 0: BaseConvBlk3d 16 -> 32 channels, 3x3x3,
// stride 2, padding 1 + BatchNorm + LeakyReLU; dsta_mvs/model/cost_volume_regulator/unet_regulator.py:286-303,
// common/common_modules.py:107-115) on pre-split activations.
//
// Why its own kernel.  The layer reads the full-resolution 16-channel volume once (1.68 GB per 64 frames of G16V) and writes
// an eighth of the voxels: 3 flop per byte, HBM-bound by a wide margin (all its MFMAs are 130 us of matrix-core time).  The
// streaming kernel (conv3d_bf16x3.hpp) spends its time in producer waves that fetch fp32 voxels into registers, split them and
// write them to LDS: 707 us, 2.96 TB/s.  Here the input arrives ALREADY SPLIT (post_vol's epilogue, csrc/conv3d_rs.hip, writes
// the split-padded format), so staging is a pure copy on the LDS-DMA path with a whole brick in flight per CU at all times:
//   * a workgroup = 4 waves, persistent, double-buffered windows: the DMA of brick u + 1 is issued before the MFMAs of brick u;
//   * the window of a brick of 4 x 16 outputs of one output plane is 3 x 9 x 33 input voxels, de-interleaved into even and odd
//     columns on the way into LDS (presplit_common.hpp: PsS2Window, shared with the extractor's stride-2 layer in
//     resblock2d_rs.hip, as are the walk, the activation, the split epilogue and the weight packer);
//   * LDS voxels are 32 B in a HI and 32 B in a LO region; a ds_read_b128 lane group reads 8 voxels' channels 0-7 and 8 OTHER
//     voxels' channels 8-15 of the same tap (k = tap-of-pair x 16 + channel): conflict-free at any pitch;
//   * wave w owns cout tile w & 1 of the brick's output rows 2 (w >> 1), + 1 with that tile's weights (14 tap pairs x hi | lo =
//     112 registers) resident for the whole launch; BatchNorm's scale is folded into the weights, its shift is the
//     accumulators' start value;
//   * the epilogue writes the 32-channel split-padded format the register-stationary 32 -> 32 kernel reads (conv3d_rs.hip).
#include "common.hpp"

#include <cstdlib>

namespace {

#include "presplit_common.hpp"

constexpr int kS2StAux = 0;     // cache policy bits of the output stores (2 = nt: measured neutral to slower)

// (windows and LDS-DMA pieces go through the FUNCTIONS of device_prims.hpp, window_desc / lds_dma16: in the kernel TEMPLATE below the
// builtins' operands would be value-dependent, and hipcc's host pass then drops the kernel's stub without a diagnostic)
__device__ __forceinline__ void s2_store16(const u32x4 v, const __amdgpu_buffer_rsrc_t dsc, const unsigned voff, const int soff) {
    __builtin_amdgcn_raw_buffer_store_b128(v, dsc, voff, soff, kS2StAux);
}

namespace s2 {
constexpr int TH = 4;                          // output rows of a brick: 4 rows x 16 outputs of one output plane
constexpr int kTaps = 27, kPairs = 14;         // 27 taps in pairs (the 28th slot: zero weights)
using Win = PsS2Window<3, 2 * TH + 1>;         // 3 planes x 9 rows x 33 columns
constexpr int TW = Win::TW, IW = Win::IW;
constexpr int LDS_BYTES = 2 * Win::IMG;        // two windows: one workgroup per CU
static_assert(LDS_BYTES <= 160 * 1024, "LDS budget");
static_assert(Win::DPW == kPairs, "one DMA piece of the next window per tap pair");
}  // namespace s2

struct S2Args {
    const unsigned char* x;    // split-padded [B][D+2][H+2][W+2][64 B] (16 channels)
    unsigned char* y;          // split-padded [B][Do+2][Ho+2][Wo+2][128 B] (32 channels)
    const bf16x8* wp;
    const float* shift;        // [32]
    int B, D, H, W, Do, Ho, Wo;
    int tiles_h, tiles_w, total_units;
    float neg_slope;
    float unscale;             // fp16 split: the packed weights and `shift` carry a power of two 1 / unscale (so that the weights' lo parts
                               // are normal fp16 numbers); the accumulators are multiplied by it in front of the activation
    unsigned* sat;             // the range report's words (csrc/api.cpp)
};

// One workgroup per CU with two windows, the window of brick u + 1 in flight under brick u.  (ONE window per workgroup and two
// workgroups per CU -- the next window requested when the workgroup is done with the current one, the partner workgroup's request
// in flight meanwhile, ~1.6 windows in flight per CU instead of 1 -- measured the same within 2 %, 565 vs 577 us per 64 frames: the
// kernel is not short of requests in flight.)
// O32P: the output is "fp32-padded" -- the split-padded geometry with plain fp32 records -- for a Winograd-form level 0 behind it
// (csrc/conv3d_wino.hip: its layers split their operands behind the transform, a pre-split input buys them nothing)
template <bool F16 = false, bool O32P = false>
__global__ __launch_bounds__(256, 1) void conv3d_s2rs_kernel(S2Args a) {
    using namespace s2;
    constexpr int IHt = Win::IHt, DPW = Win::DPW, REGION = Win::REGION, IMG = Win::IMG;
    constexpr int TPW = TH / 2;                       // tiles (output rows) per wave: waves 2 q, 2 q + 1 share rows q TPW ..
    static_assert(TH % 2 == 0, "two waves per pair of cout tiles");
    extern __shared__ __attribute__((aligned(16))) unsigned char lds[];
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int ct = wave & 1, t0 = (wave >> 1) * TPW;
    const int col = lane & 15, kg = lane >> 4;
    const int Hp = a.H + 2, Wp = a.W + 2, Hop = a.Ho + 2, Wop = a.Wo + 2;
    const long long frame_bytes = (long long)(a.D + 2) * Hp * Wp * 64, total_bytes = frame_bytes * a.B;
    const long long oframe_bytes = (long long)(a.Do + 2) * Hop * Wop * 128, ototal_bytes = oframe_bytes * a.B;
    PS_WALK(a.total_units, nmine, id0, idstep)

    // ---- this wave's weights (cout tile ct), resident ----
    bf16x8 wh[kPairs], wl[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        wh[p] = a.wp[((ct * kPairs + p) * 2) * 64 + lane];
        wl[p] = a.wp[((ct * kPairs + p) * 2 + 1) * 64 + lane];
    }
    const f32x4 bsh = *reinterpret_cast<const f32x4*>(a.shift + ct * 16 + kg * 4);

    // ---- fragment read addresses (window 0, HI region): tile i of this wave = output row t0 + i, outputs ow = col;
    //      lane (col, kg) reads chunk kg & 1 of voxel (plane kd, row 2 (t0 + i) + kh, column 2 col + kw) under tap 2 p + (kg >> 1) ----
    int rbp[kPairs];
#pragma unroll
    for (int p = 0; p < kPairs; ++p) {
        PS_PAIR_TAP(t, p, kg, kTaps)
        const int kd = t / 9, kh = (t / 3) % 3, kw = t % 3;
        rbp[p] = (((kd * IHt + 2 * t0 + kh) * IW) + PS_S2_SLOT(Win, kw, col)) * 32 + (kg & 1) * 16;
    }
    // ---- DMA plan: piece q = wave + 4 m fills LDS bytes [q * 1024, +1024) of a window ----
    unsigned voff[DPW];
#pragma unroll
    for (int m = 0; m < DPW; ++m) voff[m] = Win::voff(wave + 4 * m, lane, Hp, Wp);
    // ---- output: this lane's 16 bytes of voxel (row t0 + i, ow = col) of slice ct: lanes kg and kg ^ 1 trade halves ----
    unsigned vst = O32P ? (unsigned)((t0 * Wop + col) * 128 + ct * 64 + kg * 16)
                        : (unsigned)((t0 * Wop + col) * 128 + ct * 64 + (kg & 1) * 32 + (kg >> 1) * 16);

    // brick order (b, oh, od, ow), ow fastest: the bricks stacked along D share one of their three input planes and follow each
    // other within one XCD round
#define S2_DECODE(ID, B_, OD, OH, OW)                            \
    {                                                            \
        int t_ = (ID);                                           \
        OW = (t_ % a.tiles_w) * TW;                              \
        t_ /= a.tiles_w;                                         \
        OD = t_ % a.Do;                                          \
        t_ /= a.Do;                                              \
        OH = (t_ % a.tiles_h) * TH;                              \
        B_ = t_ / a.tiles_h;                                     \
    }
    // window of brick (b, od, oh0, ow0): origin = padded input voxel (2 od, 2 oh0, 2 ow0)
#define S2_DESC(B_, OD, OH, OW) \
    window_desc(a.x, (long long)(B_) * frame_bytes + (((long long)(2 * (OD)) * Hp + 2 * (OH)) * Wp + 2 * (OW)) * 64, total_bytes)
    int b_, od, oh0, ow0;
    S2_DECODE(id0, b_, od, oh0, ow0)
    {
        const auto dsc_ = S2_DESC(b_, od, oh0, ow0);
#pragma unroll
        for (int m = 0; m < DPW; ++m) ps_dma_piece(dsc_, lds, wave, m, voff[m]);
    }
    float satm = 0.f;          // fp16 split: running maximum |value written| (range report)
    for (int u = 0; u < nmine; ++u) {
        int nb, nod, noh, now;
        S2_DECODE(id0 + (u + 1 < nmine ? u + 1 : u) * idstep, nb, nod, noh, now)
        const int img = (u & 1) * IMG;
        asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_barrier" ::: "memory");    // window u landed; every wave is done with window u - 1
        // The window of brick u + 1 lands under this brick's MFMAs and the next wait.  Its pieces go out one per tap pair
        // (DPW == kPairs) instead of in a burst behind the barrier, where the workgroup's 56 requests queue up in the CU's address
        // path in front of the MFMAs (the burst was measured at 559 vs 486 us per 64 frames).
        // Four different issue points inside a pair for the four waves instead of one: 501 vs 493 us -- not kept
        const bool more = u + 1 < nmine;
        const auto dsc_n = S2_DESC(nb, nod, noh, now);
        // three accumulators per tile, one per product term: a tile's consecutive MFMAs then never wait for each other (with one
        // accumulator per tile a wave has two dependent chains and the matrix pipe idles half of the time)
        f32x4 acc[TPW], acc1[TPW], acc2[TPW];
#pragma unroll
        for (int i = 0; i < TPW; ++i) {
            acc[i] = bsh;
            acc1[i] = acc2[i] = f32x4{0.f, 0.f, 0.f, 0.f};
        }
        bf16x8 xh[2][TPW], xl[2][TPW];
#define S2_READ(P, BUFI)                                                                                         \
    {                                                                                                            \
        _Pragma("unroll") for (int i = 0; i < TPW; ++i) {                                                        \
            xh[BUFI][i] = *reinterpret_cast<const bf16x8*>(lds + img + rbp[P] + (2 * i * IW) * 32);              \
            xl[BUFI][i] = *reinterpret_cast<const bf16x8*>(lds + img + rbp[P] + (2 * i * IW) * 32 + REGION);     \
        }                                                                                                        \
    }
        S2_READ(0, 0)
#pragma unroll
        for (int p = 0; p < kPairs; ++p) {
            __builtin_amdgcn_sched_barrier(0);
            if (more) ps_dma_piece(dsc_n, lds + (IMG - img), wave, p, voff[p]);
            __builtin_amdgcn_sched_barrier(0);
            if (p + 1 < kPairs) S2_READ(p + 1, (p + 1) & 1)
#pragma unroll
            for (int i = 0; i < TPW; ++i) acc1[i] = sf_mfma16<F16>(wl[p], xh[p & 1][i], acc1[i]);
#pragma unroll
            for (int i = 0; i < TPW; ++i) acc2[i] = sf_mfma16<F16>(wh[p], xl[p & 1][i], acc2[i]);
#pragma unroll
            for (int i = 0; i < TPW; ++i) acc[i] = sf_mfma16<F16>(wh[p], xh[p & 1][i], acc[i]);
        }
#undef S2_READ
        {
            const auto dsc_ = window_desc(a.y, (long long)b_ * oframe_bytes + (((long long)(od + 1) * Hop + oh0 + 1) * Wop + ow0 + 1) * 128, ototal_bytes);
            const bool okc = ow0 + col < a.Wo;
#pragma unroll
            for (int i = 0; i < TPW; ++i) {
                f32x4 v = acc[i] + (acc1[i] + acc2[i]);          // the small terms first
#pragma unroll
                for (int e = 0; e < 4; ++e) v[e] = lrelu(F16 ? v[e] * a.unscale : v[e], a.neg_slope);
                if constexpr (O32P) {       // the fp32-padded format's range: +-16376 (a Winograd layer sums four of these in front of its fp16 split)
#pragma unroll
                    for (int e = 0; e < 4; ++e) v[e] = __builtin_amdgcn_fmed3f(v[e], -16376.f, 16376.f);
                    satm = sf_sat_acc(sf_sat_acc(satm, v[0], v[1]), v[2], v[3]);
                }
                u32x4 o;
                if constexpr (O32P) o = __builtin_bit_cast(u32x4, v);
                else o = ps_pack_split<F16>(v, satm);
                if (okc && oh0 + t0 + i < a.Ho) s2_store16(o, dsc_, vst, i * Wop * 128);
            }
        }
        b_ = nb; od = nod; oh0 = noh; ow0 = now;
    }
    if constexpr (F16) sf_sat_report(a.sat, O32P ? kSatWino : kSatSplit, satm, O32P ? 16376.f : kF16Max);
#undef S2_DECODE
#undef S2_DESC
}

template <bool F16 = false, bool O32P = false>
int s2_launch(S2Args a, hipStream_t st) {
    a.tiles_h = (int)mvsgi::cdiv(a.Ho, s2::TH);
    a.tiles_w = (int)mvsgi::cdiv(a.Wo, s2::TW);
    const long long nb = (long long)a.B * a.Do * a.tiles_h * a.tiles_w;
    MVSGI_REQUIRE(nb < (1ll << 31), "mvsgi_conv3d_s2rs: too many bricks");
    a.total_units = (int)nb;
    MVSGI_SAT_WORDS(sat_words_);
    a.sat = sat_words_;
    static mvsgi::PersistentGeom geo_cache[mvsgi::kMaxDevices] = {};
    return mvsgi::launch_persistent(conv3d_s2rs_kernel<F16, O32P>, 256, s2::LDS_BYTES, 1, geo_cache, "mvsgi_conv3d_s2rs", nb, st, a);
}

}  // namespace

// [Cout 32][Cin 16][27] x scale[Cout] -> [cout tile 2][14 pairs][hi | lo][64 lanes][8 x 16 bit] (ps_pack_weights_kernel's lane rule)
extern "C" size_t mvsgi_conv3d_s2rs_packed_weight_bytes(void) { return (size_t)2 * s2::kPairs * 2 * 64 * 16; }

extern "C" int mvsgi_conv3d_s2rs_pack_weights_fmt(const float* w_oidhw, const float* scale, void* w_packed, int fmt, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(w_oidhw && scale && w_packed, "mvsgi_conv3d_s2rs_pack_weights: null pointer");
    MVSGI_REQUIRE(fmt == 0 || fmt == MVSGI_SPLIT_F16, "mvsgi_conv3d_s2rs_pack_weights: fmt %d not in {0, MVSGI_SPLIT_F16}", fmt);
    hipLaunchKernelGGL(ps_pack_weights_kernel<s2::kTaps>, dim3(2 * s2::kPairs), dim3(64), 0, mvsgi::as_stream(stream), w_oidhw, scale,
                       static_cast<bf16x8*>(w_packed), 2, fmt != 0);
    return mvsgi::check_launch("mvsgi_conv3d_s2rs_pack_weights");
}
extern "C" int mvsgi_conv3d_s2rs_pack_weights(const float* w_oidhw, const float* scale, void* w_packed, mvsgi_stream_t stream) {
    return mvsgi_conv3d_s2rs_pack_weights_fmt(w_oidhw, scale, w_packed, 0, stream);
}

// y = act( conv3d(x, w, stride 2, padding 1) * scale + shift ), 16 -> 32 channels, on split-padded activations:
// x_split [B][D+2][H+2][W+2][64 B], y_split [B][Do+2][Ho+2][Wo+2][128 B] with Do = (D - 1) / 2 + 1 (likewise Ho, Wo); both
// zero-bordered, only y's interior is written.  w_packed from mvsgi_conv3d_s2rs_pack_weights (scale folded in).
// _fmt: fmt = MVSGI_SPLIT_F16 runs the layer in the fp16 split; `scale` (at packing) and `shift` then carry a power of two 1 / unscale
// chosen by the caller (the epilogue has no per-channel multiplier to hide it in), and the accumulators are multiplied by `unscale`
// _out_fmt: y_f32p != 0 (fp16 split only) writes y "fp32-padded": the same padded geometry, plain fp32 records
extern "C" int mvsgi_conv3d_s2rs_out_fmt(const void* x_split, const void* w_packed, const float* shift, void* y_split, int B, int D, int H,
                                         int W, float neg_slope, float unscale, int fmt, int y_f32p, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(x_split && w_packed && shift && y_split, "mvsgi_conv3d_s2rs: null pointer");
    MVSGI_REQUIRE(!y_f32p || fmt == MVSGI_SPLIT_F16, "mvsgi_conv3d_s2rs: the fp32-padded output exists in the fp16 split only");
    MVSGI_REQUIRE(fmt == 0 || fmt == MVSGI_SPLIT_F16, "mvsgi_conv3d_s2rs: fmt %d not in {0, MVSGI_SPLIT_F16}", fmt);
    MVSGI_REQUIRE(fmt != 0 || unscale == 1.f, "mvsgi_conv3d_s2rs: unscale is a parameter of the fp16 split");
    MVSGI_REQUIRE(unscale > 0.f, "mvsgi_conv3d_s2rs: unscale must be positive");
    MVSGI_REQUIRE(B > 0 && D > 0 && H > 0 && W > 0, "mvsgi_conv3d_s2rs: non-positive dimension");
    MVSGI_REQUIRE(neg_slope >= 0.f && neg_slope <= 1.f, "mvsgi_conv3d_s2rs: negative slope %g outside [0, 1]", (double)neg_slope);
    MVSGI_REQUIRE((long long)(D + 2) * (H + 2) * (W + 2) * 64 < 0x7fffff00ll, "mvsgi_conv3d_s2rs: input frame too large for 32-bit window offsets");
    S2Args a{};
    a.x = static_cast<const unsigned char*>(x_split);
    a.y = static_cast<unsigned char*>(y_split);
    a.wp = static_cast<const bf16x8*>(w_packed);
    a.shift = shift;
    a.B = B; a.D = D; a.H = H; a.W = W;
    a.Do = (D - 1) / 2 + 1; a.Ho = (H - 1) / 2 + 1; a.Wo = (W - 1) / 2 + 1;
    MVSGI_REQUIRE((long long)(a.Do + 2) * (a.Ho + 2) * (a.Wo + 2) * 128 < 0x7fffff00ll, "mvsgi_conv3d_s2rs: output frame too large for 32-bit offsets");
    a.neg_slope = neg_slope;
    a.unscale = unscale;
    hipStream_t st = mvsgi::as_stream(stream);
    if (fmt && y_f32p) return s2_launch<true, true>(a, st);
    if (fmt) return s2_launch<true>(a, st);
    return s2_launch<>(a, st);
}
extern "C" int mvsgi_conv3d_s2rs_fmt(const void* x_split, const void* w_packed, const float* shift, void* y_split, int B, int D, int H,
                                     int W, float neg_slope, float unscale, int fmt, mvsgi_stream_t stream) {
    return mvsgi_conv3d_s2rs_out_fmt(x_split, w_packed, shift, y_split, B, D, H, W, neg_slope, unscale, fmt, 0, stream);
}
extern "C" int mvsgi_conv3d_s2rs(const void* x_split, const void* w_packed, const float* shift, void* y_split, int B, int D, int H,
                                 int W, float neg_slope, mvsgi_stream_t stream) {
    return mvsgi_conv3d_s2rs_fmt(x_split, w_packed, shift, y_split, B, D, H, W, neg_slope, 1.f, 0, stream);
}
