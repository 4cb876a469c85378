// Forward values of the training losses of dsta_mvs/support/loss_function/distance_loss.py (VolumeCrossEntropy, MaskedSmoothL1Loss and
// InBoundsBCEDistanceLoss on an image) for every frame of a batch and pooled.  The definition is in include/mvsgi.h (section "loss
// functions") and DESIGN.md 18; per element it is the reference's fp32 arithmetic (this file is compiled with contraction off),
// only the accumulations are wider.  No gradients: this path has no autograd anywhere.
//
//   1. losses_reduce<DMAX, FUSED>  grid (G, B): a frame's OH * OW pixels are a flat run, one thread per pixel (strided by G * 256
//                         where a frame has more pixels than the grid has threads); the thread walks D.  The probabilities are
//                         either read (pred_cost, FUSED = false) or are those of the soft-argmin's softmax at that pixel, from
//                         the low-resolution costs by csrc/confidence.hip's expressions (sa_blend, max, expf(-(m - v)), the sum in
//                         order of d, e / S): no [B, D, OH, OW] tensor is read or written.  D <= 16 and D <= 32 gather the blended
//                         candidates once into registers; larger D walks them again per pass.  The thread's record: the sums of
//                         the cross-entropy and smooth-L1 addends (pairs), the two counts and the in-bounds mismatches.
//   2. losses_finalise    frame_finalise with WriteRow's formulas.
// The table's scheme -- records, slab, merge order, finalise -- is csrc/frame_reduce.hpp's; G = ceil(OH * OW / 256), at most 256.
#include "common.hpp"

#include <cmath>

namespace {

#include "frame_reduce.hpp"
#include "softargmin_axes.hpp"

using mvsgi::aligned;
constexpr int kMaxReduceBlocks = 256;     // records per frame (what frame_finalise sums in order)
constexpr int kRec = 8;                   // doubles per record
constexpr int kCols = 5;                  // vol, smooth_l1, inbounds, n_vol, n_px

enum { F_VH, F_VL, F_SH, F_SL, F_NV, F_NP, F_MM, F_PAD };

struct Params {
    int p_kind, vol_kind, px_kind, inbounds, D, H, W, OW;
    float hi, near_inv, far_inv, rs;
};

struct RecMerge {
    __device__ __forceinline__ void operator()(double* a, const double* b) const {
        sum_merge(a[F_VH], a[F_VL], b[F_VH], b[F_VL]);
        sum_merge(a[F_SH], a[F_SL], b[F_SH], b[F_SL]);
        a[F_NV] += b[F_NV];
        a[F_NP] += b[F_NP];
        a[F_MM] += b[F_MM];
    }
};

// ATen's binary_cross_entropy per element: std::max(log, -100) keeps a NaN
__device__ __forceinline__ float bce(float t, float p) {
    float lq = log1pf(-p);
    lq = lq < -100.0f ? -100.0f : lq;
    // D - 2 of a pixel's D labels are 0: there (0 - 1) * lq - 0 * lp is -lq bit for bit for every p in [0, 1] (0 * lp is a zero, and
    // -lq is never -0), so logf is left out; any other p takes the expression as written
    if (t == 0.0f && p >= 0.0f && p <= 1.0f) return -lq;
    float lp = logf(p);
    lp = lp < -100.0f ? -100.0f : lp;
    return (t - 1.0f) * lq - t * lp;
}

struct Acc {
    double vh, vl, sh, sl;
    unsigned nv, np, mm;
};

template <int DMAX, bool FUSED>
__global__ __launch_bounds__(kThreads) void losses_reduce(const float* __restrict__ labels, const float* __restrict__ pred,
                                                          const float* __restrict__ pred_cost, const float* __restrict__ costs,
                                                          const float* __restrict__ inv_list, const unsigned char* __restrict__ vol_mask,
                                                          const unsigned char* __restrict__ px_mask, float* __restrict__ true_cost,
                                                          double* __restrict__ recs, int npix, Params k) {
    const int t = threadIdx.x, b = blockIdx.y, G = gridDim.x, D = k.D;
    const long long fbase = (long long)b * npix;            // the frame in a [B][OH][OW] tensor
    const long long vbase = (long long)b * D * npix;        // the frame in a [B][D][OH][OW] tensor
    const float* lb = labels + fbase;
    Acc a = {0.0, 0.0, 0.0, 0.0, 0u, 0u, 0u};
    const long long step = (long long)G * kThreads;
    for (long long i = (long long)blockIdx.x * kThreads + t; i < npix; i += step) {
        const float L = lb[i];
        // ---- the image losses: MaskedSmoothL1Loss and InBoundsBCEDistanceLoss on pred [B][1][OH][OW]
        const bool spx = k.px_kind == 0 ? true : k.px_kind == 1 ? px_mask[fbase + i] != 0 : (L <= k.hi);
        if (spx) {                                           // a select: a NaN at an unselected pixel never reaches a sum
            a.np += 1u;
            if (pred) {
                const float P = pred[fbase + i];
                const float z = fabsf(P - L);
                const float s = z < 1.0f ? 0.5f * z * z : z - 0.5f;
                sum_add(a.sh, a.sl, (double)s);
                const bool pin = (P < k.near_inv) && (P > k.far_inv);
                const bool lin = (L < k.near_inv) && (L > k.far_inv);
                a.mm += pin != lin ? 1u : 0u;
            }
        }
        // ---- VolumeCrossEntropy: the two-hot label of the pixel, then the walk over D
        const bool walk = k.p_kind != 0 && (k.vol_kind != 1 || vol_mask[fbase + i] != 0);
        if (!walk && !true_cost) continue;
        const float x = clamp_nan(L, inv_list[D - 1], inv_list[0]);
        int below = 0;                                       // torch.bucketize(x, flipped list): the candidates below x
        for (int d = 0; d < D; ++d) below += inv_list[d] < x ? 1 : 0;
        int bin = D - below - 1;
        bin = bin < 0 ? 0 : bin > D - 2 ? D - 2 : bin;
        const float lo = inv_list[bin];
        const float dd = (x - lo) / (inv_list[bin + 1] - lo);
        const float t0 = 1.0f - dd;
        auto label = [&](int d) { return d == bin ? t0 : d == bin + 1 ? dd : 0.0f; };
        if (true_cost) {
            float* tc = true_cost + vbase + i;
            for (int d = 0; d < D; ++d) tc[(long long)d * npix] = label(d);
        }
        if (!walk) continue;
        const unsigned char* vm = k.vol_kind == 2 ? vol_mask + vbase + i : nullptr;
        auto element = [&](int d, float p) {
            if (vm && vm[(long long)d * npix] == 0) return;
            sum_add(a.vh, a.vl, (double)bce(label(d), p));
            a.nv += 1u;
        };
        if constexpr (!FUSED) {
            const float* pc = pred_cost + vbase + i;
            for (int d = 0; d < D; ++d) element(d, pc[(long long)d * npix]);
        } else {
            // the soft-argmin's softmax at this pixel: coordinates, zero-weight-tap rule and blend of csrc/confidence.hip
            const int oy = (int)(i / k.OW), ox = (int)(i - (long long)oy * k.OW);
            const Axis2 ay = axis2f(oy, k.H, k.rs), ax = axis2f(ox, k.W, k.rs);
            const long long HW = (long long)k.H * k.W;
            const float* cb = costs + (long long)b * D * HW;
            const Taps taps = sa_taps(ay, ax, k.W);
            auto sample = [&](int d) { return sa_sample(cb + d * HW, ay, ax, taps); };
            float m = -INFINITY, S = 0.f;
            if constexpr (DMAX > 0) {
                float v[DMAX];
#pragma unroll
                for (int d = 0; d < DMAX; ++d) {
                    v[d] = d < D ? sample(d) : -INFINITY;
                    if (v[d] > m) m = v[d];
                }
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    if (d < D) {
                        v[d] = expf(-(m - v[d]));
                        S = S + v[d];
                    }
#pragma unroll
                for (int d = 0; d < DMAX; ++d)
                    if (d < D) element(d, v[d] / S);
            } else {
                for (int d = 0; d < D; ++d) {
                    const float v = sample(d);
                    if (v > m) m = v;
                }
                for (int d = 0; d < D; ++d) S = S + expf(-(m - sample(d)));
                for (int d = 0; d < D; ++d) element(d, expf(-(m - sample(d))) / S);
            }
        }
    }
    double r[kRec];
    r[F_VH] = a.vh, r[F_VL] = a.vl, r[F_SH] = a.sh, r[F_SL] = a.sl;
    r[F_NV] = (double)a.nv, r[F_NP] = (double)a.np, r[F_MM] = (double)a.mm, r[F_PAD] = 0.0;
    block_reduce_store<kRec>(r, recs, b, G, RecMerge());
}

struct WriteRow {
    __device__ __forceinline__ void operator()(const double* x, double* row, int have_vol, int have_pred, int inbounds) const {
        const double nan = __builtin_nan("");
        row[0] = have_vol ? sum_value(x[F_VH], x[F_VL]) / x[F_NV] : nan;
        row[1] = have_pred ? sum_value(x[F_SH], x[F_SL]) / x[F_NP] : nan;
        row[2] = have_pred && inbounds ? 100.0 * x[F_MM] / x[F_NP] : nan;
        row[3] = have_vol ? x[F_NV] : nan;
        row[4] = x[F_NP];
    }
};

__global__ __launch_bounds__(kThreads) void losses_finalise(const double* recs, double* fsum, double* __restrict__ out, int B, int G,
                                                            int have_vol, int have_pred, int inbounds) {
    frame_finalise<kRec, kCols>(recs, fsum, out, B, G, RecMerge(), WriteRow(), have_vol, have_pred, inbounds);
}

// a reduce block per kThreads pixels of a frame
inline FrameSlab layout(int B, int OH, int OW) { return frame_slab(B, (long long)OH * OW, kThreads, kMaxReduceBlocks, kRec); }

bool dims_ok(int B, int OH, int OW) { return frame_dims_ok(B, OH, OW, (long long)kMaxReduceBlocks * kThreads); }

}  // namespace

extern "C" size_t mvsgi_losses_ws_bytes(int B, int OH, int OW) {
    if (!dims_ok(B, OH, OW)) return 0;
    return layout(B, OH, OW).total * sizeof(double);
}

extern "C" int mvsgi_losses_f32(const float* labels, const float* pred, const float* probs, int p_kind, const float* inv_list,
                                const unsigned char* vol_mask, int vol_kind, const unsigned char* px_mask, int px_kind, float label_max,
                                int inbounds, float near_inv, float far_inv, float* true_cost, void* ws, size_t ws_bytes, double* out,
                                int B, int D, int H, int W, double scale, int OH, int OW, mvsgi_stream_t stream) {
    const char* what = "mvsgi_losses_f32";
    MVSGI_REQUIRE(labels && ws && out, "%s: null pointer (labels, ws and out are required)", what);
    MVSGI_REQUIRE(p_kind >= MVSGI_LOSSES_P_NONE && p_kind <= MVSGI_LOSSES_P_FUSED, "%s: p_kind = %d (0 none, 1 given, 2 fused)", what, p_kind);
    MVSGI_REQUIRE(p_kind == MVSGI_LOSSES_P_NONE || probs, "%s: null pointer (p_kind %d needs probs)", what, p_kind);
    if (p_kind != MVSGI_LOSSES_P_NONE || true_cost) {
        MVSGI_REQUIRE(inv_list, "%s: null pointer (the volume labels need inv_list)", what);
        MVSGI_REQUIRE(D >= 2, "%s: D = %d: the volume labels need at least two candidates", what, D);
    }
    MVSGI_REQUIRE(vol_kind >= MVSGI_LOSSES_VOL_NONE && vol_kind <= MVSGI_LOSSES_VOL_VOLUME,
                  "%s: vol_kind = %d (0 none, 1 pixel mask, 2 volume mask)", what, vol_kind);
    MVSGI_REQUIRE(vol_kind == MVSGI_LOSSES_VOL_NONE || vol_mask, "%s: null pointer (vol_kind %d needs vol_mask)", what, vol_kind);
    MVSGI_REQUIRE(px_kind >= MVSGI_LOSSES_PX_NONE && px_kind <= MVSGI_LOSSES_PX_LABEL_MAX,
                  "%s: px_kind = %d (0 none, 1 mask tensor, 2 label <= label_max)", what, px_kind);
    MVSGI_REQUIRE(px_kind != MVSGI_LOSSES_PX_TENSOR || px_mask, "%s: null pointer (px_kind 1 needs px_mask)", what);
    MVSGI_REQUIRE(px_kind != MVSGI_LOSSES_PX_LABEL_MAX || label_max == label_max, "%s: label_max is a NaN", what);
    MVSGI_REQUIRE(B >= 1 && OH >= 1 && OW >= 1, "%s: non-positive dimension (B %d, OH %d, OW %d)", what, B, OH, OW);
    MVSGI_REQUIRE(dims_ok(B, OH, OW), "%s: dimensions exceed the launch geometry (B %d, OH %d, OW %d)", what, B, OH, OW);
    float rs = 1.0f;
    if (p_kind == MVSGI_LOSSES_P_FUSED) {
        MVSGI_REQUIRE(H >= 1 && W >= 1, "%s: non-positive dimension (H %d, W %d)", what, H, W);
        MVSGI_REQUIRE(std::isfinite(scale) && scale > 0.0, "%s: scale %g is not a finite positive factor", what, scale);
        // F.interpolate: floor(in * scale) in double
        const double oh = std::floor((double)H * scale), ow = std::floor((double)W * scale);
        MVSGI_REQUIRE(oh >= 1.0 && ow >= 1.0 && oh < 2147483648.0 && ow < 2147483648.0 && OH == (int)oh && OW == (int)ow,
                      "%s: caller's output %d x %d is not floor(%d x %d * %g) = %g x %g", what, OH, OW, H, W, scale, oh, ow);
        rs = (float)(1.0 / scale);
    }
    const FrameSlab l = layout(B, OH, OW);
    MVSGI_REQUIRE(ws_bytes >= l.total * sizeof(double), "%s: workspace of %zu bytes is too small (mvsgi_losses_ws_bytes: %zu)", what,
                  ws_bytes, l.total * sizeof(double));
    MVSGI_REQUIRE(aligned(ws, 8) && aligned(out, 8), "%s: ws and out must be 8-byte aligned", what);
    MVSGI_REQUIRE(aligned(labels, 4) && aligned(pred, 4) && aligned(probs, 4) && aligned(inv_list, 4) && aligned(true_cost, 4),
                  "%s: fp32 tensors must be 4-byte aligned", what);
    Params k;
    k.p_kind = p_kind, k.vol_kind = vol_kind, k.px_kind = px_kind, k.inbounds = inbounds ? 1 : 0;
    k.D = D, k.H = H, k.W = W, k.OW = OW;
    k.hi = label_max, k.near_inv = near_inv, k.far_inv = far_inv, k.rs = rs;
    const int npix = OH * OW;
    double* slab = static_cast<double*>(ws);
    hipStream_t st = mvsgi::as_stream(stream);
    const bool fused = p_kind == MVSGI_LOSSES_P_FUSED;
    auto kern = !fused ? losses_reduce<0, false>
                       : D <= 16 ? losses_reduce<16, true> : (D <= 32 ? losses_reduce<32, true> : losses_reduce<0, true>);
    hipLaunchKernelGGL(kern, dim3((unsigned)l.G, (unsigned)B), dim3(kThreads), 0, st, labels, pred, fused ? nullptr : probs,
                       fused ? probs : nullptr, inv_list, vol_mask, px_mask, true_cost, slab + l.rec, npix, k);
    if (mvsgi::check_launch("mvsgi_losses_f32 (reduce)")) return 1;
    hipLaunchKernelGGL(losses_finalise, dim3((unsigned)B + 1u), dim3(kThreads), 0, st, slab + l.rec, slab + l.fsum, out, B, l.G,
                       p_kind != MVSGI_LOSSES_P_NONE ? 1 : 0, pred ? 1 : 0, k.inbounds);
    return mvsgi::check_launch("mvsgi_losses_f32 (finalise)");
}
