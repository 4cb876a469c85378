// Photometric consistency of the predicted inverse distance: the cost volume's own fusion rule (SphericalSweepStdMasked,
// dsta_mvs/model/cost_volume_builder/spherical_sweep_avg.py:92-125: the masked variance over the cameras that see a point) applied
// to the colours the cameras show at the back-projected point, per pixel and as per-frame scores.  The definition is in
// include/mvsgi.h (section "photometric consistency") and DESIGN.md 19; steps 1-6 are reproject.hip's (the same functions of
// camera_models.hpp and sampling.hpp), so valid_n and w_n[c] are the bits of mvsgi_reproject_f32's valid and warped, which are never
// stored here.  This file is compiled with contraction off.
//
//   1. photo_reduce<IN, VEC, NT>  grid (G, B): a thread owns four consecutive pixels of a row (16-byte loads of inv and the ray
//                         planes, 16-byte stores of the fp32 planes, 4-byte stores of n_views; rows whose length is no multiple of
//                         four take the element-wise form of the same thread shape) and loops over the cameras: projection and
//                         validity once per camera, the grid coordinates of all NT >= N cameras stay in registers.  Then, per
//                         channel, one pass over the cameras fetches the samples into registers (taps set up again from the kept
//                         coordinates: eight floats of tap state per camera and pixel would not fit beside them), the mean and the
//                         deviations are taken from those registers: every tap is fetched once.  The quads of a frame are strided
//                         over G blocks.  With a table, the thread's record: the sums of std and var (pairs), the bad, scored and
//                         masked counts and the histogram of views.
//   2. photo_finalise     frame_finalise with WriteRow's formulas (with a table only).
// The table's scheme -- records, slab, merge order, finalise -- is csrc/frame_reduce.hpp's; G = ceil(quads / 256), at most 256.
#include "common.hpp"

namespace {

#include "camera_models.hpp"
#include "frame_reduce.hpp"
#include "sampling.hpp"

using mvsgi::aligned;
using mvsgi::kMaxCams;
constexpr int kCamFloats = 10;            // host camera table row, as mvsgi_reproject_f32's
constexpr int kMaxReduceBlocks = 256;     // records per frame (what frame_finalise sums in order)
constexpr int kViews = kMaxCams + 1;      // histogram bins: 0 .. 8 seen cameras
constexpr int kRec = 7 + kViews;          // doubles per record
constexpr int kCols = 5 + kViews;         // n, mean_std, rms, bad, coverage, views_0 .. views_8

enum { F_SH, F_SL, F_VH, F_VL, F_NB, F_N, F_NM, F_V0 };
enum PhotoModel { DOUBLE_SPHERE = 0, EQUIRECT = 1 };

struct PhotoCam {
    float T[12];                          // rows 0..2 of the 4 x 4 transform, row-major
    DsParams ds;                          // read when model == DOUBLE_SPHERE
    int model, pad;
};
struct PhotoRig {
    PhotoCam cam[kMaxCams];
};
struct PhotoDims {
    int N, C, Hr, Wr, H, W;
    int Wq;                               // threads per output row: ceil(W / 4)
    int nq;                               // quads per frame: H * Wq
    int mask_per_frame;
};
struct PhotoOut {
    unsigned char* n_views;
    float *var, *std, *mean;
    double* recs;
};

struct RecMerge {
    __device__ __forceinline__ void operator()(double* a, const double* b) const {
        sum_merge(a[F_SH], a[F_SL], b[F_SH], b[F_SL]);
        sum_merge(a[F_VH], a[F_VL], b[F_VH], b[F_VL]);
#pragma unroll
        for (int j = F_NB; j < kRec; ++j) a[j] += b[j];
    }
};

// IN: layout of the camera images.  VEC: W % 4 == 0; otherwise element-wise with a row tail.  NT: cameras held in registers, N <= NT.
template <int IN, bool VEC, int NT>
__global__ __launch_bounds__(kThreads) void photo_reduce(const float* __restrict__ inv, const float* __restrict__ rays,
                                                         const void* __restrict__ imgs, const float* __restrict__ cam_masks,
                                                         const unsigned char* __restrict__ mask, PhotoOut o, PhotoRig rig, PhotoDims s,
                                                         float bf, float thresh, float pi_f) {
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    stage_u8_table<IN>(lut);
    const int t = threadIdx.x, G = gridDim.x;
    const long long b = blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    const long long HWr = (long long)s.Hr * s.Wr;
    const float* invb = inv + b * HW;
    const unsigned char* mb = mask ? mask + (s.mask_per_frame ? b * HW : 0) : nullptr;
    const float fC = (float)s.C;

    double sh = 0.0, sl = 0.0, vh = 0.0, vl = 0.0;
    unsigned nbad = 0, nsc = 0, nmask = 0, hist[kViews];
#pragma unroll
    for (int k = 0; k < kViews; ++k) hist[k] = 0;

    for (int q = blockIdx.x * kThreads + t; q < s.nq; q += G * kThreads) {
        const int i = q / s.Wq;
        const int j = (q - i * s.Wq) * 4;
        const int n = VEC ? 4 : min(4, s.W - j);                          // pixels of this thread inside the row
        const long long pix = (long long)i * s.W + j;                     // first pixel of this thread inside a plane

        // steps 1, 2 of the back-projection: d = bf / v, p = r * d
        float px[4], py[4], pz[4];
        {
            float v[4], rx[4], ry[4], rz[4];
            if (VEC) {
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(invb + pix);
                const f32x4 x4 = *reinterpret_cast<const f32x4*>(rays + pix);
                const f32x4 y4 = *reinterpret_cast<const f32x4*>(rays + HW + pix);
                const f32x4 z4 = *reinterpret_cast<const f32x4*>(rays + 2 * HW + pix);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = v4[k], rx[k] = x4[k], ry[k] = y4[k], rz[k] = z4[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = k < n;
                    v[k] = in ? invb[pix + k] : 1.0f;
                    rx[k] = in ? rays[pix + k] : 0.0f;
                    ry[k] = in ? rays[HW + pix + k] : 0.0f;
                    rz[k] = in ? rays[2 * HW + pix + k] : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) back_project(bf, v[k], rx[k], ry[k], rz[k], px[k], py[k], pz[k]);
        }

        // steps 3-5 per camera, and the definition's step 1: seen = valid (& the camera's mask sampled at the same grid > 0)
        float gx[NT][4], gy[NT][4];
        unsigned valid = 0, seen = 0;                                     // bit 4 * cam + k
        float cnt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int cam = 0; cam < NT; ++cam) {
            if (cam < s.N) {
                const PhotoCam& c = rig.cam[cam];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const float x = transform_row(c.T, px[k], py[k], pz[k]);
                    const float y = transform_row(c.T + 4, px[k], py[k], pz[k]);
                    const float z = transform_row(c.T + 8, px[k], py[k], pz[k]);
                    bool in_fov = true;
                    if (c.model == DOUBLE_SPHERE)
                        in_fov = project_double_sphere(c.ds, x, y, z, gx[cam][k], gy[cam][k]);
                    else
                        project_equirect(x, y, z, pi_f, gx[cam][k], gy[cam][k]);
                    const bool ok = grid_valid(in_fov, gx[cam][k], gy[cam][k]) && k < n;
                    bool sn = ok;
                    if (ok && cam_masks) {                                // an invalid camera's taps are not fetched
                        const Bilin bt = bilin_setup(gx[cam][k], gy[cam][k], s.Wr, s.Hr);
                        sn = bilin_fetch(cam_masks + cam * HWr, bt) > 0.0f;
                    }
                    valid |= (ok ? 1u : 0u) << (4 * cam + k);
                    seen |= (sn ? 1u : 0u) << (4 * cam + k);
                    cnt[k] = cnt[k] + (sn ? 1.0f : 0.0f);                 // the definition's step 2, in camera order
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) gx[cam][k] = gy[cam][k] = 0.0f;
            }
        }
        bool ok[4];
        float kdiv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = cnt[k] > 1.0f;
            kdiv[k] = ok[k] ? cnt[k] : 1.0f;
        }

        // steps 3-5 of the definition, channel by channel; the samples of the channel stay in registers between the two passes
        float vsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        auto channel = [&](int ch) {
            float w[NT][4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            // the kept coordinates pass through an empty statement the compiler cannot see through, once per channel and ahead of
            // its loads: without it the tap set-up is hoisted out of the channel loop and its eight values per camera and pixel spill
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(gx[cam][k]), "+v"(gy[cam][k]));
            }
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[cam][k] = 0.0f;                                     // what the back-projection writes for an invalid camera
                    if (cam < s.N && ((valid >> (4 * cam + k)) & 1u)) {
                        const Bilin bt = bilin_setup(gx[cam][k], gy[cam][k], s.Wr, s.Hr);
                        const long long m = b * s.N + cam;
                        if (IN == U8HWC3)
                            w[cam][k] = bilin_fetch_u8(static_cast<const unsigned char*>(imgs) + m * HWr * 3, ch, lut, bt);
                        else
                            w[cam][k] = bilin_fetch(static_cast<const float*>(imgs) + (m * s.C + ch) * HWr, bt);
                    }
                    if (cam < s.N) acc[k] = acc[k] + w[cam][k] * (((seen >> (4 * cam + k)) & 1u) ? 1.0f : 0.0f);
                }
            }
            float avg[4], var[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                avg[k] = acc[k] / kdiv[k];
                var[k] = 0.0f;
            }
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (cam < s.N) {
                        const float x = ((seen >> (4 * cam + k)) & 1u) ? w[cam][k] : avg[k];
                        const float d = x - avg[k];
                        var[k] = var[k] + d * d;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                var[k] = ok[k] ? var[k] / kdiv[k] : 0.0f;
                vsum[k] = vsum[k] + var[k];
            }
            if (o.mean) {
                float* m = o.mean + (b * s.C + ch) * HW + pix;
                if (VEC) {
                    *reinterpret_cast<f32x4*>(m) = f32x4{avg[0], avg[1], avg[2], avg[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) m[k] = avg[k];
                }
            }
        };
        if (IN == U8HWC3) {
            channel(0), channel(1), channel(2);
        } else {
#pragma unroll 1
            for (int ch = 0; ch < s.C; ++ch) channel(ch);
        }

        // steps 5, 6 and the per-pixel outputs
        float pv[4], ps[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pv[k] = vsum[k] / fC;
            ps[k] = sqrtf(pv[k]);
        }
        if (VEC) {
            if (o.var) *reinterpret_cast<f32x4*>(o.var + b * HW + pix) = f32x4{pv[0], pv[1], pv[2], pv[3]};
            if (o.std) *reinterpret_cast<f32x4*>(o.std + b * HW + pix) = f32x4{ps[0], ps[1], ps[2], ps[3]};
            if (o.n_views)
                *reinterpret_cast<unsigned*>(o.n_views + b * HW + pix) =
                    (unsigned)cnt[0] | ((unsigned)cnt[1] << 8) | ((unsigned)cnt[2] << 16) | ((unsigned)cnt[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < n) {
                    if (o.var) o.var[b * HW + pix + k] = pv[k];
                    if (o.std) o.std[b * HW + pix + k] = ps[k];
                    if (o.n_views) o.n_views[b * HW + pix + k] = (unsigned char)cnt[k];
                }
            }
        }

        // step 7: the scores
        if (o.recs) {
            unsigned mw = 0x01010101u;
            if (mb) {
                if (VEC) {
                    mw = *reinterpret_cast<const unsigned*>(mb + pix);
                } else {
                    mw = 0u;
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) mw |= (unsigned)mb[pix + k] << (8 * k);
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool masked = k < n && ((mw >> (8 * k)) & 0xffu) != 0u;
                const int c = (int)cnt[k];
#pragma unroll
                for (int h = 0; h < kViews; ++h) hist[h] += (masked && c == h) ? 1u : 0u;
                nmask += masked ? 1u : 0u;
                if (masked && ok[k]) {                                    // a select: an unscored pixel never reaches a sum
                    sum_add(sh, sl, (double)ps[k]);
                    sum_add(vh, vl, (double)pv[k]);
                    nbad += ps[k] > thresh ? 1u : 0u;
                    nsc += 1u;
                }
            }
        }
    }
    if (!o.recs) return;

    double r[kRec];
    r[F_SH] = sh, r[F_SL] = sl, r[F_VH] = vh, r[F_VL] = vl;
    r[F_NB] = (double)nbad, r[F_N] = (double)nsc, r[F_NM] = (double)nmask;
#pragma unroll
    for (int h = 0; h < kViews; ++h) r[F_V0 + h] = (double)hist[h];
    block_reduce_store<kRec>(r, o.recs, b, G, RecMerge());
}

struct WriteRow {
    __device__ __forceinline__ void operator()(const double* x, double* row) const {
        const double n = x[F_N];
        const double nan = __builtin_nan("");
        row[0] = n;
        row[1] = n > 0.0 ? sum_value(x[F_SH], x[F_SL]) / n : nan;
        row[2] = n > 0.0 ? sqrt(sum_value(x[F_VH], x[F_VL]) / n) : nan;
        row[3] = n > 0.0 ? x[F_NB] / n : nan;
        row[4] = n / x[F_NM];
#pragma unroll
        for (int h = 0; h < kViews; ++h) row[5 + h] = x[F_V0 + h];
    }
};

__global__ __launch_bounds__(kThreads) void photo_finalise(const double* recs, double* fsum, double* __restrict__ out, int B, int G) {
    frame_finalise<kRec, kCols>(recs, fsum, out, B, G, RecMerge(), WriteRow());
}

// a reduce block per kThreads quads of a frame (a quad: four consecutive pixels of a row, a thread's unit of work)
inline FrameSlab layout(long long B, int H, int W) {
    return frame_slab(B, (long long)H * ((W + 3) / 4), kThreads, kMaxReduceBlocks, kRec);
}

bool dims_ok(long long B, int H, int W) { return frame_dims_ok(B, H, W, 4ll * kMaxReduceBlocks * kThreads); }

}  // namespace

extern "C" size_t mvsgi_photo_ws_bytes(long long B, int H, int W) {
    if (!dims_ok(B, H, W)) return 0;
    return layout(B, H, W).total * sizeof(double);
}

extern "C" int mvsgi_photo_consistency_f32(const float* inv, const float* rays, const void* imgs, int img_kind, const float* cam_masks,
                                           const float* T_host, const float* cams_host, const unsigned char* mask, int mask_per_frame,
                                           float thresh, unsigned char* n_views, float* photo_var, float* photo_std,
                                           float* mean_colour, void* ws, size_t ws_bytes, double* table, long long B, int N, int C,
                                           int Hr, int Wr, int H, int W, float bf, mvsgi_stream_t stream) {
    const char* what = "mvsgi_photo_consistency_f32";
    MVSGI_REQUIRE(inv && rays && imgs && T_host && cams_host, "%s: null pointer (inv, rays, imgs, T and cams are required)", what);
    MVSGI_REQUIRE(n_views || photo_var || photo_std || mean_colour || table, "%s: null pointer (every output is NULL)", what);
    MVSGI_REQUIRE(N >= 1 && N <= kMaxCams, "%s: N = %d cameras (need 1 <= N <= %d)", what, N, kMaxCams);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
    MVSGI_REQUIRE(img_kind == U8HWC3 || img_kind == F32CHW, "%s: unknown image kind %d (0 = uint8 HWC3, 1 = fp32 CHW)", what, img_kind);
    MVSGI_REQUIRE(C >= 1, "%s: C = %d channels (need C >= 1)", what, C);
    MVSGI_REQUIRE(img_kind != U8HWC3 || C == 3, "%s: uint8 images have C = 3 channels, got C = %d", what, C);
    MVSGI_REQUIRE(Hr >= 1 && Wr >= 1, "%s: non-positive dimension (image %d x %d)", what, Hr, Wr);
    if (check_tap_offsets(what, "image", img_kind, Hr, Wr)) return 1;
    if (cam_masks && check_tap_offsets(what, "camera mask", F32CHW, Hr, Wr)) return 1;
    MVSGI_REQUIRE(dims_ok(B, H, W), "%s: map %d x %d or batch %lld too large (H * W < 2^31 - 2^18, B < 65535)", what, H, W, B);
    MVSGI_REQUIRE(mask_per_frame == 0 || mask_per_frame == 1, "%s: mask_per_frame = %d (0: [H][W], 1: [B][H][W])", what, mask_per_frame);
    MVSGI_REQUIRE(thresh == thresh, "%s: thresh is a NaN", what);
    PhotoRig rig;
    memset(&rig, 0, sizeof(rig));
    for (int k = 0; k < N; ++k) {
        const float* t = cams_host + k * kCamFloats;
        PhotoCam& c = rig.cam[k];
        MVSGI_REQUIRE(t[0] == (float)DOUBLE_SPHERE || t[0] == (float)EQUIRECT,
                      "%s: camera %d: unknown model id %g (0 = double sphere, 1 = equirectangular)", what, k, (double)t[0]);
        c.model = (int)t[0];
        memcpy(c.T, T_host + k * 16, sizeof(c.T));
        if (c.model == DOUBLE_SPHERE) {
            // calib_h - 1 and calib_w - 1 of an integer shape: whole numbers a float holds exactly, so the casts below are exact
            auto size_m1 = [](float v) { return v >= 1.0f && v < 16777216.0f && v == truncf(v); };
            MVSGI_REQUIRE(size_m1(t[8]) && size_m1(t[9]), "%s: camera %d: calib shape (%g, %g) (need calib > 1)", what, k,
                          (double)t[8] + 1.0, (double)t[9] + 1.0);
            c.ds = make_ds_params(t[1], t[2], t[3], t[4], t[5], t[6], (int)t[8] + 1, (int)t[9] + 1, t[7]);
        }
    }
    MVSGI_REQUIRE(aligned(n_views, 16) && aligned(photo_var, 16) && aligned(photo_std, 16) && aligned(mean_colour, 16),
                  "%s: outputs must be 16-byte aligned", what);
    MVSGI_REQUIRE(aligned(cam_masks, 4) && (img_kind == U8HWC3 || aligned(imgs, 4)), "%s: fp32 images and masks must be 4-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (vec) {
        MVSGI_REQUIRE(aligned(inv, 16) && aligned(rays, 16), "%s: inv and rays must be 16-byte aligned when W %% 4 == 0", what);
        MVSGI_REQUIRE(aligned(mask, 4), "%s: mask must be 4-byte aligned when W %% 4 == 0", what);
    }
    const FrameSlab l = layout(B, H, W);
    double* slab = nullptr;
    if (table) {
        MVSGI_REQUIRE(ws, "%s: null pointer (the table needs ws)", what);
        MVSGI_REQUIRE(ws_bytes >= l.total * sizeof(double), "%s: workspace of %zu bytes is too small (mvsgi_photo_ws_bytes: %zu)", what,
                      ws_bytes, l.total * sizeof(double));
        MVSGI_REQUIRE(aligned(ws, 8) && aligned(table, 8), "%s: ws and table must be 8-byte aligned", what);
        slab = static_cast<double*>(ws);
    }
    PhotoDims s{N, C, Hr, Wr, H, W, (W + 3) / 4, H * ((W + 3) / 4), mask_per_frame};
    PhotoOut o{n_views, photo_var, photo_std, mean_colour, slab ? slab + l.rec : nullptr};
    const dim3 blocks((unsigned)l.G, (unsigned)B);
    hipStream_t st = mvsgi::as_stream(stream);
#define MVSGI_PHOTO_LAUNCH(IN, VEC)                                                                                              \
    do {                                                                                                                          \
        if (N <= 4)                                                                                                               \
            hipLaunchKernelGGL((photo_reduce<IN, VEC, 4>), blocks, dim3(kThreads), 0, st, inv, rays, imgs, cam_masks, mask, o, rig, s, \
                               bf, thresh, kPiF);                                                                                 \
        else                                                                                                                      \
            hipLaunchKernelGGL((photo_reduce<IN, VEC, 8>), blocks, dim3(kThreads), 0, st, inv, rays, imgs, cam_masks, mask, o, rig, s, \
                               bf, thresh, kPiF);                                                                                 \
    } while (0)
    MVSGI_LAUNCH_IMAGE_KIND_VEC(MVSGI_PHOTO_LAUNCH, img_kind, vec);
#undef MVSGI_PHOTO_LAUNCH
    if (mvsgi::check_launch("mvsgi_photo_consistency_f32 (reduce)")) return 1;
    if (!table) return 0;
    hipLaunchKernelGGL(photo_finalise, dim3((unsigned)B + 1u), dim3(kThreads), 0, st, slab + l.rec, slab + l.fsum, table, (int)B, l.G);
    return mvsgi::check_launch("mvsgi_photo_consistency_f32 (finalise)");
}
