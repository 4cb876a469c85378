// Photometric consistency of the predicted inverse distance: the cost volume's own fusion rule (SphericalSweepStdMasked,
// dsta_mvs/model/cost_volume_builder/spherical_sweep_avg.py:92-125: the masked variance over the cameras that see a point) applied
// to the colours the cameras show at the back-projected point, per pixel and as per-frame scores.  The definition is in
// include/mvsgi.h (section "photometric consistency") and DESIGN.md 19; steps 1-6 are reproject.hip's (the same functions of
// view_rig.hpp -- the rig, its host loop, a point's way into a camera, the byte quads read; the quad's points are its text, kept in
// photo_reduce.inc for the row-tail instances' sake -- and sampling.hpp), so
// valid_n and w_n[c] are the bits of mvsgi_reproject_f32's valid and warped, which are never stored here.  This file is compiled with
// contraction off.
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
//                         photo_reduce_seen<IN, VEC, NT> is the same text with one more input, cam_seen [B][N][H][W] bytes: a camera
//                         sees a pixel only where its byte is set (mvsgi_photo_consistency_seen_f32; photo_reduce.inc).
//   2. photo_finalise     frame_finalise with WriteRow's formulas (with a table only).
// The table's scheme -- records, slab, merge order, finalise -- is csrc/frame_reduce.hpp's; G = ceil(quads / 256), at most 256.
#include "common.hpp"

namespace {

#include "frame_reduce.hpp"
#include "sampling.hpp"
#include "view_rig.hpp"

using mvsgi::aligned;
using mvsgi::kMaxCams;
constexpr int kMaxReduceBlocks = 256;     // records per frame (what frame_finalise sums in order)
constexpr int kViews = kMaxCams + 1;      // histogram bins: 0 .. 8 seen cameras
constexpr int kRec = 7 + kViews;          // doubles per record
constexpr int kCols = 5 + kViews;         // n, mean_std, rms, bad, coverage, views_0 .. views_8

enum { F_SH, F_SL, F_VH, F_VL, F_NB, F_N, F_NM, F_V0 };

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

// the reduce kernel, without and with cam_seen (photo_reduce.inc)
#define MVSGI_PHOTO_SEEN 0
#include "photo_reduce.inc"
#undef MVSGI_PHOTO_SEEN
#define MVSGI_PHOTO_SEEN 1
#include "photo_reduce.inc"
#undef MVSGI_PHOTO_SEEN

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

// both entry points: cam_seen NULL is the form without it (the kernels that never read it)
int photo_consistency(const char* what, const float* inv, const float* rays, const void* imgs, int img_kind, const float* cam_masks,
                      const float* T_host, const float* cams_host, const unsigned char* mask, int mask_per_frame, float thresh,
                      unsigned char* n_views, float* photo_var, float* photo_std, float* mean_colour, void* ws, size_t ws_bytes,
                      double* table, long long B, int N, int C, int Hr, int Wr, int H, int W, float bf, const unsigned char* cam_seen,
                      mvsgi_stream_t stream) {
    MVSGI_REQUIRE(inv && rays && imgs && T_host && cams_host, "%s: null pointer (inv, rays, imgs, T and cams are required)", what);
    MVSGI_REQUIRE(n_views || photo_var || photo_std || mean_colour || table, "%s: null pointer (every output is NULL)", what);
    if (check_view_dims(what, B, N, H, W)) return 1;
    MVSGI_REQUIRE(img_kind == U8HWC3 || img_kind == F32CHW, "%s: unknown image kind %d (0 = uint8 HWC3, 1 = fp32 CHW)", what, img_kind);
    MVSGI_REQUIRE(C >= 1, "%s: C = %d channels (need C >= 1)", what, C);
    MVSGI_REQUIRE(img_kind != U8HWC3 || C == 3, "%s: uint8 images have C = 3 channels, got C = %d", what, C);
    MVSGI_REQUIRE(Hr >= 1 && Wr >= 1, "%s: non-positive dimension (image %d x %d)", what, Hr, Wr);
    if (check_tap_offsets(what, "image", img_kind, Hr, Wr)) return 1;
    if (cam_masks && check_tap_offsets(what, "camera mask", F32CHW, Hr, Wr)) return 1;
    MVSGI_REQUIRE(dims_ok(B, H, W), "%s: map %d x %d or batch %lld too large (H * W < 2^31 - 2^18, B < 65535)", what, H, W, B);
    MVSGI_REQUIRE(mask_per_frame == 0 || mask_per_frame == 1, "%s: mask_per_frame = %d (0: [H][W], 1: [B][H][W])", what, mask_per_frame);
    MVSGI_REQUIRE(thresh == thresh, "%s: thresh is a NaN", what);
    ViewRig rig;
    if (load_view_rig(what, T_host, cams_host, N, rig)) return 1;
    MVSGI_REQUIRE(aligned(n_views, 16) && aligned(photo_var, 16) && aligned(photo_std, 16) && aligned(mean_colour, 16),
                  "%s: outputs must be 16-byte aligned", what);
    MVSGI_REQUIRE(aligned(cam_masks, 4) && (img_kind == U8HWC3 || aligned(imgs, 4)), "%s: fp32 images and masks must be 4-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (check_quad_loads(what, inv, rays, W)) return 1;
    if (vec) MVSGI_REQUIRE(aligned(mask, 4) && aligned(cam_seen, 4), "%s: mask and cam_seen must be 4-byte aligned when W %% 4 == 0", what);
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
#define MVSGI_PHOTO_SEEN_LAUNCH(IN, VEC)                                                                                         \
    do {                                                                                                                          \
        if (N <= 4)                                                                                                               \
            hipLaunchKernelGGL((photo_reduce_seen<IN, VEC, 4>), blocks, dim3(kThreads), 0, st, inv, rays, imgs, cam_masks, mask, o, rig, \
                               s, bf, thresh, kPiF, cam_seen);                                                                    \
        else                                                                                                                      \
            hipLaunchKernelGGL((photo_reduce_seen<IN, VEC, 8>), blocks, dim3(kThreads), 0, st, inv, rays, imgs, cam_masks, mask, o, rig, \
                               s, bf, thresh, kPiF, cam_seen);                                                                    \
    } while (0)
    if (!cam_seen)
        MVSGI_LAUNCH_IMAGE_KIND_VEC(MVSGI_PHOTO_LAUNCH, img_kind, vec);
    else
        MVSGI_LAUNCH_IMAGE_KIND_VEC(MVSGI_PHOTO_SEEN_LAUNCH, img_kind, vec);
#undef MVSGI_PHOTO_SEEN_LAUNCH
#undef MVSGI_PHOTO_LAUNCH
    if (mvsgi::check_launch((std::string(what) + " (reduce)").c_str())) return 1;
    if (!table) return 0;
    hipLaunchKernelGGL(photo_finalise, dim3((unsigned)B + 1u), dim3(kThreads), 0, st, slab + l.rec, slab + l.fsum, table, (int)B, l.G);
    return mvsgi::check_launch((std::string(what) + " (finalise)").c_str());
}

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
    return photo_consistency("mvsgi_photo_consistency_f32", inv, rays, imgs, img_kind, cam_masks, T_host, cams_host, mask, mask_per_frame,
                             thresh, n_views, photo_var, photo_std, mean_colour, ws, ws_bytes, table, B, N, C, Hr, Wr, H, W, bf, nullptr,
                             stream);
}

extern "C" int mvsgi_photo_consistency_seen_f32(const float* inv, const float* rays, const void* imgs, int img_kind,
                                                const float* cam_masks, const float* T_host, const float* cams_host,
                                                const unsigned char* mask, int mask_per_frame, float thresh, unsigned char* n_views,
                                                float* photo_var, float* photo_std, float* mean_colour, void* ws, size_t ws_bytes,
                                                double* table, long long B, int N, int C, int Hr, int Wr, int H, int W, float bf,
                                                const unsigned char* cam_seen, mvsgi_stream_t stream) {
    return photo_consistency("mvsgi_photo_consistency_seen_f32", inv, rays, imgs, img_kind, cam_masks, T_host, cams_host, mask,
                             mask_per_frame, thresh, n_views, photo_var, photo_std, mean_colour, ws, ws_bytes, table, B, N, C, Hr, Wr, H, W,
                             bf, cam_seen, stream);
}
