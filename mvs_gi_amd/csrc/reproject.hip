// Back-projection of the predicted inverse distance (SphericalSweepStereo._create_warped_inputs,
// dsta_mvs/model/mvs_model/spherical_sweep_stereo.py:417-471): the rig camera's point cloud and the camera images warped
// into the rig camera's view, in one launch for all frames and all cameras.  Per frame b, output pixel (i, j), camera n:
//
//   d = bf / inv[b][i][j]                                        :422  (IEEE single division)
//   p = rays[:, i, j] * d                                        :435  -> xyz[b][:, i, j]
//   q = T_n p                                                    transform_row             as transform_points_kernel
//   (g, in_fov) = double-sphere or equirectangular projection    project_double_sphere / project_equirect   as grid_*_kernel
//   valid = in_fov & |gx| <= 1 & |gy| <= 1                       grid_valid                as resample_validity_kernel
//   warped = valid ? bilinear_grid_sample(img[b][n], g) : invalid_value          the stage of resample_bilinear_kernel
//
// The result is DEFINED as the bits of that chain of existing kernels.  Each step is the function those kernels call
// (camera_models.hpp, sampling.hpp), fp32 with contraction off, so the two agree by construction; tests/test_gpu_reproject.py
// compares them bit for bit all the same.
//
// One thread owns four consecutive pixels of a row for one camera (blockIdx.y): 16-byte loads of inv and the ray table,
// 16-byte stores per plane; rows whose length is no multiple of four take the element-wise form of the same thread shape.
// The camera table and the transforms are kernel arguments (by value, N <= 8): nothing rig-constant is loaded from memory.
// The threads of camera 0 write xyz.  The taps of an invalid pixel are never fetched.
//
// The rig argument and the host loop that fills it, the thread's quad (its place, its loads, its points), a point's way into a
// camera and the four validity bytes stored as one word are view_rig.hpp's, which photo.hip and visibility.hip call as well.
#include "common.hpp"

namespace {

#include "sampling.hpp"
#include "view_rig.hpp"

struct ReprojDims {
    long long B;      // frames
    int N, C, Hr, Wr, H, W;
    int Wq;           // threads per output row: ceil(W / 4)
};

// IN: layout of the camera images, or NO_IMAGES (warped == NULL).  VEC: W % 4 == 0; otherwise element-wise with a row tail.
template <int IN, bool VEC>
__global__ __launch_bounds__(256) void reproject_kernel(const float* __restrict__ inv, const float* __restrict__ rays,
                                                        const void* __restrict__ imgs, float* __restrict__ xyz,
                                                        float* __restrict__ warped, unsigned char* __restrict__ valid,
                                                        float* __restrict__ grid, ViewRig rig, ReprojDims s, float bf,
                                                        float invalid_value, float pi_f, int per_cam) {
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    stage_u8_table<IN>(lut);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= s.B * s.H * s.Wq) return;
    const Quad t = quad_at<VEC>(idx, s.H, s.W, s.Wq);
    const long long b = t.b;
    const int n = t.n;
    const int cam = (int)blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    const long long pix = t.pix(s.W);                                   // first pixel of this thread inside a plane

    // steps 1, 2: d = bf / v, p = r * d  (spherical_sweep_stereo.py:422, :435)
    float px[4], py[4], pz[4];
    quad_points<VEC>(inv + b * HW, rays, HW, pix, n, bf, px, py, pz);
    if (xyz && cam == 0) {
        float* o = xyz + (b * 3) * HW + pix;
        if (VEC) {
            *reinterpret_cast<f32x4*>(o) = f32x4{px[0], px[1], px[2], px[3]};
            *reinterpret_cast<f32x4*>(o + HW) = f32x4{py[0], py[1], py[2], py[3]};
            *reinterpret_cast<f32x4*>(o + 2 * HW) = f32x4{pz[0], pz[1], pz[2], pz[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[k] = px[k], o[HW + k] = py[k], o[2 * HW + k] = pz[k];
        }
    }
    if (!per_cam) return;

    const ViewCam& c = rig.cam[cam];
    float gx[4], gy[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        float x, y, z;                                                  // steps 3-5
        ok[k] = grid_valid(camera_view(c, px[k], py[k], pz[k], pi_f, x, y, z, gx[k], gy[k]), gx[k], gy[k]);
    }

    const long long m = b * s.N + cam;                                  // image and per-camera plane of this thread
    if (grid) {
        float* o = grid + (m * HW + pix) * 2;
        if (VEC) {
            *reinterpret_cast<f32x4*>(o) = f32x4{gx[0], gy[0], gx[1], gy[1]};
            *reinterpret_cast<f32x4*>(o + 4) = f32x4{gx[2], gy[2], gx[3], gy[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[2 * k] = gx[k], o[2 * k + 1] = gy[k];
        }
    }
    if (valid) {
        store_byte_quad<VEC>(valid + m * HW + pix, n,
                             (ok[0] ? 1u : 0u) | (ok[1] ? 0x100u : 0u) | (ok[2] ? 0x10000u : 0u) | (ok[3] ? 0x1000000u : 0u));
    }
    if (IN == NO_IMAGES) return;

    // step 6: the sampling stage of resample_bilinear_kernel
    Bilin bt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bt[k] = bilin_setup(gx[k], gy[k], s.Wr, s.Hr);
    const long long HWr = (long long)s.Hr * s.Wr;
    float* o = warped + (m * s.C) * HW + pix;                            // channel 0; + c * HW per plane
    auto channel = [&](int ch) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = invalid_value;
            if (ok[k] && k < n) {                                       // an invalid pixel's taps are not fetched
                if (IN == U8HWC3)
                    r[k] = bilin_fetch_u8(static_cast<const unsigned char*>(imgs) + m * HWr * 3, ch, lut, bt[k]);
                else
                    r[k] = bilin_fetch(static_cast<const float*>(imgs) + (m * s.C + ch) * HWr, bt[k]);
            }
        }
        if (VEC) {
            *reinterpret_cast<f32x4*>(o + ch * HW) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[ch * HW + k] = r[k];
        }
    };
    if (IN == U8HWC3) {
        channel(0), channel(1), channel(2);
    } else {
#pragma unroll 1
        for (int ch = 0; ch < s.C; ++ch) channel(ch);
    }
}

using mvsgi::aligned;

}  // namespace

extern "C" int mvsgi_reproject_f32(const float* inv, const float* rays, const void* imgs, int img_kind, const float* T_host,
                                   const float* cams_host, float* xyz, float* warped, unsigned char* valid, float* grid,
                                   long long B, int N, int C, int Hr, int Wr, int H, int W, float bf, float invalid_value,
                                   mvsgi_stream_t stream) {
    const char* what = "mvsgi_reproject_f32";
    MVSGI_REQUIRE(inv && rays && T_host && cams_host, "%s: null pointer (inv, rays, T and cams are required)", what);
    MVSGI_REQUIRE(xyz || warped || valid || grid, "%s: null pointer (every output is NULL)", what);
    if (check_view_dims(what, B, N, H, W)) return 1;
    MVSGI_REQUIRE(!warped || imgs, "%s: warped without imgs", what);
    MVSGI_REQUIRE(!imgs || warped, "%s: imgs without warped (imgs may be NULL exactly when warped is NULL)", what);
    int in = NO_IMAGES;
    if (warped) {
        MVSGI_REQUIRE(img_kind == U8HWC3 || img_kind == F32CHW, "%s: unknown image kind %d (0 = uint8 HWC3, 1 = fp32 CHW)", what, img_kind);
        in = img_kind;
        MVSGI_REQUIRE(C >= 1, "%s: C = %d channels (need C >= 1)", what, C);
        MVSGI_REQUIRE(in != U8HWC3 || C == 3, "%s: uint8 images have C = 3 channels, got C = %d", what, C);
        MVSGI_REQUIRE(Hr >= 1 && Wr >= 1, "%s: non-positive dimension (image %d x %d)", what, Hr, Wr);
        if (check_tap_offsets(what, "image", in, Hr, Wr)) return 1;
    }
    MVSGI_REQUIRE((long long)H * W < (1ll << 31) && B < (1ll << 31), "%s: map %d x %d or batch %lld too large", what, H, W, B);
    ViewRig rig;
    if (load_view_rig(what, T_host, cams_host, N, rig)) return 1;
    MVSGI_REQUIRE(aligned(xyz, 16) && aligned(warped, 16) && aligned(valid, 16) && aligned(grid, 16),
                  "%s: outputs must be 16-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (check_quad_loads(what, inv, rays, W)) return 1;
    ReprojDims s{B, N, C, Hr, Wr, H, W, (W + 3) / 4};
    const long long nb = mvsgi::cdiv(B * H * s.Wq, 256);
    MVSGI_REQUIRE(nb < (1ll << 31), "%s: %lld blocks (B * H * W too large for one launch)", what, nb);
    const int per_cam = (warped || valid || grid) ? 1 : 0;
    const dim3 blocks((unsigned)nb, per_cam ? (unsigned)N : 1u);
    hipStream_t st = mvsgi::as_stream(stream);
#define MVSGI_REPROJECT_LAUNCH(IN, VEC)                                                                                      \
    hipLaunchKernelGGL((reproject_kernel<IN, VEC>), blocks, dim3(256), 0, st, inv, rays, imgs, xyz, warped, valid, grid, rig, s, \
                       bf, invalid_value, kPiF, per_cam)
    if (in == NO_IMAGES) {
        if (vec) MVSGI_REPROJECT_LAUNCH(NO_IMAGES, true); else MVSGI_REPROJECT_LAUNCH(NO_IMAGES, false);
    } else {
        MVSGI_LAUNCH_IMAGE_KIND_VEC(MVSGI_REPROJECT_LAUNCH, in, vec);
    }
#undef MVSGI_REPROJECT_LAUNCH
    return mvsgi::check_launch(what);
}
