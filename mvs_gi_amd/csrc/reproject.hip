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
#include "common.hpp"

namespace {

#include "camera_models.hpp"
#include "sampling.hpp"

using mvsgi::kMaxCams;
constexpr int kCamFloats = 10;       // host camera table row: model, xi, alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1

enum ReprojModel { DOUBLE_SPHERE = 0, EQUIRECT = 1 };

struct ReprojCam {
    float T[12];                                                    // rows 0..2 of the 4 x 4 transform, row-major
    DsParams ds;                                                    // read when model == DOUBLE_SPHERE
    int model, pad;
};
struct ReprojRig {
    ReprojCam cam[kMaxCams];
};
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
                                                        float* __restrict__ grid, ReprojRig rig, ReprojDims s, float bf,
                                                        float invalid_value, float pi_f, int per_cam) {
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    stage_u8_table<IN>(lut);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= s.B * s.H * s.Wq) return;
    const int j = (int)(idx % s.Wq) * 4;
    const long long row = idx / s.Wq;
    const int i = (int)(row % s.H);
    const long long b = row / s.H;
    const int cam = (int)blockIdx.y;
    const int n = VEC ? 4 : min(4, s.W - j);                            // pixels of this thread inside the row
    const long long HW = (long long)s.H * s.W;
    const long long pix = (long long)i * s.W + j;                       // first pixel of this thread inside a plane

    // steps 1, 2: d = bf / v, p = r * d  (spherical_sweep_stereo.py:422, :435)
    float v[4], px[4], py[4], pz[4];
    {
        float rx[4], ry[4], rz[4];
        if (VEC) {
            const f32x4 v4 = *reinterpret_cast<const f32x4*>(inv + b * HW + pix);
            const f32x4 x4 = *reinterpret_cast<const f32x4*>(rays + pix);
            const f32x4 y4 = *reinterpret_cast<const f32x4*>(rays + HW + pix);
            const f32x4 z4 = *reinterpret_cast<const f32x4*>(rays + 2 * HW + pix);
#pragma unroll
            for (int k = 0; k < 4; ++k) v[k] = v4[k], rx[k] = x4[k], ry[k] = y4[k], rz[k] = z4[k];
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool in = k < n;
                v[k] = in ? inv[b * HW + pix + k] : 1.0f;
                rx[k] = in ? rays[pix + k] : 0.0f;
                ry[k] = in ? rays[HW + pix + k] : 0.0f;
                rz[k] = in ? rays[2 * HW + pix + k] : 0.0f;
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) back_project(bf, v[k], rx[k], ry[k], rz[k], px[k], py[k], pz[k]);
    }
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

    const ReprojCam& c = rig.cam[cam];
    float gx[4], gy[4];
    bool ok[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // step 3: transform_row, once per coordinate
        const float x = transform_row(c.T, px[k], py[k], pz[k]);
        const float y = transform_row(c.T + 4, px[k], py[k], pz[k]);
        const float z = transform_row(c.T + 8, px[k], py[k], pz[k]);
        // step 4: the camera's projection
        bool in_fov = true;
        if (c.model == DOUBLE_SPHERE)
            in_fov = project_double_sphere(c.ds, x, y, z, gx[k], gy[k]);
        else
            project_equirect(x, y, z, pi_f, gx[k], gy[k]);
        // step 5: grid_valid
        ok[k] = grid_valid(in_fov, gx[k], gy[k]);
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
        unsigned char* o = valid + m * HW + pix;
        if (VEC) {
            *reinterpret_cast<unsigned*>(o) = (ok[0] ? 1u : 0u) | (ok[1] ? 0x100u : 0u) | (ok[2] ? 0x10000u : 0u) | (ok[3] ? 0x1000000u : 0u);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[k] = ok[k] ? 1 : 0;
        }
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
    MVSGI_REQUIRE(N >= 1 && N <= kMaxCams, "%s: N = %d cameras (need 1 <= N <= %d)", what, N, kMaxCams);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
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
    ReprojRig rig;
    memset(&rig, 0, sizeof(rig));
    for (int k = 0; k < N; ++k) {
        const float* t = cams_host + k * kCamFloats;
        ReprojCam& c = rig.cam[k];
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
    MVSGI_REQUIRE(aligned(xyz, 16) && aligned(warped, 16) && aligned(valid, 16) && aligned(grid, 16),
                  "%s: outputs must be 16-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (vec) MVSGI_REQUIRE(aligned(inv, 16) && aligned(rays, 16), "%s: inv and rays must be 16-byte aligned when W %% 4 == 0", what);
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
