// Back-projection of the predicted inverse distance (SphericalSweepStereo._create_warped_inputs,
// dsta_mvs/model/mvs_model/spherical_sweep_stereo.py:417-471): the rig camera's point cloud and the camera images warped
// into the rig camera's view, in one launch for all frames and all cameras.  Per frame b, output pixel (i, j), camera n:
//
//   d = bf / inv[b][i][j]                                        :422  (IEEE single division)
//   p = rays[:, i, j] * d                                        :435  -> xyz[b][:, i, j]
//   q = T_n p                                                    transform_points_kernel   (grids.hip)
//   (g, in_fov) = double-sphere or equirectangular projection    grid_double_sphere_kernel / grid_equirect_kernel (grids.hip)
//   valid = in_fov & |gx| <= 1 & |gy| <= 1                       resample_validity_kernel  (resample.hip)
//   warped = valid ? bilinear_grid_sample(img[b][n], g) : invalid_value          resample_bilinear_kernel (resample.hip)
//
// The result is DEFINED as the bits of that chain of existing kernels, so the closed forms below are copies of theirs, fp32
// with contraction off, operation by operation (tests/test_gpu_reproject.py compares bit for bit and catches drift).
//
// One thread owns four consecutive pixels of a row for one camera (blockIdx.y): 16-byte loads of inv and the ray table,
// 16-byte stores per plane; rows whose length is no multiple of four take the element-wise form of the same thread shape.
// The camera table and the transforms are kernel arguments (by value, N <= 8): nothing rig-constant is loaded from memory.
// The threads of camera 0 write xyz.  The taps of an invalid pixel are never fetched.
#include "common.hpp"

namespace {

constexpr int kMaxCams = 8;          // mvsgi_sweep_max_cams()
constexpr int kCamFloats = 10;       // host camera table row: model, xi, alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1

enum ReprojModel { DOUBLE_SPHERE = 0, EQUIRECT = 1 };
enum ReprojIn { U8HWC3 = 0, F32CHW = 1, NO_IMAGES = 2 };

struct ReprojCam {
    float T[12];                                                    // rows 0..2 of the 4 x 4 transform, row-major
    float xi, alpha, one_minus_alpha, fx, fy, cx, cy, wm1, hm1, neg_w2;      // DsParams of grids.hip
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

struct Bilin {
    int o00, o01, o10, o11;     // pixel offsets y*W+x, or -1 when the tap is outside
    float w00, w01, w10, w11;   // weights of (x0,y0), (x0,y1), (x1,y0), (x1,y1)
};

// resample.hip:27-52 (K1's bilin_setup), verbatim
__device__ __forceinline__ Bilin bilin_setup(float gx, float gy, int W, int H) {
#pragma clang fp contract(off)
    Bilin t;
    // backports.py:41-42 (align_corners=False)
    const float x = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
    const float y = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
    const float xf = floorf(x), yf = floorf(y);
    const float x1f = xf + 1.0f, y1f = yf + 1.0f;
    // backports.py:52-55: weights from the unclamped coordinates
    t.w00 = (x1f - x) * (y1f - y);
    t.w01 = (x1f - x) * (y - yf);
    t.w10 = (x - xf) * (y1f - y);
    t.w11 = (x - xf) * (y - yf);
    // anything further out than one texel is outside anyway; clamping first keeps the
    // float->int conversion defined for huge or NaN coordinates
    const int x0 = (int)fminf(fmaxf(xf, -2.0f), (float)W + 1.0f);
    const int y0 = (int)fminf(fmaxf(yf, -2.0f), (float)H + 1.0f);
    const int x1 = x0 + 1, y1 = y0 + 1;
    const bool vx0 = (x0 >= 0) & (x0 < W), vx1 = (x1 >= 0) & (x1 < W);
    const bool vy0 = (y0 >= 0) & (y0 < H), vy1 = (y1 >= 0) & (y1 < H);
    t.o00 = (vx0 & vy0) ? y0 * W + x0 : -1;
    t.o01 = (vx0 & vy1) ? y1 * W + x0 : -1;
    t.o10 = (vx1 & vy0) ? y0 * W + x1 : -1;
    t.o11 = (vx1 & vy1) ? y1 * W + x1 : -1;
    return t;
}

// resample.hip:55-64 (bilin_fetch for a fp32 plane)
__device__ __forceinline__ float bilin_fetch(const float* __restrict__ plane, const Bilin& t) {
#pragma clang fp contract(off)
    // zero padding: a tap outside the image reads 0 (backports.py:58-72)
    const float i00 = t.o00 >= 0 ? plane[t.o00] : 0.0f;
    const float i01 = t.o01 >= 0 ? plane[t.o01] : 0.0f;
    const float i10 = t.o10 >= 0 ? plane[t.o10] : 0.0f;
    const float i11 = t.o11 >= 0 ? plane[t.o11] : 0.0f;
    // backports.py:86: Ia*wa + Ib*wb + Ic*wc + Id*wd, left to right
    return ((i00 * t.w00 + i01 * t.w01) + i10 * t.w10) + i11 * t.w11;
}

// resample.hip:67-74: the same for channel c of an interleaved uint8 RGB image; lut[k] = RN(k / 255.0f)
__device__ __forceinline__ float bilin_fetch_u8(const unsigned char* __restrict__ img, int c, const float* lut, const Bilin& t) {
#pragma clang fp contract(off)
    const float i00 = t.o00 >= 0 ? lut[img[t.o00 * 3 + c]] : 0.0f;
    const float i01 = t.o01 >= 0 ? lut[img[t.o01 * 3 + c]] : 0.0f;
    const float i10 = t.o10 >= 0 ? lut[img[t.o10 * 3 + c]] : 0.0f;
    const float i11 = t.o11 >= 0 ? lut[img[t.o11 * 3 + c]] : 0.0f;
    return ((i00 * t.w00 + i01 * t.w01) + i10 * t.w10) + i11 * t.w11;
}

typedef float f32x4_t __attribute__((ext_vector_type(4)));

// resample.hip:79-88: RN(k / 255.0f), k = 0..255, evaluated by the host compiler (IEEE single division)
struct U8Table {
    float v[256];
};
constexpr U8Table make_u8_table() {
    U8Table t{};
    for (int k = 0; k < 256; ++k) t.v[k] = (float)k / 255.0f;
    return t;
}
__constant__ U8Table kU8Dev = make_u8_table();

// IN: layout of the camera images, or NO_IMAGES (warped == NULL).  VEC: W % 4 == 0; otherwise element-wise with a row tail.
template <int IN, bool VEC>
__global__ __launch_bounds__(256) void reproject_kernel(const float* __restrict__ inv, const float* __restrict__ rays,
                                                        const void* __restrict__ imgs, float* __restrict__ xyz,
                                                        float* __restrict__ warped, unsigned char* __restrict__ valid,
                                                        float* __restrict__ grid, ReprojRig rig, ReprojDims s, float bf,
                                                        float invalid_value, float pi_f, int per_cam) {
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    if (IN == U8HWC3) {
        lut[threadIdx.x] = kU8Dev.v[threadIdx.x];
        __syncthreads();
    }
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
            const f32x4_t v4 = *reinterpret_cast<const f32x4_t*>(inv + b * HW + pix);
            const f32x4_t x4 = *reinterpret_cast<const f32x4_t*>(rays + pix);
            const f32x4_t y4 = *reinterpret_cast<const f32x4_t*>(rays + HW + pix);
            const f32x4_t z4 = *reinterpret_cast<const f32x4_t*>(rays + 2 * HW + pix);
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
        for (int k = 0; k < 4; ++k) {
            const float d = bf / v[k];
            px[k] = rx[k] * d, py[k] = ry[k] * d, pz[k] = rz[k] * d;
        }
    }
    if (xyz && cam == 0) {
        float* o = xyz + (b * 3) * HW + pix;
        if (VEC) {
            *reinterpret_cast<f32x4_t*>(o) = f32x4_t{px[0], px[1], px[2], px[3]};
            *reinterpret_cast<f32x4_t*>(o + HW) = f32x4_t{py[0], py[1], py[2], py[3]};
            *reinterpret_cast<f32x4_t*>(o + 2 * HW) = f32x4_t{pz[0], pz[1], pz[2], pz[3]};
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
        // step 3: grids.hip:49-50 (transform_points_kernel): matmul row (k-ordered accumulation) + translation
        const float x = fmaf(c.T[2], pz[k], fmaf(c.T[1], py[k], c.T[0] * px[k])) + c.T[3];
        const float y = fmaf(c.T[6], pz[k], fmaf(c.T[5], py[k], c.T[4] * px[k])) + c.T[7];
        const float z = fmaf(c.T[10], pz[k], fmaf(c.T[9], py[k], c.T[8] * px[k])) + c.T[11];
        bool in_fov;
        if (c.model == DOUBLE_SPHERE) {
            // step 4: grids.hip:69-78 (grid_double_sphere_kernel; torch_cuda_sweep.py:276-295)
            const float x2 = x * x, y2 = y * y, z2 = z * z;
            const float d1 = sqrtf((x2 + y2) + z2);
            const float sd = c.xi * d1 + z;
            const float d2 = sqrtf((x2 + y2) + sd * sd);
            const float t = c.alpha * d2 + c.one_minus_alpha * sd;
            gx[k] = ((c.fx / t * x + c.cx) / c.wm1) * 2.0f - 1.0f;
            gy[k] = ((c.fy / t * y + c.cy) / c.hm1) * 2.0f - 1.0f;
            in_fov = z > c.neg_w2 * d1;
        } else {
            // step 4: grids.hip:91-95 (grid_equirect_kernel; torch_cuda_sweep.py:316-332)
            const float xz = sqrtf(x * x + z * z);
            const float lon = -1.0f * atan2f(z, x);
            const float lat = atan2f(y, xz);
            gx[k] = lon / pi_f;
            gy[k] = (2.0f * lat) / pi_f;
            in_fov = true;
        }
        // step 5: resample.hip:177 (resample_validity_kernel): a NaN coordinate compares false
        ok[k] = in_fov && fabsf(gx[k]) <= 1.0f && fabsf(gy[k]) <= 1.0f;
    }

    const long long m = b * s.N + cam;                                  // image and per-camera plane of this thread
    if (grid) {
        float* o = grid + (m * HW + pix) * 2;
        if (VEC) {
            *reinterpret_cast<f32x4_t*>(o) = f32x4_t{gx[0], gy[0], gx[1], gy[1]};
            *reinterpret_cast<f32x4_t*>(o + 4) = f32x4_t{gx[2], gy[2], gx[3], gy[3]};
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

    // step 6: resample.hip:137-168 (resample_bilinear_kernel)
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
            *reinterpret_cast<f32x4_t*>(o + ch * HW) = f32x4_t{r[0], r[1], r[2], r[3]};
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

inline bool aligned16(const void* p) { return (uintptr_t)p % 16 == 0; }

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
        // tap offsets are 32-bit, as in the resampler: (y * Wr + x) * 3 + c for the interleaved bytes, y up to Hr + 1
        const long long row_bytes = (long long)Wr * (in == U8HWC3 ? 3 : 4);
        MVSGI_REQUIRE(row_bytes < (1ll << 23) && ((long long)Hr + 2) * row_bytes < (1ll << 31),
                      "%s: image %d x %d: row bytes %lld (limit 2^23) or image bytes beyond the 32-bit tap offsets", what, Hr, Wr,
                      row_bytes);
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
            MVSGI_REQUIRE(t[8] >= 1.0f && t[9] >= 1.0f, "%s: camera %d: calib shape (%g, %g) (need calib > 1)", what, k,
                          (double)t[8] + 1.0, (double)t[9] + 1.0);
            // DsParams as mvsgi_grid_double_sphere_f32 fills them (grids.hip:165)
            c.xi = t[1], c.alpha = t[2], c.one_minus_alpha = (float)(1.0 - (double)t[2]);
            c.fx = t[3], c.fy = t[4], c.cx = t[5], c.cy = t[6];
            c.neg_w2 = -t[7], c.hm1 = t[8], c.wm1 = t[9];
        }
    }
    MVSGI_REQUIRE(aligned16(xyz) && aligned16(warped) && aligned16(valid) && aligned16(grid),
                  "%s: outputs must be 16-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (vec) MVSGI_REQUIRE(aligned16(inv) && aligned16(rays), "%s: inv and rays must be 16-byte aligned when W %% 4 == 0", what);
    ReprojDims s{B, N, C, Hr, Wr, H, W, (W + 3) / 4};
    const long long nb = mvsgi::cdiv(B * H * s.Wq, 256);
    MVSGI_REQUIRE(nb < (1ll << 31), "%s: %lld blocks (B * H * W too large for one launch)", what, nb);
    const int per_cam = (warped || valid || grid) ? 1 : 0;
    const dim3 blocks((unsigned)nb, per_cam ? (unsigned)N : 1u);
    hipStream_t st = mvsgi::as_stream(stream);
#define MVSGI_REPROJECT_LAUNCH(IN, VEC)                                                                                      \
    hipLaunchKernelGGL((reproject_kernel<IN, VEC>), blocks, dim3(256), 0, st, inv, rays, imgs, xyz, warped, valid, grid, rig, s, \
                       bf, invalid_value, 3.14159274101257324f /* float32(np.pi) */, per_cam)
    if (in == U8HWC3) {
        if (vec) MVSGI_REPROJECT_LAUNCH(U8HWC3, true); else MVSGI_REPROJECT_LAUNCH(U8HWC3, false);
    } else if (in == F32CHW) {
        if (vec) MVSGI_REPROJECT_LAUNCH(F32CHW, true); else MVSGI_REPROJECT_LAUNCH(F32CHW, false);
    } else {
        if (vec) MVSGI_REPROJECT_LAUNCH(NO_IMAGES, true); else MVSGI_REPROJECT_LAUNCH(NO_IMAGES, false);
    }
#undef MVSGI_REPROJECT_LAUNCH
    return mvsgi::check_launch(what);
}
