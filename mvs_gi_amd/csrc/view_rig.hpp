// What every kernel that looks at the prediction through the rig shares, once: the rig as a kernel argument and the host loop that
// fills it from the camera table, the thread that owns four consecutive pixels of a row (its place, its 16-byte loads of inv and the
// ray planes with their element-wise tail, its back-projected points), one point's way into one camera, the four bytes a thread
// reads or writes as one word, and the four floats or integers it stores as sixteen bytes.  The fused back-projection (reproject.hip), photometric consistency (photo.hip / photo_reduce.inc) and
// the camera range images and visibility (visibility.hip) call these, so q, the grid and valid_n of the latter two are the bits of
// mvsgi_reproject_f32 by construction, not by three texts that agree.  One exception: photo_reduce.inc keeps the text of quad_points
// and of its n_views store inline (as calls its row-tail instances became other, slower code).  fp32 with contraction
// off, like camera_models.hpp, which this includes.  Include inside the translation unit's anonymous namespace, after common.hpp.
#pragma once

#include "camera_models.hpp"

constexpr int kCamFloats = 10;       // host camera table row: model, xi, alpha, fx, fy, cx, cy, w2, calib_h - 1, calib_w - 1

enum ViewModel { DOUBLE_SPHERE = 0, EQUIRECT = 1 };

struct ViewCam {
    float T[12];                                                    // rows 0..2 of the 4 x 4 transform, row-major
    DsParams ds;                                                    // read when model == DOUBLE_SPHERE
    int model, pad;
};
struct ViewRig {                                                    // a kernel argument, by value: nothing rig-constant is loaded
    ViewCam cam[mvsgi::kMaxCams];
};

// ---- host: the checks every entry point makes with the same words, and the rig from the camera table; 0 on success ----

inline int check_view_dims(const char* what, long long B, int N, int H, int W) {
    MVSGI_REQUIRE(N >= 1 && N <= mvsgi::kMaxCams, "%s: N = %d cameras (need 1 <= N <= %d)", what, N, mvsgi::kMaxCams);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
    return 0;
}

inline int load_view_rig(const char* what, const float* T_host, const float* cams_host, int N, ViewRig& rig) {
    memset(&rig, 0, sizeof(rig));
    for (int k = 0; k < N; ++k) {
        const float* t = cams_host + k * kCamFloats;
        ViewCam& c = rig.cam[k];
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
    return 0;
}

inline int check_quad_loads(const char* what, const float* inv, const float* rays, int W) {
    if (W % 4 == 0)
        MVSGI_REQUIRE(mvsgi::aligned(inv, 16) && mvsgi::aligned(rays, 16), "%s: inv and rays must be 16-byte aligned when W %% 4 == 0", what);
    return 0;
}

// ---- device: the thread's quad.  VEC: W % 4 == 0; otherwise element-wise with a row tail ----

// a thread's place in the map [B][H][W], one thread per four consecutive pixels of a row (Wq = ceil(W / 4) threads per row): quad idx
// of B * H * Wq.  The caller checks idx against that count and forms pix where it did before this header (reproject_kernel in its
// body after the plane size, visibility.hip in its quad_of_thread): moved in here, either came out as other code
struct Quad {
    long long b;                                                    // frame
    int i, j;                                                       // row; first column
    int n;                                                          // pixels of the thread inside the row
    __device__ __forceinline__ long long pix(int W) const { return (long long)i * W + j; }    // first pixel inside a plane
};
template <bool VEC>
__device__ __forceinline__ Quad quad_at(long long idx, int H, int W, int Wq) {
    const int j = (int)(idx % Wq) * 4;
    const long long row = idx / Wq;
    return Quad{row / H, (int)(row % H), j, VEC ? 4 : min(4, W - j)};
}

// steps 1, 2 of the back-projection for the n pixels at pix of the frame inv points to (planes of HW pixels): d = bf / v, p = r * d
// (spherical_sweep_stereo.py:422, :435), and each(k, v, d) for what else a caller takes from a pixel.  A lane past the row's end has
// v = 1, r = 0.
template <bool VEC, class Each>
__device__ __forceinline__ void quad_points(const float* __restrict__ inv, const float* __restrict__ rays, long long HW, long long pix,
                                            int n, float bf, float (&px)[4], float (&py)[4], float (&pz)[4], Each each) {
#pragma clang fp contract(off)
    float v[4], rx[4], ry[4], rz[4];
    if (VEC) {
        const f32x4 v4 = *reinterpret_cast<const f32x4*>(inv + pix);
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(rays + pix);
        const f32x4 y4 = *reinterpret_cast<const f32x4*>(rays + HW + pix);
        const f32x4 z4 = *reinterpret_cast<const f32x4*>(rays + 2 * HW + pix);
#pragma unroll
        for (int k = 0; k < 4; ++k) v[k] = v4[k], rx[k] = x4[k], ry[k] = y4[k], rz[k] = z4[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < n;
            v[k] = in ? inv[pix + k] : 1.0f;
            rx[k] = in ? rays[pix + k] : 0.0f;
            ry[k] = in ? rays[HW + pix + k] : 0.0f;
            rz[k] = in ? rays[2 * HW + pix + k] : 0.0f;
        }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) each(k, v[k], back_project(bf, v[k], rx[k], ry[k], rz[k], px[k], py[k], pz[k]));
}
template <bool VEC>
__device__ __forceinline__ void quad_points(const float* __restrict__ inv, const float* __restrict__ rays, long long HW, long long pix,
                                            int n, float bf, float (&px)[4], float (&py)[4], float (&pz)[4]) {
#pragma clang fp contract(off)
    quad_points<VEC>(inv, rays, HW, pix, n, bf, px, py, pz, [](int, float, float) {});
}

// steps 3, 4 of the back-projection for one point and one camera: q = T p (transform_row, once per coordinate), then the camera's
// projection; returns in_fov.  Step 5 is the caller's grid_valid(in_fov, gx, gy).
__device__ __forceinline__ bool camera_view(const ViewCam& c, float px, float py, float pz, float pi_f, float& x, float& y, float& z,
                                            float& gx, float& gy) {
#pragma clang fp contract(off)
    x = transform_row(c.T, px, py, pz);
    y = transform_row(c.T + 4, px, py, pz);
    z = transform_row(c.T + 8, px, py, pz);
    bool in_fov = true;
    if (c.model == DOUBLE_SPHERE)
        in_fov = project_double_sphere(c.ds, x, y, z, gx, gy);
    else
        project_equirect(x, y, z, pi_f, gx, gy);
    return in_fov;
}

// four bytes of a row (a byte per pixel of the quad) as one word, byte k in bits 8 k ..: a 4-byte access, or the first n bytes one by one
template <bool VEC>
__device__ __forceinline__ unsigned load_byte_quad(const unsigned char* __restrict__ p, int n) {
    if (VEC) return *reinterpret_cast<const unsigned*>(p);
    unsigned w = 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k)
        if (k < n) w |= (unsigned)p[k] << (8 * k);
    return w;
}
template <bool VEC>
__device__ __forceinline__ void store_byte_quad(unsigned char* __restrict__ p, int n, unsigned w) {
    if (VEC) {
        *reinterpret_cast<unsigned*>(p) = w;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[k] = (unsigned char)(w >> (8 * k));
    }
}

// four floats, or four 32-bit integers, of a row at p + at (p == nullptr: an output nobody wants, nothing is stored): a 16-byte
// store, or the first n elements one by one
template <bool VEC>
__device__ __forceinline__ void store_f32_quad(float* p, long long at, int n, const float (&r)[4]) {
    if (!p) return;
    if (VEC) {
        *reinterpret_cast<f32x4*>(p + at) = f32x4{r[0], r[1], r[2], r[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[at + k] = r[k];
    }
}
template <bool VEC>
__device__ __forceinline__ void store_u32_quad(int* p, long long at, int n, const int (&r)[4]) {
    if (!p) return;
    if (VEC) {
        *reinterpret_cast<u32x4*>(p + at) = u32x4{(unsigned)r[0], (unsigned)r[1], (unsigned)r[2], (unsigned)r[3]};
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (k < n) p[at + k] = r[k];
    }
}
