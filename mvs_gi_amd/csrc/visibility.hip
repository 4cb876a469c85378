// Camera range images and visibility of the predicted inverse distance: the predicted surface forward-rendered into every camera,
// the nearest point kept per cell (a z-buffer), and per pixel and camera whether the pixel's own point is that nearest one.  The
// definition is in include/mvsgi.h (section "camera range images and visibility") and DESIGN.md 20; steps 1-5 are reproject.hip's
// (the same functions of camera_models.hpp), so q, the grid and valid_n are the bits of mvsgi_reproject_f32.  This file is compiled
// with contraction off.
//
//   1. fill_kernel          z2 = +inf (0x7f800000), 16 bytes per thread with an element-wise tail.
//   2. range_splat_kernel   reproject_kernel's thread shape: a thread owns four consecutive pixels of a row for one camera
//                           (blockIdx.y), 16-byte loads of inv and the ray planes, rows whose length is no multiple of four take the
//                           element-wise form.  A live, valid, unmasked pixel takes the minimum of its squared range into its cell
//                           (or its four cells, footprint 2).
//   3. visibility_kernel    the same thread shape; the test at the nearest cell, visible as one 4-byte store per thread.  With
//                           n_visible the thread loops over the cameras instead (gridDim.y = 1) and counts in a register: the
//                           stores of visible keep their shape.
//   4. range_kernel         range = sqrtf(z2), element-wise (optional).
//
// The minimum is the project's one atomic.  r2 is a sum of squares, so it is never negative and never -0, and a NaN q makes the pixel
// invalid: the fp32 bit patterns that reach a cell order like unsigned integers, +inf (an overflowed r2) is the fill value itself, and
// the minimum of a set does not depend on the order its members arrive in.  atomicMin on unsigned, result unused: a device-scope
// no-return vector atomic.  Every cell index is clamped to the buffer before it is used.
#include "common.hpp"

#include <cfloat>

namespace {

#include "camera_models.hpp"
#include "device_prims.hpp"

using mvsgi::aligned;
using mvsgi::kMaxCams;
constexpr int kCamFloats = 10;            // host camera table row, as mvsgi_reproject_f32's
constexpr unsigned kInfBits = 0x7f800000u;

enum VisModel { DOUBLE_SPHERE = 0, EQUIRECT = 1 };

struct VisCam {
    float T[12];                          // rows 0..2 of the 4 x 4 transform, row-major
    DsParams ds;                          // read when model == DOUBLE_SPHERE
    int model, pad;
};
struct VisRig {
    VisCam cam[kMaxCams];
};
struct VisDims {
    long long B;                          // frames
    int N, H, W;
    int Wq;                               // threads per map row: ceil(W / 4)
    int Hz, Wz;                           // a camera's buffer
    int mask_per_frame, footprint;
};

// steps 1, 2 of the back-projection for a thread's four pixels, and the definition's step 2: live = 0 < v <= FLT_MAX && d <= FLT_MAX
// (a NaN compares false; v = +inf would give d = 0, the rig camera's own centre); a lane past the row's end is not live
template <bool VEC>
__device__ __forceinline__ void quad_points(const float* __restrict__ inv, const float* __restrict__ rays, long long HW, long long pix,
                                            int n, float bf, bool (&live)[4], float (&px)[4], float (&py)[4], float (&pz)[4]) {
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
    for (int k = 0; k < 4; ++k) {
        const float d = back_project(bf, v[k], rx[k], ry[k], rz[k], px[k], py[k], pz[k]);
        live[k] = k < n && v[k] > 0.0f && v[k] <= FLT_MAX && d <= FLT_MAX;
    }
}

// steps 3-5 of the back-projection and the definition's step 3: the grid coordinates, the squared range; returns valid_n
__device__ __forceinline__ bool camera_view(const VisCam& c, float px, float py, float pz, float pi_f, float& gx, float& gy, float& r2) {
#pragma clang fp contract(off)
    const float x = transform_row(c.T, px, py, pz);
    const float y = transform_row(c.T + 4, px, py, pz);
    const float z = transform_row(c.T + 8, px, py, pz);
    bool in_fov = true;
    if (c.model == DOUBLE_SPHERE)
        in_fov = project_double_sphere(c.ds, x, y, z, gx, gy);
    else
        project_equirect(x, y, z, pi_f, gx, gy);
    r2 = (x * x + y * y) + z * z;
    return grid_valid(in_fov, gx, gy);
}

__device__ __forceinline__ int clamp_cell(float f, int n) { return min(max((int)f, 0), n - 1); }

// step 4: the nearest cell of a valid coordinate (|g| <= 1, so the float is in [0, n] and the conversion is exact)
__device__ __forceinline__ int nearest_cell(float g, int n) {
#pragma clang fp contract(off)
    return clamp_cell(floorf(((g + 1.0f) * (float)n) * 0.5f), n);
}

// step 5 with footprint 2: the lower of the two cells whose centres enclose the coordinate, as a float in [-1, n - 1]
__device__ __forceinline__ float lower_cell(float g, int n) {
#pragma clang fp contract(off)
    return floorf(((g + 1.0f) * (float)n - 1.0f) * 0.5f);
}

__global__ __launch_bounds__(256) void fill_kernel(unsigned* __restrict__ z2, long long count) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 4 <= count) {
        *reinterpret_cast<uint4*>(z2 + i) = uint4{kInfBits, kInfBits, kInfBits, kInfBits};
    } else {
        for (long long k = i; k < count; ++k) z2[k] = kInfBits;
    }
}

// a thread's place in the map: reproject_kernel's
struct Quad {
    long long b, pix;
    int n;
};
template <bool VEC>
__device__ __forceinline__ bool quad_of_thread(const VisDims& s, Quad& q) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= s.B * s.H * s.Wq) return false;
    const int j = (int)(idx % s.Wq) * 4;
    const long long row = idx / s.Wq;
    const int i = (int)(row % s.H);
    q.b = row / s.H;
    q.n = VEC ? 4 : min(4, s.W - j);
    q.pix = (long long)i * s.W + j;
    return true;
}

template <bool VEC>
__global__ __launch_bounds__(256) void range_splat_kernel(const float* __restrict__ inv, const float* __restrict__ rays,
                                                          const unsigned char* __restrict__ mask, unsigned* __restrict__ z2, VisRig rig,
                                                          VisDims s, float bf, float pi_f) {
#pragma clang fp contract(off)
    Quad t;
    if (!quad_of_thread<VEC>(s, t)) return;
    const int cam = (int)blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    bool live[4];
    float px[4], py[4], pz[4];
    quad_points<VEC>(inv + t.b * HW, rays, HW, t.pix, t.n, bf, live, px, py, pz);

    unsigned mw = 0x01010101u;
    if (mask) {
        const unsigned char* mb = mask + (s.mask_per_frame ? t.b * HW : 0) + t.pix;
        if (VEC) {
            mw = *reinterpret_cast<const unsigned*>(mb);
        } else {
            mw = 0u;
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < t.n) mw |= (unsigned)mb[k] << (8 * k);
        }
    }
    const VisCam& c = rig.cam[cam];
    unsigned* plane = z2 + ((t.b * s.N + cam) * s.Hz) * (long long)s.Wz;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!live[k] || ((mw >> (8 * k)) & 0xffu) == 0u) continue;
        float gx, gy, r2;
        if (!camera_view(c, px[k], py[k], pz[k], pi_f, gx, gy, r2)) continue;
        const unsigned bits = __float_as_uint(r2);
        if (s.footprint == 1) {
            atomicMin(plane + (long long)nearest_cell(gy, s.Hz) * s.Wz + nearest_cell(gx, s.Wz), bits);
        } else {
            const float x0 = lower_cell(gx, s.Wz), y0 = lower_cell(gy, s.Hz);
#pragma unroll
            for (int dy = 0; dy < 2; ++dy) {
#pragma unroll
                for (int dx = 0; dx < 2; ++dx)
                    atomicMin(plane + (long long)clamp_cell(y0 + (float)dy, s.Hz) * s.Wz + clamp_cell(x0 + (float)dx, s.Wz), bits);
            }
        }
    }
}

// LOOP: the thread takes every camera in turn and counts (gridDim.y = 1); otherwise blockIdx.y is its camera
template <bool VEC, bool LOOP>
__global__ __launch_bounds__(256) void visibility_kernel(const float* __restrict__ inv, const float* __restrict__ rays,
                                                         const float* __restrict__ z2, unsigned char* __restrict__ visible,
                                                         unsigned char* __restrict__ n_visible, VisRig rig, VisDims s, float bf, float k2,
                                                         float pi_f) {
#pragma clang fp contract(off)
    Quad t;
    if (!quad_of_thread<VEC>(s, t)) return;
    const long long HW = (long long)s.H * s.W;
    bool live[4];
    float px[4], py[4], pz[4];
    quad_points<VEC>(inv + t.b * HW, rays, HW, t.pix, t.n, bf, live, px, py, pz);

    unsigned count = 0;                                                   // byte k: the cameras that see pixel k (at most 8)
    const int cam0 = LOOP ? 0 : (int)blockIdx.y, cam1 = LOOP ? s.N : cam0 + 1;
#pragma unroll 1
    for (int cam = cam0; cam < cam1; ++cam) {
        const VisCam& c = rig.cam[cam];
        const float* plane = z2 + ((t.b * s.N + cam) * s.Hz) * (long long)s.Wz;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!live[k]) continue;
            float gx, gy, r2;
            if (!camera_view(c, px[k], py[k], pz[k], pi_f, gx, gy, r2)) continue;
            const float z = plane[(long long)nearest_cell(gy, s.Hz) * s.Wz + nearest_cell(gx, s.Wz)];
            word |= (r2 <= z * k2 ? 1u : 0u) << (8 * k);
        }
        count += word;
        if (visible) {
            unsigned char* o = visible + (t.b * s.N + cam) * HW + t.pix;
            if (VEC) {
                *reinterpret_cast<unsigned*>(o) = word;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k)
                    if (k < t.n) o[k] = (unsigned char)((word >> (8 * k)) & 0xffu);
            }
        }
    }
    if (LOOP) {
        unsigned char* o = n_visible + t.b * HW + t.pix;
        if (VEC) {
            *reinterpret_cast<unsigned*>(o) = count;
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < t.n) o[k] = (unsigned char)((count >> (8 * k)) & 0xffu);
        }
    }
}

__global__ __launch_bounds__(256) void range_kernel(const float* __restrict__ z2, float* __restrict__ range, long long count) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i + 4 <= count) {
        const f32x4 z = *reinterpret_cast<const f32x4*>(z2 + i);
        *reinterpret_cast<f32x4*>(range + i) = f32x4{sqrtf(z[0]), sqrtf(z[1]), sqrtf(z[2]), sqrtf(z[3])};
    } else {
        for (long long k = i; k < count; ++k) range[k] = sqrtf(z2[k]);
    }
}

// the checks and the rig both entry points share; 0 on success
int vis_setup(const char* what, const float* inv, const float* rays, const float* T_host, const float* cams_host, long long B, int N,
              int H, int W, int Hz, int Wz, VisRig& rig, long long& cells) {
    MVSGI_REQUIRE(inv && rays && T_host && cams_host, "%s: null pointer (inv, rays, T and cams are required)", what);
    MVSGI_REQUIRE(N >= 1 && N <= kMaxCams, "%s: N = %d cameras (need 1 <= N <= %d)", what, N, kMaxCams);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
    MVSGI_REQUIRE(Hz >= 1 && Wz >= 1, "%s: non-positive dimension (buffer %d x %d)", what, Hz, Wz);
    MVSGI_REQUIRE(Hz <= (1 << 24) && Wz <= (1 << 24), "%s: buffer %d x %d: a side above 2^24 is no exact float", what, Hz, Wz);
    MVSGI_REQUIRE((long long)H * W < (1ll << 31) && (long long)Hz * Wz < (1ll << 31) && B < (1ll << 31),
                  "%s: map %d x %d, buffer %d x %d or batch %lld too large", what, H, W, Hz, Wz, B);
    // one launch takes fewer than 2^31 blocks of 1024 cells; bounded before the product is formed (B * N < 2^34 fits, the cells need not)
    const long long plane = (long long)Hz * Wz;
    MVSGI_REQUIRE(B * N <= ((1ll << 41) - 1) / plane, "%s: B * N * Hz * Wz = %lld * %lld cells is too large for one launch (< 2^41)", what,
                  B * N, plane);
    cells = B * N * plane;
    memset(&rig, 0, sizeof(rig));
    for (int k = 0; k < N; ++k) {
        const float* t = cams_host + k * kCamFloats;
        VisCam& c = rig.cam[k];
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
    if (W % 4 == 0) MVSGI_REQUIRE(aligned(inv, 16) && aligned(rays, 16), "%s: inv and rays must be 16-byte aligned when W %% 4 == 0", what);
    MVSGI_REQUIRE(mvsgi::cdiv(B * H * ((W + 3) / 4), 256) < (1ll << 31), "%s: B * H * W too large for one launch", what);
    return 0;
}

}  // namespace

extern "C" int mvsgi_camera_range_f32(const float* inv, const float* rays, const float* T_host, const float* cams_host,
                                      const unsigned char* mask, int mask_per_frame, int footprint, float* z2, long long B, int N, int H,
                                      int W, int Hz, int Wz, float bf, mvsgi_stream_t stream) {
    const char* what = "mvsgi_camera_range_f32";
    VisRig rig;
    long long cells = 0;
    if (vis_setup(what, inv, rays, T_host, cams_host, B, N, H, W, Hz, Wz, rig, cells)) return 1;
    MVSGI_REQUIRE(z2, "%s: null pointer (z2)", what);
    MVSGI_REQUIRE(footprint == 1 || footprint == 2, "%s: footprint = %d (1: the nearest cell, 2: the four cells around the point)", what, footprint);
    MVSGI_REQUIRE(mask_per_frame == 0 || mask_per_frame == 1, "%s: mask_per_frame = %d (0: [H][W], 1: [B][H][W])", what, mask_per_frame);
    MVSGI_REQUIRE(aligned(z2, 16), "%s: z2 must be 16-byte aligned", what);
    const bool vec = W % 4 == 0;
    if (vec) MVSGI_REQUIRE(aligned(mask, 4), "%s: mask must be 4-byte aligned when W %% 4 == 0", what);
    VisDims s{B, N, H, W, (W + 3) / 4, Hz, Wz, mask_per_frame, footprint};
    hipStream_t st = mvsgi::as_stream(stream);
    unsigned* cells_u = reinterpret_cast<unsigned*>(z2);
    hipLaunchKernelGGL(fill_kernel, dim3((unsigned)mvsgi::cdiv(cells, 1024)), dim3(256), 0, st, cells_u, cells);
    if (mvsgi::check_launch("mvsgi_camera_range_f32 (fill)")) return 1;
    const dim3 blocks((unsigned)mvsgi::cdiv(B * H * s.Wq, 256), (unsigned)N);
    if (vec)
        hipLaunchKernelGGL(range_splat_kernel<true>, blocks, dim3(256), 0, st, inv, rays, mask, cells_u, rig, s, bf, kPiF);
    else
        hipLaunchKernelGGL(range_splat_kernel<false>, blocks, dim3(256), 0, st, inv, rays, mask, cells_u, rig, s, bf, kPiF);
    return mvsgi::check_launch("mvsgi_camera_range_f32 (splat)");
}

extern "C" int mvsgi_visibility_f32(const float* inv, const float* rays, const float* T_host, const float* cams_host, const float* z2,
                                    float k2, unsigned char* visible, unsigned char* n_visible, float* range, long long B, int N, int H,
                                    int W, int Hz, int Wz, float bf, mvsgi_stream_t stream) {
    const char* what = "mvsgi_visibility_f32";
    VisRig rig;
    long long cells = 0;
    if (vis_setup(what, inv, rays, T_host, cams_host, B, N, H, W, Hz, Wz, rig, cells)) return 1;
    MVSGI_REQUIRE(z2, "%s: null pointer (z2)", what);
    MVSGI_REQUIRE(visible || n_visible || range, "%s: null pointer (every output is NULL)", what);
    MVSGI_REQUIRE(k2 >= 1.0f && k2 <= FLT_MAX, "%s: k2 = %g (need 1 <= (1 + tol)^2 < inf)", what, (double)k2);
    MVSGI_REQUIRE(aligned(z2, 16) && aligned(visible, 16) && aligned(n_visible, 16) && aligned(range, 16),
                  "%s: z2 and the outputs must be 16-byte aligned", what);
    VisDims s{B, N, H, W, (W + 3) / 4, Hz, Wz, 0, 1};
    hipStream_t st = mvsgi::as_stream(stream);
    if (visible || n_visible) {
        const bool vec = W % 4 == 0;
        const unsigned nb = (unsigned)mvsgi::cdiv(B * H * s.Wq, 256);
#define MVSGI_VISIBILITY_LAUNCH(VEC, LOOP)                                                                                             \
    hipLaunchKernelGGL((visibility_kernel<VEC, LOOP>), dim3(nb, LOOP ? 1u : (unsigned)N), dim3(256), 0, st, inv, rays, z2, visible,    \
                       n_visible, rig, s, bf, k2, kPiF)
        if (n_visible) {
            if (vec) MVSGI_VISIBILITY_LAUNCH(true, true); else MVSGI_VISIBILITY_LAUNCH(false, true);
        } else {
            if (vec) MVSGI_VISIBILITY_LAUNCH(true, false); else MVSGI_VISIBILITY_LAUNCH(false, false);
        }
#undef MVSGI_VISIBILITY_LAUNCH
        if (mvsgi::check_launch("mvsgi_visibility_f32 (test)")) return 1;
    }
    if (!range) return 0;
    hipLaunchKernelGGL(range_kernel, dim3((unsigned)mvsgi::cdiv(cells, 1024)), dim3(256), 0, st, z2, range, cells);
    return mvsgi::check_launch("mvsgi_visibility_f32 (range)");
}
