// Camera range images and visibility of the predicted inverse distance: the predicted surface forward-rendered into every camera,
// the nearest point kept per cell (a z-buffer), and per pixel and camera whether the pixel's own point is that nearest one.  The
// definition is in include/mvsgi.h (section "camera range images and visibility") and DESIGN.md 20; steps 1-5 are reproject.hip's
// (the same functions of view_rig.hpp: the rig and its host loop, the thread's quad and its points, a point's way into a camera, the
// byte quads), so q, the grid and valid_n are the bits of mvsgi_reproject_f32.  The `live` rule and the squared range are this
// file's.  This file is compiled with contraction off.
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

#include "device_prims.hpp"
#include "view_rig.hpp"

using mvsgi::aligned;
constexpr unsigned kInfBits = 0x7f800000u;

struct VisDims {
    long long B;                          // frames
    int N, H, W;
    int Wq;                               // threads per map row: ceil(W / 4)
    int Hz, Wz;                           // a camera's buffer
    int mask_per_frame, footprint;
};

// the points of the thread's quad (view_rig.hpp) and the definition's step 2: live = 0 < v <= FLT_MAX && d <= FLT_MAX (a NaN compares
// false; v = +inf would give d = 0, the rig camera's own centre); a lane past the row's end is not live
template <bool VEC>
__device__ __forceinline__ void live_points(const float* __restrict__ inv, const float* __restrict__ rays, long long HW, long long pix,
                                            int n, float bf, bool (&live)[4], float (&px)[4], float (&py)[4], float (&pz)[4]) {
#pragma clang fp contract(off)
    quad_points<VEC>(inv, rays, HW, pix, n, bf, px, py, pz,
                     [&](int k, float v, float d) { live[k] = k < n && v > 0.0f && v <= FLT_MAX && d <= FLT_MAX; });
}

// steps 3, 4 of the back-projection (view_rig.hpp) and the definition's step 3: the grid coordinates, the squared range; returns in_fov,
// and valid_n is the caller's grid_valid of it (applied there, the kernels are the code they were)
__device__ __forceinline__ bool view_range(const ViewCam& c, float px, float py, float pz, float pi_f, float& gx, float& gy, float& r2) {
#pragma clang fp contract(off)
    float x, y, z;
    const bool in_fov = camera_view(c, px, py, pz, pi_f, x, y, z, gx, gy);
    r2 = (x * x + y * y) + z * z;
    return in_fov;
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

// a thread's place in the map: view_rig.hpp's split behind the bounds check, in the form these kernels had it (a bool and the pixel
// offset; with the check and the offset in the kernels their row-tail instances came out as other, slower code: DESIGN.md 20)
struct VisQuad {
    long long b, pix;
    int n;
};
template <bool VEC>
__device__ __forceinline__ bool quad_of_thread(const VisDims& s, VisQuad& q) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= s.B * s.H * s.Wq) return false;
    const Quad t = quad_at<VEC>(idx, s.H, s.W, s.Wq);
    q.b = t.b, q.n = t.n, q.pix = t.pix(s.W);
    return true;
}

template <bool VEC>
__global__ __launch_bounds__(256) void range_splat_kernel(const float* __restrict__ inv, const float* __restrict__ rays,
                                                          const unsigned char* __restrict__ mask, unsigned* __restrict__ z2, ViewRig rig,
                                                          VisDims s, float bf, float pi_f) {
#pragma clang fp contract(off)
    VisQuad t;
    if (!quad_of_thread<VEC>(s, t)) return;
    const int cam = (int)blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    bool live[4];
    float px[4], py[4], pz[4];
    live_points<VEC>(inv + t.b * HW, rays, HW, t.pix, t.n, bf, live, px, py, pz);

    unsigned mw = 0x01010101u;
    if (mask) mw = load_byte_quad<VEC>(mask + (s.mask_per_frame ? t.b * HW : 0) + t.pix, t.n);
    const ViewCam& c = rig.cam[cam];
    unsigned* plane = z2 + ((t.b * s.N + cam) * s.Hz) * (long long)s.Wz;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!live[k] || ((mw >> (8 * k)) & 0xffu) == 0u) continue;
        float gx, gy, r2;
        if (!grid_valid(view_range(c, px[k], py[k], pz[k], pi_f, gx, gy, r2), gx, gy)) continue;
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
                                                         unsigned char* __restrict__ n_visible, ViewRig rig, VisDims s, float bf, float k2,
                                                         float pi_f) {
#pragma clang fp contract(off)
    VisQuad t;
    if (!quad_of_thread<VEC>(s, t)) return;
    const long long HW = (long long)s.H * s.W;
    bool live[4];
    float px[4], py[4], pz[4];
    live_points<VEC>(inv + t.b * HW, rays, HW, t.pix, t.n, bf, live, px, py, pz);

    unsigned count = 0;                                                   // byte k: the cameras that see pixel k (at most 8)
    const int cam0 = LOOP ? 0 : (int)blockIdx.y, cam1 = LOOP ? s.N : cam0 + 1;
#pragma unroll 1
    for (int cam = cam0; cam < cam1; ++cam) {
        const ViewCam& c = rig.cam[cam];
        const float* plane = z2 + ((t.b * s.N + cam) * s.Hz) * (long long)s.Wz;
        unsigned word = 0;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!live[k]) continue;
            float gx, gy, r2;
            if (!grid_valid(view_range(c, px[k], py[k], pz[k], pi_f, gx, gy, r2), gx, gy)) continue;
            const float z = plane[(long long)nearest_cell(gy, s.Hz) * s.Wz + nearest_cell(gx, s.Wz)];
            word |= (r2 <= z * k2 ? 1u : 0u) << (8 * k);
        }
        count += word;
        if (visible) store_byte_quad<VEC>(visible + (t.b * s.N + cam) * HW + t.pix, t.n, word);
    }
    if (LOOP) store_byte_quad<VEC>(n_visible + t.b * HW + t.pix, t.n, count);
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
              int H, int W, int Hz, int Wz, ViewRig& rig, long long& cells) {
    MVSGI_REQUIRE(inv && rays && T_host && cams_host, "%s: null pointer (inv, rays, T and cams are required)", what);
    if (check_view_dims(what, B, N, H, W)) return 1;
    MVSGI_REQUIRE(Hz >= 1 && Wz >= 1, "%s: non-positive dimension (buffer %d x %d)", what, Hz, Wz);
    MVSGI_REQUIRE(Hz <= (1 << 24) && Wz <= (1 << 24), "%s: buffer %d x %d: a side above 2^24 is no exact float", what, Hz, Wz);
    MVSGI_REQUIRE((long long)H * W < (1ll << 31) && (long long)Hz * Wz < (1ll << 31) && B < (1ll << 31),
                  "%s: map %d x %d, buffer %d x %d or batch %lld too large", what, H, W, Hz, Wz, B);
    // one launch takes fewer than 2^31 blocks of 1024 cells; bounded before the product is formed (B * N < 2^34 fits, the cells need not)
    const long long plane = (long long)Hz * Wz;
    MVSGI_REQUIRE(B * N <= ((1ll << 41) - 1) / plane, "%s: B * N * Hz * Wz = %lld * %lld cells is too large for one launch (< 2^41)", what,
                  B * N, plane);
    cells = B * N * plane;
    if (load_view_rig(what, T_host, cams_host, N, rig) || check_quad_loads(what, inv, rays, W)) return 1;
    MVSGI_REQUIRE(mvsgi::cdiv(B * H * ((W + 3) / 4), 256) < (1ll << 31), "%s: B * H * W too large for one launch", what);
    return 0;
}

}  // namespace

extern "C" int mvsgi_camera_range_f32(const float* inv, const float* rays, const float* T_host, const float* cams_host,
                                      const unsigned char* mask, int mask_per_frame, int footprint, float* z2, long long B, int N, int H,
                                      int W, int Hz, int Wz, float bf, mvsgi_stream_t stream) {
    const char* what = "mvsgi_camera_range_f32";
    ViewRig rig;
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
    ViewRig rig;
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
