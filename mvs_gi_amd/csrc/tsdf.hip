// Volumetric fusion: the predicted inverse distance integrated into a world-fixed, rolling truncated signed distance volume around the
// rig, and that volume ray-cast back into the rig's view.  The definition is in include/mvsgi.h (section "volumetric fusion") and
// DESIGN.md 24.  The row of a transform is camera_models.hpp's function, and the cell of the panorama (the equirectangular projection,
// the affine map, floor and wrap, the test) is panorama_map.hpp's pano_cell, the function temporal.hip's splat calls in its step 4, so
// a voxel centre lands in the cell a splatted point at the same place lands in.  The ray-cast's thread placement (frame_quad), the
// pose's rows (load_pose_rows) and the host checks of the map are that header's too, the per-quad stores view_rig.hpp's.  This file
// is compiled with contraction off.
//
//   1. tsdf_integrate_kernel    a thread owns two consecutive slots of a sequence's store (16 bytes: f, w, f, w), one where the
//                               sequence's slot count is odd (8-byte accesses).  Slot -> world index (floored modulus around the
//                               origin), the fresh test against the previous coverage, the centre in the rig frame, its cell of the
//                               panorama, one gather of the measurement (and of std, mask), the running weighted mean, one store.
//   2. tsdf_raycast_kernel      temporal_fuse_kernel's thread shape over the target pixels: a thread owns four consecutive pixels of
//                               a row and marches the four rays together, so four dependent 8-byte gathers are in flight per thread;
//                               the loop ends when all four have crossed or at K.
//
// The pose and the origins are READ FROM DEVICE MEMORY (a captured launch follows a moving rig): a block never straddles sequences,
// so their addresses are uniform over the block.  No atomics: every slot and every pixel has one owner.  No slot index is formed from
// device data but by a floored modulus, which lies in [0, N) whatever the origin holds; the cell of the panorama is checked on the
// floats before it addresses the measurement.
#include "common.hpp"

#include <cfloat>

namespace {

#include "device_prims.hpp"
#include "panorama_map.hpp"

using mvsgi::aligned;
typedef float f32x2 __attribute__((ext_vector_type(2)));

struct TsdfGrid {
    int Nx, Ny, Nz;
    int n;                                // slots per sequence: Nx * Ny * Nz < 2^31
    unsigned per_seq;                     // blocks per sequence
};

// i mod n, floored: in [0, n) for every i
__device__ __forceinline__ int floor_mod(int i, int n) {
    const int m = i % n;
    return m < 0 ? m + n : m;
}

struct TsdfMeasure {
    const float* inv;
    const float* std;
    const unsigned char* mask;
    PanoMap map;
    float bf;
};
struct TsdfParams {
    float vs, trunc, t2, w_max, r_min, r_max;
};

// steps 1-7 for slot e of a sequence; fw: the stored pair in, the pair to store out; returns r (0 where r2 is rejected)
__device__ __forceinline__ float integrate_voxel(int e, const TsdfGrid& g, const int (&org)[3], const int (&prev)[3], const float (&tr)[12],
                                                 const TsdfMeasure& m, const TsdfParams& p, float pi_f, f32x2& fw) {
#pragma clang fp contract(off)
    const int sx = e % g.Nx, sy = (e / g.Nx) % g.Ny, sz = e / (g.Nx * g.Ny);
    const int ix = org[0] + floor_mod(sx - org[0], g.Nx);                  // step 1
    const int iy = org[1] + floor_mod(sy - org[1], g.Ny);
    const int iz = org[2] + floor_mod(sz - org[2], g.Nz);
    const bool fresh = ix < prev[0] || ix >= prev[0] + g.Nx || iy < prev[1] || iy >= prev[1] + g.Ny || iz < prev[2] || iz >= prev[2] + g.Nz;
    const float f = fresh ? 1.0f : fw[0], w = fresh ? 0.0f : fw[1];
    fw = f32x2{f, w};
    const float cx = ((float)ix + 0.5f) * p.vs, cy = ((float)iy + 0.5f) * p.vs, cz = ((float)iz + 0.5f) * p.vs;     // step 2
    const float qx = transform_row(tr, cx, cy, cz);
    const float qy = transform_row(tr + 4, cx, cy, cz);
    const float qz = transform_row(tr + 8, cx, cy, cz);
    const float r2 = (qx * qx + qy * qy) + qz * qz;
    if (!(r2 > 0.0f && r2 <= FLT_MAX)) return 0.0f;
    const float r = sqrtf(r2);
    if (!(r >= p.r_min && r <= p.r_max)) return r;
    int row, col;                                                          // step 3
    if (!pano_cell(m.map, qx, qy, qz, pi_f, row, col)) return r;
    const long long cell = (long long)row * m.map.W + col;
    const float mv = m.inv[cell];                                          // step 4
    if (m.mask && m.mask[cell] == 0) return r;
    const float d = m.bf / mv;
    if (!(mv > 0.0f && mv <= FLT_MAX && d <= FLT_MAX)) return r;
    const float sdf = d - r;                                               // step 5
    if (sdf < -p.trunc) return r;
    const float obs = fminf(sdf, p.trunc) / p.trunc;
    float w_obs = 1.0f;                                                    // step 6
    if (m.std) {
        const float sd = m.std[cell];
        const float sig = sd * d / mv;
        w_obs = p.t2 / (p.t2 + sig * sig);
        if (!(w_obs > 0.0f && w_obs <= 1.0f)) return r;
    }
    const float Wn = w + w_obs;                                            // step 7
    fw = f32x2{(f * w + obs * w_obs) / Wn, fminf(Wn, p.w_max)};
    return r;
}

template <bool VEC>
__global__ __launch_bounds__(256) void tsdf_integrate_kernel(float* __restrict__ vol, const float* __restrict__ T,
                                                             const int* __restrict__ origin, const int* __restrict__ origin_prev,
                                                             float* __restrict__ range, TsdfGrid g, TsdfMeasure m, TsdfParams p, float pi_f) {
#pragma clang fp contract(off)
    const long long b = blockIdx.x / g.per_seq;
    const unsigned blk = blockIdx.x % g.per_seq;
    const long long first = ((long long)blk * 256 + threadIdx.x) * (VEC ? 2 : 1);
    if (first >= g.n) return;
    const int e = (int)first;
    int org[3], prev[3];                                                   // uniform over the block
    float tr[12];
#pragma unroll
    for (int k = 0; k < 3; ++k) org[k] = origin[b * 3 + k], prev[k] = origin_prev[b * 3 + k];
    load_pose_rows(T, b, tr);
    const long long HW = (long long)m.map.H * m.map.W;
    m.inv += b * HW;
    if (m.std) m.std += b * HW;
    if (m.mask) m.mask += b * HW;
    float* at = vol + (b * g.n + e) * 2;
    float* rat = range ? range + b * g.n + e : nullptr;
    if (VEC) {
        const f32x4 in = *reinterpret_cast<const f32x4*>(at);
        f32x2 a = f32x2{in[0], in[1]}, c = f32x2{in[2], in[3]};
        const float r0 = integrate_voxel(e, g, org, prev, tr, m, p, pi_f, a);
        const float r1 = integrate_voxel(e + 1, g, org, prev, tr, m, p, pi_f, c);
        *reinterpret_cast<f32x4*>(at) = f32x4{a[0], a[1], c[0], c[1]};
        if (rat) *reinterpret_cast<f32x2*>(rat) = f32x2{r0, r1};
    } else {
        f32x2 a = *reinterpret_cast<const f32x2*>(at);
        const float r0 = integrate_voxel(e, g, org, prev, tr, m, p, pi_f, a);
        *reinterpret_cast<f32x2*>(at) = a;
        if (rat) *rat = r0;
    }
}

struct RayMarch {
    float t0, step, inv_vs, w_min, bf;
    int K;
};

template <bool VEC>
__global__ __launch_bounds__(256) void tsdf_raycast_kernel(const float* __restrict__ vol, const float* __restrict__ rays,
                                                           const float* __restrict__ P, const int* __restrict__ origin,
                                                           float* __restrict__ inv, float* __restrict__ weight, int* __restrict__ steps,
                                                           TsdfGrid g, FrameMap s, RayMarch mr) {
#pragma clang fp contract(off)
    Quad t;
    if (!frame_quad<VEC>(s, t)) return;
    const long long b = t.b;
    const long long HW = (long long)s.H * s.W;
    const long long pix = t.pix(s.W);
    const long long at = b * HW + pix;
    float pr[12];                                                          // uniform over the block
    int org[3];
    load_pose_rows(P, b, pr);
#pragma unroll
    for (int k = 0; k < 3; ++k) org[k] = origin[b * 3 + k];
    const float lo[3] = {(float)org[0], (float)org[1], (float)org[2]};
    const float hi[3] = {(float)(org[0] + g.Nx), (float)(org[1] + g.Ny), (float)(org[2] + g.Nz)};
    float dx[4], dy[4], dz[4];
    if (VEC) {
        const f32x4 x4 = *reinterpret_cast<const f32x4*>(rays + pix);
        const f32x4 y4 = *reinterpret_cast<const f32x4*>(rays + HW + pix);
        const f32x4 z4 = *reinterpret_cast<const f32x4*>(rays + 2 * HW + pix);
#pragma unroll
        for (int k = 0; k < 4; ++k) dx[k] = x4[k], dy[k] = y4[k], dz[k] = z4[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < t.n;
            dx[k] = in ? rays[pix + k] : 0.0f, dy[k] = in ? rays[HW + pix + k] : 0.0f, dz[k] = in ? rays[2 * HW + pix + k] : 0.0f;
        }
    }
    float oi[4], ow[4], pf[4];
    int os[4];
    bool pv[4], done[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {                                          // step 1: the row of the transform without its translation
        const float x = dx[k], y = dy[k], z = dz[k];
        dx[k] = fmaf(pr[2], z, fmaf(pr[1], y, pr[0] * x));
        dy[k] = fmaf(pr[6], z, fmaf(pr[5], y, pr[4] * x));
        dz[k] = fmaf(pr[10], z, fmaf(pr[9], y, pr[8] * x));
        oi[k] = 0.0f, ow[k] = 0.0f, os[k] = mr.K, pf[k] = 0.0f, pv[k] = false, done[k] = k >= t.n;
    }
    const float* base = vol + b * g.n * 2;
    for (int it = 0; it < mr.K; ++it) {                              // step 2
        if (done[0] && done[1] && done[2] && done[3]) break;
        const float tk = mr.t0 + (float)it * mr.step;
        f32x2 fw[4];
        bool inside[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {                                      // the four gathers are issued before any is used
            const float gxf = floorf((pr[3] + dx[k] * tk) * mr.inv_vs);
            const float gyf = floorf((pr[7] + dy[k] * tk) * mr.inv_vs);
            const float gzf = floorf((pr[11] + dz[k] * tk) * mr.inv_vs);
            inside[k] = !done[k] && gxf >= lo[0] && gxf < hi[0] && gyf >= lo[1] && gyf < hi[1] && gzf >= lo[2] && gzf < hi[2];
            fw[k] = f32x2{0.0f, 0.0f};
            if (inside[k]) {
                const int slot = (floor_mod((int)gzf, g.Nz) * g.Ny + floor_mod((int)gyf, g.Ny)) * g.Nx + floor_mod((int)gxf, g.Nx);
                fw[k] = *reinterpret_cast<const f32x2*>(base + (long long)slot * 2);
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (done[k]) continue;
            const float f = fw[k][0], w = fw[k][1];
            const bool valid = inside[k] && w >= mr.w_min;
            if (valid && pv[k] && pf[k] > 0.0f && f <= 0.0f) {             // step 3 (pv is false at the first sample)
                const float tp = mr.t0 + (float)(it - 1) * mr.step;
                const float ts = tp + mr.step * (pf[k] / (pf[k] - f));
                oi[k] = mr.bf / ts, ow[k] = w, os[k] = it, done[k] = true;
            }
            pf[k] = f, pv[k] = valid;
        }
    }
    store_f32_quad<VEC>(inv, at, t.n, oi);
    store_f32_quad<VEC>(weight, at, t.n, ow);
    store_u32_quad<VEC>(steps, at, t.n, os);
}

// the volume's checks both entry points share; 0 on success
int tsdf_grid(const char* what, long long B, int Nx, int Ny, int Nz, TsdfGrid& g) {
    MVSGI_REQUIRE(B >= 1 && Nx >= 1 && Ny >= 1 && Nz >= 1, "%s: non-positive dimension (B = %lld, Nx = %d, Ny = %d, Nz = %d)", what, B, Nx, Ny, Nz);
    const long long n = (long long)Nx * Ny * Nz;
    MVSGI_REQUIRE((long long)Nx * Ny < (1ll << 31) && n < (1ll << 31), "%s: volume %d x %d x %d: Nx * Ny * Nz must be below 2^31", what, Nx, Ny, Nz);
    g = TsdfGrid{Nx, Ny, Nz, (int)n, 0u};
    return 0;
}

int tsdf_map(const char* what, int H, int W) {
    MVSGI_REQUIRE(H >= 1 && W >= 1, "%s: non-positive dimension (H = %d, W = %d)", what, H, W);
    return check_pano_sides(what, H, W, 31, "");
}

}  // namespace

extern "C" int mvsgi_tsdf_integrate_f32(float* vol, const float* inv, const float* std, const unsigned char* mask, const float* T,
                                        const int* origin, const int* origin_prev, float* range, long long B, int Nx, int Ny, int Nz,
                                        int H, int W, float vs, float trunc, float t2, float w_max, float r_min, float r_max, float bf,
                                        float au, float bu, float av, float bv, int wrap, mvsgi_stream_t stream) {
    const char* what = "mvsgi_tsdf_integrate_f32";
    MVSGI_REQUIRE(vol && inv && T && origin && origin_prev, "%s: null pointer (vol, inv, T, origin and origin_prev are required)", what);
    TsdfGrid g;
    if (tsdf_grid(what, B, Nx, Ny, Nz, g) || tsdf_map(what, H, W)) return 1;
    MVSGI_REQUIRE(vs > 0.0f && vs <= FLT_MAX, "%s: vs = %g (need 0 < voxel size < inf)", what, (double)vs);
    MVSGI_REQUIRE(trunc > 0.0f && trunc <= FLT_MAX && t2 > 0.0f && t2 <= FLT_MAX, "%s: trunc = %g, t2 = %g (need 0 < trunc, trunc^2 < inf)", what,
                  (double)trunc, (double)t2);
    MVSGI_REQUIRE(w_max > 0.0f && w_max <= FLT_MAX, "%s: w_max = %g (need 0 < w_max < inf)", what, (double)w_max);
    MVSGI_REQUIRE(r_min >= 0.0f && r_min < r_max && r_max <= FLT_MAX, "%s: r_min = %g, r_max = %g (need 0 <= r_min < r_max <= FLT_MAX)", what,
                  (double)r_min, (double)r_max);
    if (check_pano_affine(what, au, bu, av, bv, wrap)) return 1;
    MVSGI_REQUIRE(aligned(vol, 16) && aligned(inv, 16) && aligned(std, 16) && aligned(mask, 16) && aligned(T, 16) && aligned(origin, 16) &&
                      aligned(origin_prev, 16) && aligned(range, 16),
                  "%s: vol, inv, std, mask, T, origin, origin_prev and range must be 16-byte aligned", what);
    const bool vec = g.n % 2 == 0;
    const long long per_seq = mvsgi::cdiv(vec ? (long long)g.n / 2 : (long long)g.n, 256);
    MVSGI_REQUIRE(B <= ((1ll << 31) - 1) / per_seq, "%s: B * Nx * Ny * Nz too large for one launch (%lld sequences of %lld blocks)", what, B, per_seq);
    g.per_seq = (unsigned)per_seq;
    const TsdfMeasure m{inv, std, mask, PanoMap{H, W, au, bu, av, bv, wrap}, bf};
    const TsdfParams p{vs, trunc, t2, w_max, r_min, r_max};
    hipStream_t st = mvsgi::as_stream(stream);
    if (vec)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, dim3((unsigned)(B * per_seq)), dim3(256), 0, st, vol, T, origin, origin_prev, range, g, m, p, kPiF);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, dim3((unsigned)(B * per_seq)), dim3(256), 0, st, vol, T, origin, origin_prev, range, g, m, p, kPiF);
    return mvsgi::check_launch(what);
}

extern "C" int mvsgi_tsdf_raycast_f32(const float* vol, const float* rays, const float* P, const int* origin, float* inv, float* weight,
                                      int* steps, long long B, int Nx, int Ny, int Nz, int H, int W, float inv_vs, float t0, float step,
                                      int K, float w_min, float bf, mvsgi_stream_t stream) {
    const char* what = "mvsgi_tsdf_raycast_f32";
    MVSGI_REQUIRE(vol && rays && P && origin, "%s: null pointer (vol, rays, P and origin are required)", what);
    MVSGI_REQUIRE(inv || weight || steps, "%s: null pointer (every output is NULL)", what);
    TsdfGrid g;
    if (tsdf_grid(what, B, Nx, Ny, Nz, g) || tsdf_map(what, H, W)) return 1;
    MVSGI_REQUIRE(B <= (1ll << 62) / ((long long)g.n * 2), "%s: B * Nx * Ny * Nz too large", what);
    MVSGI_REQUIRE(K >= 1 && K <= 4096, "%s: K = %d march steps (need 1 <= K <= 4096)", what, K);
    MVSGI_REQUIRE(inv_vs > 0.0f && inv_vs <= FLT_MAX, "%s: inv_vs = %g (need 0 < 1 / voxel size < inf)", what, (double)inv_vs);
    MVSGI_REQUIRE(t0 >= 0.0f && t0 <= FLT_MAX && step > 0.0f && step <= FLT_MAX, "%s: t0 = %g, step = %g (need 0 <= t0 < inf, 0 < step < inf)", what,
                  (double)t0, (double)step);
    MVSGI_REQUIRE(w_min - w_min == 0.0f, "%s: w_min = %g must be finite", what, (double)w_min);
    MVSGI_REQUIRE(aligned(vol, 16) && aligned(rays, 16) && aligned(P, 16) && aligned(origin, 16) && aligned(inv, 16) && aligned(weight, 16) &&
                      aligned(steps, 16),
                  "%s: vol, rays, P, origin and the outputs must be 16-byte aligned", what);
    FrameMap s;
    long long blocks = 0;
    if (check_frame_launch(what, B, H, W, s, blocks)) return 1;
    const RayMarch mr{t0, step, inv_vs, w_min, bf, K};
    hipStream_t st = mvsgi::as_stream(stream);
    if (W % 4 == 0)
        hipLaunchKernelGGL(tsdf_raycast_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, vol, rays, P, origin, inv, weight, steps, g, s, mr);
    else
        hipLaunchKernelGGL(tsdf_raycast_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, vol, rays, P, origin, inv, weight, steps, g, s, mr);
    return mvsgi::check_launch(what);
}
