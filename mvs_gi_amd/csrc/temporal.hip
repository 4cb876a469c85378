// Temporal fusion: the previous fused inverse distance of a sequence warped to the rig's new pose (a z-buffer that carries its source
// pixel) and fused with the new measurement (a gated per-pixel Kalman update).  The definition is in include/mvsgi.h (section
// "temporal fusion") and DESIGN.md 23.  Steps 1-3 of the splat are reproject.hip's and visibility.hip's (the same functions of
// view_rig.hpp and camera_models.hpp: the thread's quad and its points, the row of a transform, the equirectangular projection), so p,
// q, r2 and the grid are their bits.  Step 4, the cell of the panorama, is panorama_map.hpp's pano_cell, which tsdf.hip calls for a
// voxel centre; the thread's frame and quad (frame_quad), the pose's rows (load_pose_rows) and the host checks of the map are that
// header's too, the per-quad stores view_rig.hpp's.  This file is compiled with contraction off.
//
//   1. temporal_fill_kernel     zkey = EMPTY (+inf over the largest index), 16 bytes per thread with an element-wise tail.
//   2. temporal_splat_kernel    range_splat_kernel's thread shape: a thread owns four consecutive pixels of a row, 16-byte loads of
//                               prev_inv and the ray planes, rows whose length is no multiple of four take the element-wise form.  A live
//                               pixel whose point lands inside the map takes the minimum of its key into its cell.
//   3. temporal_fuse_kernel     the same thread shape over the target pixels: two 16-byte loads of two keys each, then the dependent
//                               gathers of the state at the key's source index, the update, and 16-byte (4-byte for the ages) stores.
//
// Two things no other file of the library does.  The transform is READ FROM DEVICE MEMORY (it changes every step, and a captured
// launch must see the value of the replay): a block never straddles frames (the grid is B * blocks-per-frame, the frame is
// blockIdx.x / blocks-per-frame: frame_quad), so the address of T[b] is uniform over the block and the twelve floats arrive by scalar
// loads.  And the minimum is atomicMin on unsigned long long, result unused: the key's upper word is the bit pattern of a positive
// finite r2, which orders like an unsigned integer, the lower word the source index, so the nearest source wins and the lower index
// among equals, in whatever order they arrive.  Every cell index is checked before it addresses the buffer; every source index read
// back from a key is clamped before the gather.
#include "common.hpp"

#include <cfloat>

namespace {

#include "device_prims.hpp"
#include "panorama_map.hpp"

using mvsgi::aligned;
typedef unsigned long long u64;
typedef u64 u64x2 __attribute__((ext_vector_type(2)));
constexpr u64 kEmpty = 0x7F800000FFFFFFFFull;
constexpr float kInf = __builtin_inff();

__global__ __launch_bounds__(256) void temporal_fill_kernel(u64* __restrict__ zkey, long long count) {
    const long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 2;
    if (i + 2 <= count) {
        *reinterpret_cast<u64x2*>(zkey + i) = u64x2{kEmpty, kEmpty};
    } else if (i < count) {
        zkey[i] = kEmpty;
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void temporal_splat_kernel(const float* __restrict__ prev_inv, const unsigned char* __restrict__ prev_age,
                                                             const float* __restrict__ rays, const float* __restrict__ T,
                                                             u64* __restrict__ zkey, FrameMap s, float bf, float au, float bu, float av,
                                                             float bv, int wrap, float pi_f) {
#pragma clang fp contract(off)
    Quad t;
    if (!frame_quad<VEC>(s, t)) return;
    const long long pix = t.pix(s.W);
    const long long HW = (long long)s.H * s.W;
    // steps 1, 2: visibility.hip's live rule through view_rig.hpp's quad, and the age
    const unsigned aw = load_byte_quad<VEC>(prev_age + t.b * HW + pix, t.n);
    bool live[4];
    float px[4], py[4], pz[4];
    quad_points<VEC>(prev_inv + t.b * HW, rays, HW, pix, t.n, bf, px, py, pz, [&](int k, float v, float d) {
        live[k] = k < t.n && ((aw >> (8 * k)) & 0xffu) != 0u && v > 0.0f && v <= FLT_MAX && d <= FLT_MAX;
    });
    float tr[12];
    load_pose_rows(T, t.b, tr);
    const PanoMap map{s.H, s.W, au, bu, av, bv, wrap};
    u64* plane = zkey + t.b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        if (!live[k]) continue;
        const float qx = transform_row(tr, px[k], py[k], pz[k]);          // step 3
        const float qy = transform_row(tr + 4, px[k], py[k], pz[k]);
        const float qz = transform_row(tr + 8, px[k], py[k], pz[k]);
        const float r2 = (qx * qx + qy * qy) + qz * qz;
        if (!(r2 > 0.0f && r2 <= FLT_MAX)) continue;
        int row, col;                                                     // step 4
        if (!pano_cell(map, qx, qy, qz, pi_f, row, col)) continue;
        const u64 key = ((u64)__float_as_uint(r2) << 32) | (u64)(unsigned)(pix + k);    // step 5
        atomicMin(plane + (long long)row * s.W + col, key);
    }
}

template <bool VEC>
__global__ __launch_bounds__(256) void temporal_fuse_kernel(const u64* __restrict__ zkey, const float* __restrict__ prev_inv,
                                                            const float* __restrict__ prev_var, const unsigned char* __restrict__ prev_age,
                                                            const float* __restrict__ cur_inv, const float* __restrict__ cur_std,
                                                            float* __restrict__ fused, float* __restrict__ var, unsigned char* __restrict__ age,
                                                            float* __restrict__ warped_inv, float* __restrict__ warped_var,
                                                            int* __restrict__ src, FrameMap s, float bf, float gate2, float q_var,
                                                            float meas_std) {
#pragma clang fp contract(off)
    Quad t;
    if (!frame_quad<VEC>(s, t)) return;
    const long long pix = t.pix(s.W);
    const long long HW = (long long)s.H * s.W;
    const long long at = t.b * HW + pix;
    const unsigned last = (unsigned)(HW - 1);
    u64 key[4];
    float m[4], sd[4];
    if (VEC) {
        const u64x2 k01 = *reinterpret_cast<const u64x2*>(zkey + at), k23 = *reinterpret_cast<const u64x2*>(zkey + at + 2);
        key[0] = k01[0], key[1] = k01[1], key[2] = k23[0], key[3] = k23[1];
        const f32x4 m4 = *reinterpret_cast<const f32x4*>(cur_inv + at);
        f32x4 s4 = f32x4{meas_std, meas_std, meas_std, meas_std};
        if (cur_std) s4 = *reinterpret_cast<const f32x4*>(cur_std + at);
#pragma unroll
        for (int k = 0; k < 4; ++k) m[k] = m4[k], sd[k] = s4[k];
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const bool in = k < t.n;
            key[k] = in ? zkey[at + k] : kEmpty;
            m[k] = in ? cur_inv[at + k] : 0.0f;
            sd[k] = in && cur_std ? cur_std[at + k] : meas_std;
        }
    }
    float of[4], ov[4], wi[4], wv[4];
    int os[4];
    unsigned oa = 0u;
    const float* pinv = prev_inv + t.b * HW;
    const float* pvar = prev_var + t.b * HW;
    const unsigned char* page = prev_age + t.b * HW;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const bool filled = key[k] != kEmpty;
        const float r2 = __uint_as_float((unsigned)(key[k] >> 32));       // step 1
        const unsigned sk = min((unsigned)key[k], last);
        const float w_inv = bf / sqrtf(r2);                               // step 2
        const float ratio = w_inv / pinv[sk];
        const float g = ratio * ratio;
        const float var_w = pvar[sk] * (g * g) + q_var;
        const unsigned a_s = page[sk];
        const bool prior = filled && var_w >= 0.0f && var_w <= FLT_MAX;   // step 3
        const float var_m = sd[k] * sd[k];                                // step 4
        const bool meas = m[k] > 0.0f && m[k] <= FLT_MAX && var_m > 0.0f && var_m <= FLT_MAX;     // step 5
        float f = m[k], v = kInf;                                         // step 6: neither
        unsigned a = 0u;
        if (meas) v = var_m, a = 1u;                                      // measurement only, or restart
        if (prior) {
            bool agree = !meas;                                           // prior only
            float K = 0.0f, e = 0.0f;
            if (meas) {
                e = m[k] - w_inv;
                const float S = var_w + var_m;
                agree = e * e <= gate2 * S;
                K = var_w / S;
            }
            if (agree) {
                f = meas ? w_inv + K * e : w_inv;
                v = meas ? var_w - K * var_w : var_w;
                a = meas ? min(a_s + 1u, 255u) : a_s;
            }
        }
        of[k] = f, ov[k] = v, oa |= a << (8 * k);
        wi[k] = filled ? w_inv : 0.0f, wv[k] = filled ? var_w : kInf, os[k] = filled ? (int)sk : -1;     // step 7
    }
    store_f32_quad<VEC>(fused, at, t.n, of);
    store_f32_quad<VEC>(var, at, t.n, ov);
    store_f32_quad<VEC>(warped_inv, at, t.n, wi);
    store_f32_quad<VEC>(warped_var, at, t.n, wv);
    if (age) store_byte_quad<VEC>(age + at, t.n, oa);
    store_u32_quad<VEC>(src, at, t.n, os);
}

// the checks both entry points share; 0 on success
int temporal_dims(const char* what, long long B, int H, int W, FrameMap& s, long long& blocks) {
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
    return check_pano_sides(what, H, W, 32, " (a key holds the source index in 32 bits)") || check_frame_launch(what, B, H, W, s, blocks);
}

}  // namespace

extern "C" int mvsgi_temporal_splat_f32(const float* prev_inv, const unsigned char* prev_age, const float* rays, const float* T,
                                        unsigned long long* zkey, long long B, int H, int W, float bf, float au, float bu, float av,
                                        float bv, int wrap, mvsgi_stream_t stream) {
    const char* what = "mvsgi_temporal_splat_f32";
    MVSGI_REQUIRE(prev_inv && prev_age && rays && T && zkey, "%s: null pointer (prev_inv, prev_age, rays, T and zkey are required)", what);
    FrameMap s;
    long long blocks = 0;
    if (temporal_dims(what, B, H, W, s, blocks)) return 1;
    if (check_pano_affine(what, au, bu, av, bv, wrap)) return 1;
    MVSGI_REQUIRE(aligned(prev_inv, 16) && aligned(prev_age, 16) && aligned(rays, 16) && aligned(T, 16) && aligned(zkey, 16),
                  "%s: prev_inv, prev_age, rays, T and zkey must be 16-byte aligned", what);
    const long long cells = B * H * (long long)W;
    MVSGI_REQUIRE(mvsgi::cdiv(cells, 512) < (1ll << 31), "%s: B * H * W = %lld cells is too large for one launch", what, cells);
    hipStream_t st = mvsgi::as_stream(stream);
    hipLaunchKernelGGL(temporal_fill_kernel, dim3((unsigned)mvsgi::cdiv(cells, 512)), dim3(256), 0, st, zkey, cells);
    if (mvsgi::check_launch("mvsgi_temporal_splat_f32 (fill)")) return 1;
    if (W % 4 == 0)
        hipLaunchKernelGGL(temporal_splat_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, prev_inv, prev_age, rays, T, zkey, s, bf, au,
                           bu, av, bv, wrap, kPiF);
    else
        hipLaunchKernelGGL(temporal_splat_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, prev_inv, prev_age, rays, T, zkey, s, bf, au,
                           bu, av, bv, wrap, kPiF);
    return mvsgi::check_launch("mvsgi_temporal_splat_f32 (splat)");
}

extern "C" int mvsgi_temporal_fuse_f32(const unsigned long long* zkey, const float* prev_inv, const float* prev_var,
                                       const unsigned char* prev_age, const float* cur_inv, const float* cur_std, float meas_std,
                                       float* fused, float* var, unsigned char* age, float* warped_inv, float* warped_var, int* src,
                                       long long B, int H, int W, float bf, float gate2, float q_var, mvsgi_stream_t stream) {
    const char* what = "mvsgi_temporal_fuse_f32";
    MVSGI_REQUIRE(zkey && prev_inv && prev_var && prev_age && cur_inv,
                  "%s: null pointer (zkey, prev_inv, prev_var, prev_age and cur_inv are required)", what);
    MVSGI_REQUIRE(fused || var || age || warped_inv || warped_var || src, "%s: null pointer (every output is NULL)", what);
    FrameMap s;
    long long blocks = 0;
    if (temporal_dims(what, B, H, W, s, blocks)) return 1;
    MVSGI_REQUIRE(gate2 > 0.0f && gate2 <= FLT_MAX, "%s: gate2 = %g (need 0 < gate^2 < inf)", what, (double)gate2);
    MVSGI_REQUIRE(q_var >= 0.0f && q_var <= FLT_MAX, "%s: q_var = %g (need 0 <= q_var < inf)", what, (double)q_var);
    MVSGI_REQUIRE(cur_std || (meas_std > 0.0f && meas_std <= FLT_MAX), "%s: meas_std = %g without cur_std (need 0 < meas_std < inf)", what,
                  (double)meas_std);
    MVSGI_REQUIRE(aligned(zkey, 16) && aligned(prev_inv, 16) && aligned(prev_var, 16) && aligned(prev_age, 16) && aligned(cur_inv, 16) &&
                      aligned(cur_std, 16),
                  "%s: zkey, the state and the measurement must be 16-byte aligned", what);
    MVSGI_REQUIRE(aligned(fused, 16) && aligned(var, 16) && aligned(age, 16) && aligned(warped_inv, 16) && aligned(warped_var, 16) &&
                      aligned(src, 16),
                  "%s: the outputs must be 16-byte aligned", what);
    const void* state[3] = {prev_inv, prev_var, prev_age};
    const void* outs[6] = {fused, var, age, warped_inv, warped_var, src};
    for (const void* o : outs)
        for (const void* p : state) MVSGI_REQUIRE(!o || o != p, "%s: an output aliases the state (the state is gathered at the source index)", what);
    hipStream_t st = mvsgi::as_stream(stream);
    if (W % 4 == 0)
        hipLaunchKernelGGL(temporal_fuse_kernel<true>, dim3((unsigned)blocks), dim3(256), 0, st, zkey, prev_inv, prev_var, prev_age, cur_inv,
                           cur_std, fused, var, age, warped_inv, warped_var, src, s, bf, gate2, q_var, meas_std);
    else
        hipLaunchKernelGGL(temporal_fuse_kernel<false>, dim3((unsigned)blocks), dim3(256), 0, st, zkey, prev_inv, prev_var, prev_age, cur_inv,
                           cur_std, fused, var, age, warped_inv, warped_var, src, s, bf, gate2, q_var, meas_std);
    return mvsgi::check_launch(what);
}
