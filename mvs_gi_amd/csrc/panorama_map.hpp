// What the stages that look at the rig panorama through a pose read from device memory share, once: the cell of the panorama a point
// of the rig frame lands in (temporal.hip's splat, tsdf.hip's integrate: a voxel centre lands in the cell a splatted point at the same
// place lands in by construction, not by two texts that agree), the thread that owns four consecutive pixels of a row of ONE frame
// (the grid is B * blocks-per-frame, so a block never straddles frames and what it reads of frame b has a uniform address), the twelve
// floats of that frame's transform, and the host checks the entry points make with the same words.  fp32 with contraction off, like
// view_rig.hpp, which this includes.  Include inside the translation unit's anonymous namespace, after common.hpp.
#pragma once

#include "view_rig.hpp"

// the rig panorama as a map of equirectangular grid coordinates: column = floor(gx * au + bu), row = floor(gy * av + bv)
// (include/mvsgi.h, "temporal fusion"); wrap: the longitude closes
struct PanoMap {
    int H, W;
    float au, bu, av, bv;
    int wrap;
};

// q of the rig frame -> whether it lands inside the map, and then its row and column: the equirectangular projection, the affine map,
// floor, the column wrapped once, the test on the floats, the conversions
__device__ __forceinline__ bool pano_cell(const PanoMap& m, float qx, float qy, float qz, float pi_f, int& row, int& col) {
#pragma clang fp contract(off)
    float gx, gy;
    project_equirect(qx, qy, qz, pi_f, gx, gy);
    const float u = gx * m.au + m.bu, v = gy * m.av + m.bv;
    const float Wf = (float)m.W, Hf = (float)m.H;
    float fx = floorf(u);
    const float fy = floorf(v);
    if (m.wrap) {
        if (fx < 0.0f) fx += Wf;
        else if (fx >= Wf) fx -= Wf;
    }
    if (!(fx >= 0.0f && fx < Wf && fy >= 0.0f && fy < Hf)) return false;   // a NaN compares false; inside, the conversions are exact
    row = (int)fy, col = (int)fx;
    return true;
}

// a map [B][H][W] launched frame per block: blockIdx.x = b * per_frame + the block inside the frame
struct FrameMap {
    int H, W;
    int Wq;                               // threads per map row: ceil(W / 4)
    unsigned per_frame;                   // blocks per frame: ceil(H * Wq / 256)
};
// a thread's place: the frame of its block and view_rig.hpp's split of the quad index inside the frame; false past the frame's end.
// The caller forms pix where it did before this header, like view_rig.hpp's callers
template <bool VEC>
__device__ __forceinline__ bool frame_quad(const FrameMap& s, Quad& t) {
    const unsigned blk = blockIdx.x % s.per_frame;
    const long long idx = (long long)blk * 256 + threadIdx.x;
    if (idx >= (long long)s.H * s.Wq) return false;
    t = quad_at<VEC>(idx, s.H, s.W, s.Wq);
    t.b = blockIdx.x / s.per_frame;
    return true;
}

// rows 0..2 of frame b's 4 x 4 transform: uniform over the block, so the twelve floats arrive by scalar loads
__device__ __forceinline__ void load_pose_rows(const float* T, long long b, float (&tr)[12]) {
#pragma unroll
    for (int k = 0; k < 12; ++k) tr[k] = T[b * 16 + k];
}

// ---- host: the checks the entry points make with the same words; 0 on success.  The caller has checked H, W >= 1 ----

// the sides are exact floats and a cell's index fits index_bits bits (why: what holds it, appended to the message)
inline int check_pano_sides(const char* what, int H, int W, int index_bits, const char* why) {
    MVSGI_REQUIRE(H <= (1 << 24) && W <= (1 << 24), "%s: map %d x %d: a side above 2^24 is no exact float", what, H, W);
    MVSGI_REQUIRE((long long)H * W < (1ll << index_bits), "%s: map %d x %d: H * W must be below 2^%d%s", what, H, W, index_bits, why);
    return 0;
}

inline int check_frame_launch(const char* what, long long B, int H, int W, FrameMap& s, long long& blocks) {
    const int Wq = (W + 3) / 4;
    const long long per_frame = mvsgi::cdiv((long long)H * Wq, 256);
    MVSGI_REQUIRE(B <= ((1ll << 31) - 1) / per_frame, "%s: B * H * W too large for one launch (%lld frames of %lld blocks)", what, B, per_frame);
    s = FrameMap{H, W, Wq, (unsigned)per_frame};
    blocks = B * per_frame;
    return 0;
}

inline int check_pano_affine(const char* what, float au, float bu, float av, float bv, int wrap) {
    MVSGI_REQUIRE(wrap == 0 || wrap == 1, "%s: wrap = %d (0: the map's longitude ends at its edges, 1: it closes)", what, wrap);
    MVSGI_REQUIRE(au - au == 0.0f && bu - bu == 0.0f && av - av == 0.0f && bv - bv == 0.0f,
                  "%s: the affine map (au, bu, av, bv) = (%g, %g, %g, %g) must be finite", what, (double)au, (double)bu, (double)av, (double)bv);
    return 0;
}
