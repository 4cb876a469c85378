// The closed forms of the sampling-grid generator (dsta_mvs/support/dataset/torch_cuda_sweep.py), once: the rigid transform,
// the double-sphere and the equirectangular projection into grid_sample coordinates, and the validity rule of the image
// sampler.  The element-wise kernels of grids.hip and resample.hip and the fused back-projection (reproject.hip) all call
// these, fp32 with contraction off and the operation order of the reference's torch expressions, so the fused kernel is the
// bits of the chain by construction.  One step is not the reference's: it writes `self.fx / t` with a Python float on the left,
// which torch evaluates as reciprocal(t) * fx (two roundings); project_double_sphere divides once (fx / t, one rounding, the
// more accurate of the two).  The mask is the reference's bit for bit, the grid its last bits only: tests/grid_exact_cases.py
// emulates this file operation by operation and tests/test_grid_exact_host.py counts the golden elements either form
// reproduces.  Include inside the translation unit's anonymous namespace.
#pragma once

constexpr float kPiF = 3.14159274101257324f;      // float32(np.pi)

// transform_3D_points_torch (torch_cuda_sweep.py:385-408): one row of p' = R p + t, t = row i of the row-major 4 x 4
// transform: matmul row (k-ordered accumulation) + translation
__device__ __forceinline__ float transform_row(const float* t, float x, float y, float z) {
#pragma clang fp contract(off)
    return fmaf(t[2], z, fmaf(t[1], y, t[0] * x)) + t[3];
}

// Back-projection of one pixel (spherical_sweep_stereo.py:422, :435): d = bf / v (an IEEE single division), p = r * d.  The
// fused back-projection (reproject.hip) and the point-cloud packer (cloud.hip) both call this, so a packed point is the
// bits of xyz.  Returns d.
__device__ __forceinline__ float back_project(float bf, float v, float rx, float ry, float rz, float& px, float& py, float& pz) {
#pragma clang fp contract(off)
    const float d = bf / v;
    px = rx * d, py = ry * d, pz = rz * d;
    return d;
}

struct DsParams {
    float xi, alpha, one_minus_alpha, fx, fy, cx, cy, wm1, hm1, neg_w2;
};

// the host's part of DoubleSphereSampleGridMaker: 1 - alpha is a Python-float difference applied as a fp32 scalar
inline DsParams make_ds_params(float xi, float alpha, float fx, float fy, float cx, float cy, int calib_h, int calib_w, float w2) {
    return DsParams{xi, alpha, (float)(1.0 - (double)alpha), fx, fy, cx, cy, (float)(calib_w - 1), (float)(calib_h - 1), -w2};
}

// DoubleSphereSampleGridMaker.make_grid (torch_cuda_sweep.py:262-298): point -> (gx, gy) in [-1, 1]; returns whether the
// point is inside the model's field of view.
__device__ __forceinline__ bool project_double_sphere(const DsParams& c, float x, float y, float z, float& gx, float& gy) {
#pragma clang fp contract(off)
    const float x2 = x * x, y2 = y * y, z2 = z * z;                      // :276-278
    const float d1 = sqrtf((x2 + y2) + z2);                             // :280
    const float s = c.xi * d1 + z;
    const float d2 = sqrtf((x2 + y2) + s * s);                          // :281
    const float t = c.alpha * d2 + c.one_minus_alpha * s;               // :283
    gx = ((c.fx / t * x + c.cx) / c.wm1) * 2.0f - 1.0f;                 // :287
    gy = ((c.fy / t * y + c.cy) / c.hm1) * 2.0f - 1.0f;                 // :288
    return z > c.neg_w2 * d1;                                           // :295
}

// EquirectangularSampleGridMaker.make_grid (torch_cuda_sweep.py:305-335): point -> (gx, gy); every point is in view.
__device__ __forceinline__ void project_equirect(float x, float y, float z, float pi_f, float& gx, float& gy) {
#pragma clang fp contract(off)
    const float xz = sqrtf(x * x + z * z);                              // :316-320
    const float lon = -1.0f * atan2f(z, x);                             // :325
    const float lat = atan2f(y, xz);                                    // :326
    gx = lon / pi_f;                                                    // :331
    gy = (2.0f * lat) / pi_f;                                           // :332
}

// validity of a sampling-table entry: inside the field of view and inside the image (a NaN coordinate compares false: invalid)
__device__ __forceinline__ bool grid_valid(bool in_fov, float gx, float gy) {
    return in_fov && fabsf(gx) <= 1.0f && fabsf(gy) <= 1.0f;
}
