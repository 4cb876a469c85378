// Fisheye -> surrogate-view resampler: raw camera images sampled through a per-camera table
// (grid [T][H][W][2] in grid_sample coordinates of the raw image + validity [T][H][W]) into the fp32 planar
// [M][C][H][W] views the RGB stem reads.  The table is rig-constant (dropin/image_sampler.py builds it once with the
// kernels of grids.hip); this kernel is the per-frame part:
//
//   out = valid ? bilinear_grid_sample(img, grid, align_corners=False) : invalid_value
//
// with the arithmetic of the reference's own sampler (dsta_mvs/model/backports/backports.py:34-86), operation by
// operation and with fp contraction off, exactly as K1 (sweep.hip) evaluates it: weights from the unclamped
// coordinates, zero padding, Ia*wa + Ib*wb + Ic*wc + Id*wd summed left to right.  A uint8 image is converted as
// the facade does (api/inference_pytorch.py:58-59: .float() / 255.0) through a 256-entry table of RN(k / 255.0f).
//
// One thread owns four consecutive output pixels of a row: 32 B of grid and 4 B of validity read contiguously,
// one 16-byte store per channel plane.  Rows whose length is no multiple of four take the element-wise form of
// the same thread shape.  The taps of an invalid pixel are never fetched (its grid may be anything, NaN included).
// Image m uses table m % T: T cameras, M = frames x cameras.
#include "common.hpp"

namespace {

#include "camera_models.hpp"
#include "sampling.hpp"

constexpr U8Table kU8Host = make_u8_table();

struct ResampleDims {
    long long M;      // images
    int T, C, Hr, Wr, H, W;
    int Wq;           // threads per output row: ceil(W / 4)
};

// IN: layout of the raw images.  VEC: W % 4 == 0 (16-byte table reads and stores); otherwise element-wise with a row tail.
template <int IN, bool VEC>
__global__ __launch_bounds__(256) void resample_bilinear_kernel(const void* __restrict__ imgs, const float* __restrict__ grid,
                                                                const unsigned char* __restrict__ valid,
                                                                float* __restrict__ out, ResampleDims s, float invalid_value) {
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    stage_u8_table<IN>(lut);
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= s.M * s.H * s.Wq) return;
    const int j = (int)(idx % s.Wq) * 4;
    const long long row = idx / s.Wq;
    const int i = (int)(row % s.H);
    const long long m = row / s.H;
    const int t = (int)(m % s.T);
    const int n = VEC ? 4 : min(4, s.W - j);                            // pixels of this thread inside the row
    const long long tab = ((long long)t * s.H + i) * s.W + j;           // first table entry of this thread

    float gx[4], gy[4];
    bool ok[4];
    if (VEC) {
        const f32x4 g0 = *reinterpret_cast<const f32x4*>(grid + tab * 2);
        const f32x4 g1 = *reinterpret_cast<const f32x4*>(grid + tab * 2 + 4);
        const unsigned v = *reinterpret_cast<const unsigned*>(valid + tab);
        gx[0] = g0.x, gy[0] = g0.y, gx[1] = g0.z, gy[1] = g0.w;
        gx[2] = g1.x, gy[2] = g1.y, gx[3] = g1.z, gy[3] = g1.w;
#pragma unroll
        for (int k = 0; k < 4; ++k) ok[k] = ((v >> (8 * k)) & 0xffu) != 0;
    } else {
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = k < n && valid[tab + k] != 0;
            gx[k] = ok[k] ? grid[(tab + k) * 2] : 0.0f;
            gy[k] = ok[k] ? grid[(tab + k) * 2 + 1] : 0.0f;
        }
    }
    Bilin bt[4];
#pragma unroll
    for (int k = 0; k < 4; ++k) bt[k] = bilin_setup(gx[k], gy[k], s.Wr, s.Hr);

    const long long HWr = (long long)s.Hr * s.Wr, HW = (long long)s.H * s.W;
    float* o = out + ((m * s.C) * s.H + i) * s.W + j;                     // channel 0; + c * HW per plane
    auto channel = [&](int c) {
        float r[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            r[k] = invalid_value;
            if (ok[k]) {                                                // an invalid pixel's taps are not fetched
                if (IN == U8HWC3)
                    r[k] = bilin_fetch_u8(static_cast<const unsigned char*>(imgs) + m * HWr * 3, c, lut, bt[k]);
                else
                    r[k] = bilin_fetch(static_cast<const float*>(imgs) + (m * s.C + c) * HWr, bt[k]);
            }
        }
        if (VEC) {
            *reinterpret_cast<f32x4*>(o + c * HW) = f32x4{r[0], r[1], r[2], r[3]};
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (k < n) o[c * HW + k] = r[k];
        }
    };
    if (IN == U8HWC3) {
        channel(0), channel(1), channel(2);
    } else {
#pragma unroll 1
        for (int c = 0; c < s.C; ++c) channel(c);
    }
}

// rig validity of the resampler: ds_mask & |gx| <= 1 & |gy| <= 1 (a NaN coordinate compares false: invalid)
__global__ __launch_bounds__(256) void resample_validity_kernel(const float* __restrict__ grid, const unsigned char* __restrict__ ds_mask,
                                                                unsigned char* __restrict__ valid, long long n) {
    const long long idx = (long long)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const float gx = grid[idx * 2], gy = grid[idx * 2 + 1];
    valid[idx] = grid_valid(ds_mask[idx] != 0, gx, gy) ? 1 : 0;
}

int launch_resample(const char* what, int in, const void* imgs, const float* grid, const unsigned char* valid, float* out,
                    long long M, int T, int C, int Hr, int Wr, int H, int W, float invalid_value, mvsgi_stream_t stream) {
    MVSGI_REQUIRE(imgs && grid && valid && out, "%s: null pointer", what);
    MVSGI_REQUIRE(T >= 1, "%s: T = %d tables (need T >= 1)", what, T);
    MVSGI_REQUIRE(M >= 1 && M % T == 0, "%s: M = %lld images is no multiple of T = %d tables", what, M, T);
    MVSGI_REQUIRE(C >= 1 && Hr >= 1 && Wr >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension", what);
    if (check_tap_offsets(what, "raw image", in, Hr, Wr)) return 1;
    MVSGI_REQUIRE((long long)H * W < (1ll << 31) && M < (1ll << 31), "%s: view %d x %d or batch %lld too large", what, H, W, M);
    const bool vec = W % 4 == 0;
    if (vec)
        MVSGI_REQUIRE(((uintptr_t)grid % 16 == 0) && ((uintptr_t)out % 16 == 0) && ((uintptr_t)valid % 4 == 0),
                      "%s: grid and out must be 16-byte aligned, valid 4-byte aligned", what);
    ResampleDims s{M, T, C, Hr, Wr, H, W, (W + 3) / 4};
    const long long nb = mvsgi::cdiv(M * H * s.Wq, 256);
    MVSGI_REQUIRE(nb < (1ll << 31), "%s: %lld blocks (M * H * W too large for one launch)", what, nb);
    hipStream_t st = mvsgi::as_stream(stream);
#define MVSGI_RESAMPLE_LAUNCH(IN, VEC)                                                                                      \
    hipLaunchKernelGGL((resample_bilinear_kernel<IN, VEC>), dim3((unsigned)nb), dim3(256), 0, st, imgs, grid, valid, out, s, \
                       invalid_value)
    MVSGI_LAUNCH_IMAGE_KIND_VEC(MVSGI_RESAMPLE_LAUNCH, in, vec);
#undef MVSGI_RESAMPLE_LAUNCH
    return mvsgi::check_launch(what);
}

}  // namespace

extern "C" int mvsgi_resample_bilinear_u8_f32(const unsigned char* imgs, const float* grid, const unsigned char* valid, float* out,
                                              long long M, int T, int Hr, int Wr, int H, int W, float invalid_value,
                                              mvsgi_stream_t stream) {
    return launch_resample("mvsgi_resample_bilinear_u8_f32", U8HWC3, imgs, grid, valid, out, M, T, 3, Hr, Wr, H, W, invalid_value,
                           stream);
}

extern "C" int mvsgi_resample_bilinear_f32(const float* imgs, const float* grid, const unsigned char* valid, float* out, long long M,
                                           int T, int C, int Hr, int Wr, int H, int W, float invalid_value, mvsgi_stream_t stream) {
    return launch_resample("mvsgi_resample_bilinear_f32", F32CHW, imgs, grid, valid, out, M, T, C, Hr, Wr, H, W, invalid_value,
                           stream);
}

extern "C" int mvsgi_resample_validity_u8(const float* grid, const unsigned char* ds_mask, unsigned char* valid, long long n,
                                          mvsgi_stream_t stream) {
    MVSGI_REQUIRE(grid && ds_mask && valid, "mvsgi_resample_validity_u8: null pointer");
    const long long nb = mvsgi::cdiv(n, 256);
    MVSGI_REQUIRE(n > 0 && nb < (1ll << 31), "mvsgi_resample_validity_u8: bad element count %lld", n);
    hipLaunchKernelGGL(resample_validity_kernel, dim3((unsigned)nb), dim3(256), 0, mvsgi::as_stream(stream), grid, ds_mask, valid, n);
    return mvsgi::check_launch("mvsgi_resample_validity_u8");
}

extern "C" int mvsgi_resample_u8_table_f32(float* table256) {
    MVSGI_REQUIRE(table256, "mvsgi_resample_u8_table_f32: null pointer");
    memcpy(table256, kU8Host.v, sizeof(kU8Host.v));
    return 0;
}
