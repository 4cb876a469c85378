// The per-frame score table that csrc/metrics.hip, csrc/losses.hip and csrc/photo.hip share: float64 [B + 1][cols], row b of
// frame b, row B pooled, the same bits on every run (no atomics, no allocation, no host synchronisation).  One scheme:
//   - a thread of the reduce kernel (grid (G, B), kThreads threads) keeps its sums as compensated float64 pairs (sum_add) and its
//     counts as integers, and puts them into a record double r[REC];
//   - block_reduce_store: a wave merges by shuffles at offsets 32, 16, ..., 1, thread 0 merges waves 1, 2, 3 in that order
//     through LDS and stores the block's record into the slab [B][G][REC] records | [B][REC] frame sums (FrameSlab).  G depends
//     on the frame's size alone: frame b's records, and with them row b, do not depend on B;
//   - frame_finalise (the body of a file's finalise kernel, grid B + 1): block b sums frame b's G records in index order
//     (sum_records) -> row b; block B sums every frame the same way, one thread per frame, keeps the sums in the slab and then
//     sums them in frame order -> the pooled row.
// Every merge has the accumulator on the left: the order and the operand sides written here are what defines the table's bits.
// What is a file's own: the record's fields and their merge, the unit of work and G's rule, the row's formulas.
// Include inside the translation unit's anonymous namespace (behind common.hpp), as device_prims.hpp is.
#pragma once

constexpr int kThreads = 256;
constexpr int kWaves = kThreads / 64;

// torch.clamp: min(max(t, lo), hi), a NaN stays a NaN
__device__ __forceinline__ float clamp_nan(float t, float lo, float hi) { return t != t ? t : fminf(fmaxf(t, lo), hi); }

// (h, l) += x with the rounding error of h + x kept in l (Knuth's two-sum; h stays the plain running sum)
__device__ __forceinline__ void sum_add(double& h, double& l, double x) {
    const double t = h + x;
    const double bp = t - h;
    l += (h - (t - bp)) + (x - bp);
    h = t;
}
__device__ __forceinline__ void sum_merge(double& h, double& l, double bh, double bl) {
    sum_add(h, l, bh);
    l += bl;
}
// the pair's value; an infinite or NaN sum leaves a NaN in l, the sum is then h
__device__ __forceinline__ double sum_value(double h, double l) { return l - l == 0.0 ? h + l : h; }

__device__ __forceinline__ double shfl_down(double v, int off) { return __shfl_down(v, off, 64); }

// The slab, in doubles: [B][G][rec] records | [B][rec] frame sums (written and read by the pooled row's block)
struct FrameSlab {
    int G;
    size_t rec, fsum, total;
};

// a reduce block per units_per_block units of a frame (pixels, quads), at least one and at most max_blocks
inline FrameSlab frame_slab(long long B, long long units, int units_per_block, int max_blocks, int rec) {
    FrameSlab l;
    const long long g = mvsgi::cdiv(units, units_per_block);
    l.G = (int)(g < 1 ? 1 : g > max_blocks ? max_blocks : g);
    l.rec = 0;
    l.fsum = l.rec + (size_t)B * l.G * rec;
    l.total = l.fsum + (size_t)B * rec;
    return l;
}

// B is a grid's y extent; grid_pixels: the pixels one pass of the whole grid covers, which a 32-bit index may overshoot H * W by
inline bool frame_dims_ok(long long B, int H, int W, long long grid_pixels) {
    return B >= 1 && H >= 1 && W >= 1 && B < 65535 && (long long)H * W < (1ll << 31) - grid_pixels;
}

// The block's record from every thread's r, stored by thread 0 as record blockIdx.x of frame b's G (grid (G, B)).  merge(a, b):
// a (op)= b, field by field.  The record's address is formed by thread 0 alone, behind the barrier: formed ahead of the call it
// is scheduled into the shuffles.
template <int REC, class Merge>
__device__ __forceinline__ void block_reduce_store(double (&r)[REC], double* recs, long long b, int G, Merge merge) {
    __shared__ double red[kWaves][REC];
    const int t = threadIdx.x;
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) {
        double o[REC];
#pragma unroll
        for (int j = 0; j < REC; ++j) o[j] = shfl_down(r[j], off);
        merge(r, o);
    }
    if ((t & 63) == 0) {
#pragma unroll
        for (int j = 0; j < REC; ++j) red[t >> 6][j] = r[j];
    }
    __syncthreads();
    if (t == 0) {
        for (int w = 1; w < kWaves; ++w) merge(r, red[w]);
        double* out = recs + (b * G + blockIdx.x) * REC;
#pragma unroll
        for (int j = 0; j < REC; ++j) out[j] = r[j];
    }
}

// x (op)= count records from src, REC doubles apart, in index order; x starts as the caller set it
template <int REC, class Merge>
__device__ __forceinline__ void sum_records(const double* src, int count, double* x, Merge merge) {
    for (int g = 0; g < count; ++g) merge(x, src + (long long)g * REC);
}

// the same from zeros: what a record of sums and counts starts as
template <int REC, class Merge>
__device__ __forceinline__ void sum_records_from_zero(const double* src, int count, double* x, Merge merge) {
#pragma unroll
    for (int j = 0; j < REC; ++j) x[j] = 0.0;
    sum_records<REC>(src, count, x, merge);
}

// The finalise kernel of losses and photo: the whole body of a __global__ function of grid B + 1, kThreads threads.  merge(a, b) as
// above; row(x, row of COLS doubles, args...): the row's formulas on summed fields.  The kernels themselves stay plain functions of
// their files, under their own short names: a kernel's name is stored ahead of the code in its code object, and the longer name of
// a template instance moved photo.hip's code by 256 bytes, which alone cost photo_reduce (100 KB and more of code per instance)
// 0.4 - 0.6 % at 128 frames.
template <int REC, int COLS, class Merge, class Row, class... Args>
__device__ __forceinline__ void frame_finalise(const double* recs, double* fsum, double* __restrict__ out, int B, int G, Merge merge,
                                               Row row, Args... args) {
    const int t = threadIdx.x, b = blockIdx.x;
    double x[REC];
    if (b < B) {
        if (t == 0) {
            sum_records_from_zero<REC>(recs + (long long)b * G * REC, G, x, merge);
            row(x, out + (long long)b * COLS, args...);
        }
        return;
    }
    // the pooled row: every frame's sum as its own block computes it, then the frames in frame order
    for (int f = t; f < B; f += kThreads) {
        sum_records_from_zero<REC>(recs + (long long)f * G * REC, G, x, merge);
#pragma unroll
        for (int j = 0; j < REC; ++j) fsum[(long long)f * REC + j] = x[j];
    }
    __syncthreads();
    if (t == 0) {
        sum_records_from_zero<REC>(fsum, B, x, merge);
        row(x, out + (long long)B * COLS, args...);
    }
}
