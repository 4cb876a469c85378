// Validation metrics of a batch of predictions against labels: dsta_mvs/support/loss_function/metrics.py (RMSEMetric, MAEMetric,
// BadPixelRatioMetric, SSIMMetric, each also behind InverseMetricWrapper) for every frame and pooled, forward only.  The
// definition is in include/mvsgi.h (section "validation metrics") and DESIGN.md 15; per pixel it is the reference's fp32
// arithmetic (this file is compiled with contraction off), only the accumulations are wider.
//
//   1. metrics_reduce     grid (G, B): one flat pass over a frame's preds / target / mask in quads of 16 bytes (4 of the mask), the
//                         last H * W % 4 pixels one by one; both forms from one load.  A frame is a flat run: W % 4 needs no
//                         row tail, and where H * W % 4 != 0 the frames that start off a 16-byte boundary use the same quads
//                         through 4-byte aligned loads.  The thread's record, per form: S2 = sum e^2 and S1 = sum |e| (pairs: a
//                         pair holds the sum of its fp32 addends to ~2^-100), the two counts and the four extrema (fp32 in the
//                         thread, merged by NaN-sticky min / max).
//   2. metrics_finalise   grid B: sums frame b's G records in index order -> the frame's sums (slab) and the reduction columns of
//                         row b; c1 / c2 of the SSIM from the frame's extrema, or from those of every record of the launch
//                         (extrema do not depend on an order).
//   3. metrics_ssim       grid (tiles, B, 2 forms): P and T of a 16 x 32 output tile with its 10-pixel apron are staged in LDS as
//                         fp32, the horizontal 11-tap pass of {P, T, PP, TT, PT} goes to LDS in float64, the vertical pass reads it
//                         back; the tile's sum of the map goes to the slab.  LDS rows are 32 consecutive doubles (or 42 floats read
//                         by 32 consecutive lanes): a half-wave always touches consecutive addresses, no bank is hit twice.
//   4. metrics_last       grid B + 1: block b sums frame b's tile sums (fixed order); block B the pooled row from the frames' sums
//                         in frame order.
// The records, the slab's first two parts and the merge order are csrc/frame_reduce.hpp's (G = ceil(H * W / 4096), at most 64); the
// two finalising kernels are this file's own: they carry two forms, the extrema and the SSIM tiles.
#include "common.hpp"

namespace {

#include "frame_reduce.hpp"

using mvsgi::aligned;
constexpr int kMaxReduceBlocks = 64;      // records per frame (what metrics_finalise sums in order)
constexpr int kPixPerBlock = 4096;        // a reduce block covers at least this many pixels, while there are fewer than the cap
constexpr int kFields = 10;               // per form: S2 hi, S2 lo, S1 hi, S1 lo, NB, n, minP, maxP, minT, maxT
constexpr int kRec = 2 * kFields;         // doubles per record: [form][field]
constexpr int kTaps = 11;
constexpr int kTileH = 16, kTileW = 32;   // SSIM output pixels per block
constexpr int kInH = kTileH + kTaps - 1, kInW = kTileW + kTaps - 1;

enum { F_S2H, F_S2L, F_S1H, F_S1L, F_NB, F_N, F_MINP, F_MAXP, F_MINT, F_MAXT };

struct Params {
    float lo, hi, bf, cmin, cmax, thresh[2];
    int mask_kind;
};

// four floats that need only a float's alignment (a frame of H * W % 4 != 0 pixels starts anywhere)
struct __attribute__((packed, aligned(4))) quad {
    float x, y, z, w;
};

struct Gauss {
    double w[kTaps];
};

// The slab, in doubles: FrameSlab's two parts | [B][2 forms][c1, c2] | [2 forms][B][T] tile sums
struct Layout : FrameSlab {
    int tx, ty, T;
    size_t consts, tiles;
};

inline Layout layout(int B, int H, int W) {
    Layout l;
    // a reduce block per kPixPerBlock pixels of a frame
    static_cast<FrameSlab&>(l) = frame_slab(B, (long long)H * W, kPixPerBlock, kMaxReduceBlocks, kRec);
    l.ty = H >= kTaps && W >= kTaps ? (int)mvsgi::cdiv(H - kTaps + 1, kTileH) : 0;
    l.tx = H >= kTaps && W >= kTaps ? (int)mvsgi::cdiv(W - kTaps + 1, kTileW) : 0;
    l.T = l.tx * l.ty;
    l.consts = l.total;
    l.tiles = l.consts + (size_t)B * 4;
    l.total = l.tiles + (size_t)2 * B * l.T;
    return l;
}

// MVSMetric.clamp_and_scale (form 0), behind InverseMetricWrapper's 1 / x (form 1)
__device__ __forceinline__ void scaled(int form, float p, float t, const Params& k, float& P, float& T) {
    if (form) {
        p = 1.0f / p;
        t = 1.0f / t;
    }
    P = p / k.bf;
    T = clamp_nan(t, k.cmin, k.cmax) / k.bf;
}

// extrema in which a NaN sticks (torch.min / torch.max)
__device__ __forceinline__ float min_nan(float m, float v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ float max_nan(float m, float v) { return (v > m || v != v) ? v : m; }
__device__ __forceinline__ double dmin_nan(double m, double v) { return (v < m || v != v) ? v : m; }
__device__ __forceinline__ double dmax_nan(double m, double v) { return (v > m || v != v) ? v : m; }

struct Acc {
    double s2h[2], s2l[2], s1h[2], s1l[2];
    unsigned nb[2], n;
    float mnP[2], mxP[2], mnT[2], mxT[2];
};

__device__ __forceinline__ void pixel(Acc& a, float p, float t, unsigned m, const Params& k) {
    const bool v = k.mask_kind == 0 ? true : k.mask_kind == 1 ? m != 0 : (t >= k.lo && t <= k.hi);
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        float P, T;
        scaled(f, p, t, k, P, T);
        a.mnP[f] = min_nan(a.mnP[f], P);
        a.mxP[f] = max_nan(a.mxP[f], P);
        a.mnT[f] = min_nan(a.mnT[f], T);
        a.mxT[f] = max_nan(a.mxT[f], T);
        if (v) {                                   // a select: a NaN at an invalid pixel never reaches a sum
            const float e = P - T;
            const float ab = fabsf(e);
            const float s = e * e;
            sum_add(a.s2h[f], a.s2l[f], (double)s);
            sum_add(a.s1h[f], a.s1l[f], (double)ab);
            a.nb[f] += ab > k.thresh[f] ? 1u : 0u;
        }
    }
    a.n += v ? 1u : 0u;
}

// the fields of one form: x (op)= y
__device__ __forceinline__ void form_merge(double* x, const double* y) {
    sum_merge(x[F_S2H], x[F_S2L], y[F_S2H], y[F_S2L]);
    sum_merge(x[F_S1H], x[F_S1L], y[F_S1H], y[F_S1L]);
    x[F_NB] += y[F_NB];
    x[F_N] += y[F_N];
    x[F_MINP] = dmin_nan(x[F_MINP], y[F_MINP]);
    x[F_MAXP] = dmax_nan(x[F_MAXP], y[F_MAXP]);
    x[F_MINT] = dmin_nan(x[F_MINT], y[F_MINT]);
    x[F_MAXT] = dmax_nan(x[F_MAXT], y[F_MAXT]);
}

// field j of record a (op)= field j of record b
struct RecMerge {
    __device__ __forceinline__ void operator()(double* a, const double* b) const {
#pragma unroll
        for (int f = 0; f < 2; ++f) form_merge(a + f * kFields, b + f * kFields);
    }
};

__global__ __launch_bounds__(kThreads) void metrics_reduce(const float* __restrict__ preds, const float* __restrict__ target,
                                                           const unsigned char* __restrict__ mask, double* __restrict__ recs,
                                                           int npix, Params k) {
    const int t = threadIdx.x, b = blockIdx.y, G = gridDim.x;
    const long long base = (long long)b * npix;
    const float* pb = preds + base;
    const float* tb = target + base;
    const unsigned char* mb = k.mask_kind == 1 ? mask + base : nullptr;
    Acc a;
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        a.s2h[f] = a.s2l[f] = a.s1h[f] = a.s1l[f] = 0.0;
        a.nb[f] = 0;
        a.mnP[f] = a.mnT[f] = __builtin_inff();
        a.mxP[f] = a.mxT[f] = -__builtin_inff();
    }
    a.n = 0;
    const int step = G * kThreads;
    // quads [4q, 4q + 4) of the frame: 16 bytes per load.  With H * W % 4 != 0 a frame need not start 16-byte aligned; the quads
    // are the same ones (the assignment of pixels to threads depends on the frame's size alone), only the load is then a
    // 4-byte aligned one.  The last H * W % 4 pixels: one each for the first threads of block 0.
    const int nq = npix >> 2;
    for (int q = blockIdx.x * kThreads + t; q < nq; q += step) {
        const quad p = *reinterpret_cast<const quad*>(pb + 4ll * q);
        const quad g = *reinterpret_cast<const quad*>(tb + 4ll * q);
        unsigned m = 0u;
        if (mb) __builtin_memcpy(&m, mb + 4ll * q, 4);
        pixel(a, p.x, g.x, m & 0xffu, k);
        pixel(a, p.y, g.y, (m >> 8) & 0xffu, k);
        pixel(a, p.z, g.z, (m >> 16) & 0xffu, k);
        pixel(a, p.w, g.w, m >> 24, k);
    }
    if (blockIdx.x == 0 && t < (npix & 3)) {
        const int i = 4 * nq + t;
        pixel(a, pb[i], tb[i], mb ? mb[i] : 0u, k);
    }
    double r[kRec];
#pragma unroll
    for (int f = 0; f < 2; ++f) {
        double* x = r + f * kFields;
        x[F_S2H] = a.s2h[f];
        x[F_S2L] = a.s2l[f];
        x[F_S1H] = a.s1h[f];
        x[F_S1L] = a.s1l[f];
        x[F_NB] = (double)a.nb[f];
        x[F_N] = (double)a.n;
        x[F_MINP] = (double)a.mnP[f];
        x[F_MAXP] = (double)a.mxP[f];
        x[F_MINT] = (double)a.mnT[f];
        x[F_MAXT] = (double)a.mxT[f];
    }
    block_reduce_store<kRec>(r, recs, b, G, RecMerge());
}

// threads 0 and 1 (form f): count records of kRec doubles from src, in index order -> dst[f * kFields ...]
__device__ __forceinline__ void sum_form(const double* __restrict__ src, int count, double* dst, int f) {
    double x[kFields];
    x[F_S2H] = x[F_S2L] = x[F_S1H] = x[F_S1L] = x[F_NB] = x[F_N] = 0.0;
    x[F_MINP] = x[F_MINT] = __builtin_inf();
    x[F_MAXP] = x[F_MAXT] = -__builtin_inf();
    sum_records<kRec>(src, count, x, [f](double* a, const double* rec) { form_merge(a, rec + f * kFields); });
#pragma unroll
    for (int j = 0; j < kFields; ++j) dst[f * kFields + j] = x[j];
}

// the reduction columns of one row of the table from summed fields x (form f); n_bad: the divisor of the unmasked bad-pixel ratio
__device__ __forceinline__ void write_row(const double* x, double* row, int f, int mask_kind, double n_bad) {
    const double n = x[F_N];
    row[4 * f + 0] = sqrt(sum_value(x[F_S2H], x[F_S2L]) / n);
    row[4 * f + 1] = sum_value(x[F_S1H], x[F_S1L]) / n;
    row[4 * f + 2] = mask_kind == 0 ? x[F_NB] / n_bad : (n > 0.0 ? x[F_NB] / n : 1.0);
    if (f == 0) row[8] = n;
}

__global__ __launch_bounds__(kThreads) void metrics_finalise(const double* __restrict__ recs, double* __restrict__ fsum,
                                                             double* __restrict__ consts, double* __restrict__ out, int B, int G,
                                                             int npix, int mask_kind, int batch_scope) {
    __shared__ double sh[kRec];
    __shared__ double ext[kWaves][8];
    const int t = threadIdx.x, b = blockIdx.x;
    if (t < 2) {
        sum_form(recs + (long long)b * G * kRec, G, sh, t);
        for (int j = 0; j < kFields; ++j) fsum[(long long)b * kRec + t * kFields + j] = sh[t * kFields + j];
        write_row(sh + t * kFields, out + (long long)b * 9, t, mask_kind, (double)npix);
    }
    if (batch_scope) {       // the extrema of every record of the launch: any order gives the same value
        double e[8];
#pragma unroll
        for (int f = 0; f < 2; ++f) {
            e[4 * f + 0] = e[4 * f + 2] = __builtin_inf();
            e[4 * f + 1] = e[4 * f + 3] = -__builtin_inf();
        }
        const long long nrec = (long long)B * G;
        for (long long r = t; r < nrec; r += kThreads) {
#pragma unroll
            for (int f = 0; f < 2; ++f) {
                const double* y = recs + r * kRec + f * kFields;
                e[4 * f + 0] = dmin_nan(e[4 * f + 0], y[F_MINP]);
                e[4 * f + 1] = dmax_nan(e[4 * f + 1], y[F_MAXP]);
                e[4 * f + 2] = dmin_nan(e[4 * f + 2], y[F_MINT]);
                e[4 * f + 3] = dmax_nan(e[4 * f + 3], y[F_MAXT]);
            }
        }
#pragma unroll
        for (int off = 32; off >= 1; off >>= 1) {
#pragma unroll
            for (int j = 0; j < 8; ++j) {
                const double o = shfl_down(e[j], off);
                e[j] = (j & 1) ? dmax_nan(e[j], o) : dmin_nan(e[j], o);
            }
        }
        if ((t & 63) == 0) {
#pragma unroll
            for (int j = 0; j < 8; ++j) ext[t >> 6][j] = e[j];
        }
    }
    __syncthreads();
    if (t < 2) {
        double mnP = sh[t * kFields + F_MINP], mxP = sh[t * kFields + F_MAXP];
        double mnT = sh[t * kFields + F_MINT], mxT = sh[t * kFields + F_MAXT];
        if (batch_scope) {
            mnP = ext[0][4 * t + 0], mxP = ext[0][4 * t + 1], mnT = ext[0][4 * t + 2], mxT = ext[0][4 * t + 3];
            for (int w = 1; w < kWaves; ++w) {
                mnP = dmin_nan(mnP, ext[w][4 * t + 0]);
                mxP = dmax_nan(mxP, ext[w][4 * t + 1]);
                mnT = dmin_nan(mnT, ext[w][4 * t + 2]);
                mxT = dmax_nan(mxT, ext[w][4 * t + 3]);
            }
        }
        const double R = dmax_nan(mxP - mnP, mxT - mnT);
        const double a1 = 0.01 * R, a2 = 0.03 * R;
        consts[(long long)b * 4 + 2 * t + 0] = a1 * a1;
        consts[(long long)b * 4 + 2 * t + 1] = a2 * a2;
    }
}

// sum over the block of one double per thread, in a fixed order; valid in thread 0
__device__ __forceinline__ double block_sum(double v, double* sh) {
#pragma unroll
    for (int off = 32; off >= 1; off >>= 1) v += shfl_down(v, off);
    if ((threadIdx.x & 63) == 0) sh[threadIdx.x >> 6] = v;
    __syncthreads();
    if (threadIdx.x == 0)
        for (int w = 1; w < kWaves; ++w) v += sh[w];
    return v;
}

__global__ __launch_bounds__(kThreads) void metrics_ssim(const float* __restrict__ preds, const float* __restrict__ target,
                                                         const double* __restrict__ consts, double* __restrict__ tiles, int B,
                                                         int H, int W, int tx, Params k, Gauss g) {
    __shared__ float sP[kInH][kInW], sT[kInH][kInW];
    __shared__ double hb[5][kInH][kTileW];
    __shared__ double red[kWaves];
    const int t = threadIdx.x, tile = blockIdx.x, b = blockIdx.y, form = blockIdx.z;
    const int i0 = (tile / tx) * kTileH, j0 = (tile % tx) * kTileW;
    const long long base = (long long)b * H * W;
    // P and T of the tile's input window; behind the image's edge zeros, which only reach outputs that are not counted
    for (int idx = t; idx < kInH * kInW; idx += kThreads) {
        const int r = idx / kInW, c = idx - r * kInW;
        const int gi = i0 + r, gj = j0 + c;
        float P = 0.f, T = 0.f;
        if (gi < H && gj < W) {
            const long long o = base + (long long)gi * W + gj;
            scaled(form, preds[o], target[o], k, P, T);
        }
        sP[r][c] = P;
        sT[r][c] = T;
    }
    __syncthreads();
    for (int it = t; it < kInH * kTileW; it += kThreads) {
        const int r = it / kTileW, c = it % kTileW;
        double mP = 0.0, mT = 0.0, mPP = 0.0, mTT = 0.0, mPT = 0.0;
#pragma unroll
        for (int u = 0; u < kTaps; ++u) {
            const double p = (double)sP[r][c + u], q = (double)sT[r][c + u], w = g.w[u];
            mP = fma(w, p, mP);
            mT = fma(w, q, mT);
            mPP = fma(w, p * p, mPP);          // products of two fp32 values: exact in float64
            mTT = fma(w, q * q, mTT);
            mPT = fma(w, p * q, mPT);
        }
        hb[0][r][c] = mP;
        hb[1][r][c] = mT;
        hb[2][r][c] = mPP;
        hb[3][r][c] = mTT;
        hb[4][r][c] = mPT;
    }
    __syncthreads();
    const double c1 = consts[(long long)b * 4 + 2 * form], c2 = consts[(long long)b * 4 + 2 * form + 1];
    double acc = 0.0;
    for (int it = t; it < kTileH * kTileW; it += kThreads) {
        const int i = it / kTileW, c = it % kTileW;
        double m[5] = {0.0, 0.0, 0.0, 0.0, 0.0};
#pragma unroll
        for (int u = 0; u < kTaps; ++u) {
            const double w = g.w[u];
#pragma unroll
            for (int q = 0; q < 5; ++q) m[q] = fma(w, hb[q][i + u][c], m[q]);
        }
        if (i0 + i < H - kTaps + 1 && j0 + c < W - kTaps + 1) {
            const double muPP = m[0] * m[0], muTT = m[1] * m[1], muPT = m[0] * m[1];
            const double sPv = m[2] - muPP, sTv = m[3] - muTT, sPT = m[4] - muPT;
            acc += ((2.0 * muPT + c1) * (2.0 * sPT + c2)) / ((muPP + muTT + c1) * (sPv + sTv + c2));
        }
    }
    acc = block_sum(acc, red);
    if (t == 0) tiles[((long long)form * B + b) * gridDim.x + tile] = acc;
}

__global__ __launch_bounds__(kThreads) void metrics_last(const double* __restrict__ fsum, const double* __restrict__ tiles,
                                                         double* __restrict__ out, int B, int T, int npix, double windows,
                                                         int mask_kind) {
    __shared__ double sh[kRec];
    __shared__ double red[kWaves];
    const int t = threadIdx.x, b = blockIdx.x;
    const bool pooled = b == B;
    double* row = out + (long long)b * 9;
    if (pooled && t < 2) {
        sum_form(fsum, B, sh, t);
        write_row(sh + t * kFields, row, t, mask_kind, (double)npix);      // the reference's H * W under the pooled count, literally
    }
    // frame b: the mean of its map; pooled: the mean of the frames' means, all of them over the same number of windows
    const long long cnt = pooled ? (long long)B * T : T;
    for (int f = 0; f < 2; ++f) {
        const double* src = tiles + ((long long)f * B + (pooled ? 0 : b)) * T;
        double v = 0.0;
        for (long long i = t; i < cnt; i += kThreads) v += src[i];
        v = block_sum(v, red);
        if (t == 0) row[4 * f + 3] = T > 0 ? v / (windows * (pooled ? (double)B : 1.0)) : __builtin_nan("");
        __syncthreads();
    }
}

bool dims_ok(int B, int H, int W) { return frame_dims_ok(B, H, W, 4ll * kMaxReduceBlocks * kThreads); }

}  // namespace

extern "C" size_t mvsgi_metrics_ws_bytes(int B, int H, int W) {
    if (!dims_ok(B, H, W)) return 0;
    return layout(B, H, W).total * sizeof(double);
}

extern "C" int mvsgi_metrics_f32(const float* preds, const float* target, const unsigned char* mask, int mask_kind, float lo, float hi,
                                 float bf, float cmin, float cmax, float thresh, float thresh_dist, int range_scope, void* ws,
                                 size_t ws_bytes, double* out, int B, int H, int W, mvsgi_stream_t stream) {
    const char* what = "mvsgi_metrics_f32";
    MVSGI_REQUIRE(preds && target && ws && out, "%s: null pointer (preds, target, ws and out are required)", what);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B %d, H %d, W %d)", what, B, H, W);
    MVSGI_REQUIRE(dims_ok(B, H, W), "%s: dimensions exceed the launch geometry (B %d, H %d, W %d)", what, B, H, W);
    MVSGI_REQUIRE(mask_kind >= MVSGI_METRICS_MASK_NONE && mask_kind <= MVSGI_METRICS_MASK_RANGE,
                  "%s: mask_kind = %d (0 none, 1 mask tensor, 2 label range)", what, mask_kind);
    MVSGI_REQUIRE(mask_kind != MVSGI_METRICS_MASK_TENSOR || mask, "%s: null pointer (mask_kind 1 needs a mask)", what);
    MVSGI_REQUIRE(mask_kind != MVSGI_METRICS_MASK_RANGE || lo <= hi, "%s: label range lo = %g > hi = %g (or a NaN)", what, (double)lo,
                  (double)hi);
    MVSGI_REQUIRE(range_scope == MVSGI_METRICS_RANGE_FRAME || range_scope == MVSGI_METRICS_RANGE_BATCH,
                  "%s: range_scope = %d (0 per frame, 1 whole batch)", what, range_scope);
    MVSGI_REQUIRE(bf > 0.f, "%s: bf = %g must be positive", what, (double)bf);
    const Layout l = layout(B, H, W);
    MVSGI_REQUIRE(ws_bytes >= l.total * sizeof(double), "%s: workspace of %zu bytes is too small (mvsgi_metrics_ws_bytes: %zu)", what,
                  ws_bytes, l.total * sizeof(double));
    MVSGI_REQUIRE(aligned(preds, 16) && aligned(target, 16), "%s: preds and target must be 16-byte aligned", what);
    MVSGI_REQUIRE(!mask || mask_kind != MVSGI_METRICS_MASK_TENSOR || aligned(mask, 4), "%s: mask must be 4-byte aligned", what);
    MVSGI_REQUIRE(aligned(ws, 8) && aligned(out, 8), "%s: ws and out must be 8-byte aligned", what);
    const int npix = H * W;
    Params k;
    k.lo = lo, k.hi = hi, k.bf = bf, k.cmin = cmin, k.cmax = cmax, k.thresh[0] = thresh, k.thresh[1] = thresh_dist;
    k.mask_kind = mask_kind;
    double* slab = static_cast<double*>(ws);
    hipStream_t st = mvsgi::as_stream(stream);
    hipLaunchKernelGGL(metrics_reduce, dim3((unsigned)l.G, (unsigned)B), dim3(kThreads), 0, st, preds, target, mask, slab + l.rec, npix,
                       k);
    if (mvsgi::check_launch("mvsgi_metrics_f32 (reduce)")) return 1;
    hipLaunchKernelGGL(metrics_finalise, dim3((unsigned)B), dim3(kThreads), 0, st, slab + l.rec, slab + l.fsum, slab + l.consts, out, B,
                       l.G, npix, mask_kind, range_scope == MVSGI_METRICS_RANGE_BATCH ? 1 : 0);
    if (mvsgi::check_launch("mvsgi_metrics_f32 (finalise)")) return 1;
    if (l.T > 0) {
        Gauss g;                                    // exp(-(u / 1.5)^2 / 2), u = -5 .. 5, normalised to sum 1
        double sum = 0.0;
        for (int u = 0; u < kTaps; ++u) {
            const double d = (double)(u - kTaps / 2) / 1.5;
            g.w[u] = std::exp(-(d * d) / 2.0);
            sum += g.w[u];
        }
        for (int u = 0; u < kTaps; ++u) g.w[u] /= sum;
        hipLaunchKernelGGL(metrics_ssim, dim3((unsigned)l.T, (unsigned)B, 2u), dim3(kThreads), 0, st, preds, target, slab + l.consts,
                           slab + l.tiles, B, H, W, l.tx, k, g);
        if (mvsgi::check_launch("mvsgi_metrics_f32 (ssim)")) return 1;
    }
    hipLaunchKernelGGL(metrics_last, dim3((unsigned)B + 1u), dim3(kThreads), 0, st, slab + l.fsum, slab + l.tiles, out, B, l.T, npix,
                       (double)(H - kTaps + 1) * (double)(W - kTaps + 1), mask_kind);
    return mvsgi::check_launch("mvsgi_metrics_f32 (last)");
}
