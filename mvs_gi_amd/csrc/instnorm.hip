// Instance norm on channels-last fp32 activations: [B][S][C] (NDHWC with S = D*H*W, or NHWC with S = H*W).
// Replaces nn.InstanceNorm3d / nn.InstanceNorm2d with input statistics (track_running_stats=False) in the conv blocks of
// dsta_mvs/model/common/common_modules.py:107-115: conv -> norm -> (+ res) -> act.  The statistics of a (frame, channel) are
// those of the conv's whole output, so they cannot fold into the conv epilogue as the eval BatchNorm does; two launches:
//
//   1. instnorm_stats: workgroup (k, b) reads rows [k*R, min((k+1)*R, S)) of frame b with 16-byte loads (one thread = 4
//      channels of one row), each thread runs Welford over its rows of x - x[b][0] (the frame's row 0 as a pivot: the
//      running mean stays O(std) even where |mean| >> std, so its fp32 rounding is relative to the spread, not the level), the threads of one channel are merged through LDS in
//      a fixed order (Chan's formula), and the chunk's (mean, M2) per channel is stored to ws[b][k][2][C] -- plain stores,
//      no atomics; workgroup 0 of a frame also stores the pivot to ws[b][nch][0][C].  R depends on S and C only (chunking()), so a frame's statistics do not depend on B or the device.
//   2. instnorm_apply: every workgroup first merges its frame's nch partials in a fixed order (from L2; nch <= kMaxChunks),
//      then writes y = act((x - mean) * rstd * gamma + beta (+ res)) over its own row range with 16-byte loads / stores.
//      y may alias x (each element is read and written by the same thread).
//
// var is the biased variance M2 / S; rstd = 1 / sqrt(var + eps) (F.instance_norm).  No E[x^2] - E[x]^2 anywhere: at
// S = 409600 and |mean| >> std that loses every digit in fp32.
#include "common.hpp"

namespace {

constexpr int kThreads = 256;
constexpr int kMaxChunks = 64;        // statistics partials per frame (what the apply prologue merges)
constexpr int kMaxApplyBlocks = 256;  // apply workgroups per frame
constexpr int kUnroll = 4;            // 16-byte loads in flight per thread

struct Chunking {
    int rpp;      // rows per pass of a workgroup (C / 4 threads per row)
    int rs;       // rows per statistics chunk (a multiple of rpp)
    int nch;      // statistics chunks per frame
    int ra;       // rows per apply workgroup (a multiple of rpp)
    int nap;      // apply workgroups per frame
};

// The geometry of both kernels: a function of (S, C) alone.
inline Chunking chunking(int S, int C) {
    Chunking k;
    const int cg = C / 4;
    k.rpp = kThreads / cg;
    const long long min_rows = mvsgi::cdiv(16384, 4LL * C);                 // >= 16 KB per statistics chunk
    long long r = mvsgi::cdiv(S, kMaxChunks);
    if (r < min_rows) r = min_rows;
    k.rs = (int)(mvsgi::cdiv(r, k.rpp) * k.rpp);
    k.nch = (int)mvsgi::cdiv(S, k.rs);
    const long long min_rows_a = mvsgi::cdiv(65536, 4LL * C);               // >= 64 KB per apply workgroup (amortises the prologue)
    long long ra = mvsgi::cdiv(S, kMaxApplyBlocks);
    if (ra < min_rows_a) ra = min_rows_a;
    k.ra = (int)(mvsgi::cdiv(ra, k.rpp) * k.rpp);
    k.nap = (int)mvsgi::cdiv(S, k.ra);
    return k;
}

// (n_a, mean_a, m2_a) += (n_b, mean_b, m2_b)  (Chan et al.); n_b > 0
__device__ __forceinline__ void chan_merge(float& na, float& ma, float& m2a, float nb, float mb, float m2b) {
    const float n = na + nb;
    const float d = mb - ma;
    const float fb = nb / n;
    ma = ma + d * fb;
    m2a = m2a + m2b + d * d * (na * fb);
    na = n;
}

__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }

// act(((v - piv) - mu) * a + be (+ r)); act(u) = u > 0 ? u : u * neg_slope.  mu is the mean of (x - piv) (see instnorm_stats);
// the differences first: with |mean| >> std, v * a + (be - mean * a) would cancel two large terms.
__device__ __forceinline__ float4 norm_act(float4 v, float4 r, bool has_res, const float* piv, const float* mu, const float* a,
                                           const float* be, float neg_slope) {
    float e[4] = {v.x, v.y, v.z, v.w};
    const float rr[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        e[i] = fmaf((e[i] - piv[i]) - mu[i], a[i], be[i]);
        if (has_res) e[i] += rr[i];
        e[i] = e[i] > 0.f ? e[i] : e[i] * neg_slope;
    }
    return make_float4(e[0], e[1], e[2], e[3]);
}

__global__ __launch_bounds__(kThreads) void instnorm_stats(const float* __restrict__ x, float* __restrict__ ws, int S, int C,
                                                           int rs, int nch) {
    __shared__ float lds[2 * kThreads * 4];                  // [2][rpp][C] (rpp * C <= 4 * kThreads)
    const int cg = C >> 2, rpp = kThreads / cg;
    const int t = threadIdx.x;
    const int q = t % cg, j = t / cg;                        // channel group, row offset in the pass
    const int k = blockIdx.x, b = blockIdx.y;
    const int r0 = k * rs, nr = min(rs, S - r0);
    const float* xb = x + ((long long)b * S + r0) * C + 4 * q;
    float n = 0.f, m[4] = {0.f, 0.f, 0.f, 0.f}, m2[4] = {0.f, 0.f, 0.f, 0.f};
    if (j < rpp) {
        const float4 kv = ld4(x + (long long)b * S * C + 4 * q);      // the frame's pivot (row 0)
        const float piv[4] = {kv.x, kv.y, kv.z, kv.w};
        int r = j;
        for (; r + (kUnroll - 1) * rpp < nr; r += kUnroll * rpp) {
            float4 v[kUnroll];
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) v[u] = ld4(xb + (long long)(r + u * rpp) * C);
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) {
                n += 1.f;
                const float inv = 1.f / n;
                const float e[4] = {v[u].x - piv[0], v[u].y - piv[1], v[u].z - piv[2], v[u].w - piv[3]};
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const float d = e[i] - m[i];
                    m[i] += d * inv;
                    m2[i] += d * (e[i] - m[i]);
                }
            }
        }
        for (; r < nr; r += rpp) {
            const float4 v = ld4(xb + (long long)r * C);
            n += 1.f;
            const float inv = 1.f / n;
            const float e[4] = {v.x - piv[0], v.y - piv[1], v.z - piv[2], v.w - piv[3]};
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float d = e[i] - m[i];
                m[i] += d * inv;
                m2[i] += d * (e[i] - m[i]);
            }
        }
        float* lm = lds + j * C + 4 * q;
        float* l2 = lds + rpp * C + j * C + 4 * q;
#pragma unroll
        for (int i = 0; i < 4; ++i) { lm[i] = m[i]; l2[i] = m2[i]; }
    }
    __syncthreads();
    // one thread per channel merges the rpp row offsets in order (row offset jj holds ceil((nr - jj) / rpp) rows)
    float* wsb = ws + (long long)b * (2 * nch + 1) * C;       // frame b: [nch][2][C] partials, then [C] pivot
    float* out = wsb + (long long)k * 2 * C;
    if (k == 0)           // the pivot travels to instnorm_apply in ws: with y == x, row 0 may be overwritten while others still need it
        for (int c = t; c < C; c += kThreads) wsb[(long long)nch * 2 * C + c] = x[(long long)b * S * C + c];
    for (int c = t; c < C; c += kThreads) {
        float na = 0.f, ma = 0.f, m2a = 0.f;
        for (int jj = 0; jj < rpp && jj < nr; ++jj) {
            const float nb = (float)((nr - jj + rpp - 1) / rpp);
            chan_merge(na, ma, m2a, nb, lds[jj * C + c], lds[rpp * C + jj * C + c]);
        }
        out[c] = ma;
        out[C + c] = m2a;
    }
}

__global__ __launch_bounds__(kThreads) void instnorm_apply(const float* x, const float* res, const float* __restrict__ gamma,
                                                           const float* __restrict__ beta, float* y, const float* __restrict__ ws,
                                                           int S, int C, int rs, int nch, int ra, float eps, float neg_slope) {
    // [0, C): mean; [C, 2C): rstd * gamma; [2C, 3C): beta; [3C, 3C + 2 * kThreads): merge scratch (mean, M2)
    extern __shared__ float lds[];
    float* s_mean = lds;
    float* s_a = lds + C;
    float* s_b = lds + 2 * C;
    float* s_tm = lds + 3 * C;
    float* s_t2 = s_tm + kThreads;
    const int t = threadIdx.x;
    const int b = blockIdx.y;
    const float* wb = ws + (long long)b * (2 * nch + 1) * C;
    // --- prologue: merge the frame's nch chunk partials (identical code and order in every workgroup of the frame)
    const int tpc = C >= kThreads ? 1 : kThreads / C;       // threads per channel
    const int cpp = kThreads / tpc;                          // channels per pass
    for (int c0 = 0; c0 < C; c0 += cpp) {
        const int c = c0 + t / tpc, s = t % tpc;
        float na = 0.f, ma = 0.f, m2a = 0.f;
        if (t < cpp * tpc && c < C) {
            for (int kk = s; kk < nch; kk += tpc) {
                const float nb = (float)min(rs, S - kk * rs);
                chan_merge(na, ma, m2a, nb, wb[(long long)kk * 2 * C + c], wb[(long long)kk * 2 * C + C + c]);
            }
        }
        s_tm[t] = ma;
        s_t2[t] = m2a;
        __syncthreads();
        if (s == 0 && t < cpp * tpc && c < C) {
            // lane s of this channel merged chunks s, s + tpc, ...: its count is known from (S, rs, nch) alone
            float n0 = 0.f, m0 = 0.f, q0 = 0.f;
            for (int ss = 0; ss < tpc && ss < nch; ++ss) {
                float nb = 0.f;
                for (int kk = ss; kk < nch; kk += tpc) nb += (float)min(rs, S - kk * rs);
                chan_merge(n0, m0, q0, nb, s_tm[t + ss], s_t2[t + ss]);
            }
            const float var = q0 / (float)S;
            const float rstd = 1.f / sqrtf(var + eps);
            s_mean[c] = m0;
            s_a[c] = rstd * (gamma ? gamma[c] : 1.f);
            s_b[c] = beta ? beta[c] : 0.f;
        }
        __syncthreads();
    }
    // --- apply over rows [blockIdx.x * ra, ...)
    const int cg = C >> 2, rpp = kThreads / cg;
    const int q = t % cg, j = t / cg;
    if (j >= rpp) return;
    const float4 kv = ld4(wb + (long long)nch * 2 * C + 4 * q);    // the frame's pivot, stored by instnorm_stats
    const float piv[4] = {kv.x, kv.y, kv.z, kv.w};
    float mu[4], a[4], be[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        mu[i] = s_mean[4 * q + i];
        a[i] = s_a[4 * q + i];
        be[i] = s_b[4 * q + i];
    }
    const int r0 = blockIdx.x * ra, nr = min(ra, S - r0);
    const long long base = ((long long)b * S + r0) * C + 4 * q;
    // (all kUnroll loads of a step are issued before its stores: x may alias y, so the compiler could not hoist them itself)
    int r = j;
    for (; r + (kUnroll - 1) * rpp < nr; r += kUnroll * rpp) {
        float4 v[kUnroll], rv[kUnroll] = {};
#pragma unroll
        for (int u = 0; u < kUnroll; ++u) v[u] = ld4(x + base + (long long)(r + u * rpp) * C);
        if (res) {
#pragma unroll
            for (int u = 0; u < kUnroll; ++u) rv[u] = ld4(res + base + (long long)(r + u * rpp) * C);
        }
#pragma unroll
        for (int u = 0; u < kUnroll; ++u)
            *reinterpret_cast<float4*>(y + base + (long long)(r + u * rpp) * C) = norm_act(v[u], rv[u], res != nullptr, piv, mu, a, be, neg_slope);
    }
    for (; r < nr; r += rpp) {
        const long long o = base + (long long)r * C;
        const float4 v = ld4(x + o);
        const float4 rv = res ? ld4(res + o) : make_float4(0.f, 0.f, 0.f, 0.f);
        *reinterpret_cast<float4*>(y + o) = norm_act(v, rv, res != nullptr, piv, mu, a, be, neg_slope);
    }
}

using mvsgi::aligned;

int check_dims(const char* what, int B, int S, int C) {
    MVSGI_REQUIRE(B > 0 && C > 0, "%s: non-positive dimension (B %d, C %d)", what, B, C);
    MVSGI_REQUIRE(C % 4 == 0 && C <= 4 * kThreads, "%s: C = %d must be a multiple of 4 and at most %d", what, C, 4 * kThreads);
    MVSGI_REQUIRE(S >= 2, "%s: S = %d: instance norm needs more than one spatial element per channel", what, S);
    MVSGI_REQUIRE(B < 65536 && (long long)S * C < (1ll << 31), "%s: dimensions exceed the launch geometry (B %d, S %d, C %d)", what,
                  B, S, C);
    return 0;
}

}  // namespace

extern "C" size_t mvsgi_instance_norm_ws_bytes(int B, int S, int C) {
    if (B <= 0 || S < 2 || C <= 0 || C % 4 || C > 4 * kThreads) return 0;
    const Chunking k = chunking(S, C);
    return (size_t)B * (2 * k.nch + 1) * C * sizeof(float);
}

extern "C" int mvsgi_instance_norm_f32(const float* x, const float* res, const float* gamma, const float* beta, float* y, float* ws,
                                       int B, int S, int C, float eps, float neg_slope, mvsgi_stream_t stream) {
    const char* what = "mvsgi_instance_norm_f32";
    MVSGI_REQUIRE(x && y && ws, "%s: null pointer (x, y and ws are required)", what);
    if (check_dims(what, B, S, C)) return 1;
    MVSGI_REQUIRE(aligned(x, 16) && aligned(y, 16) && aligned(ws, 16) && (!res || aligned(res, 16)),
                  "%s: x, res, y and ws must be 16-byte aligned", what);
    MVSGI_REQUIRE(eps >= 0.f, "%s: eps = %g must be >= 0", what, (double)eps);
    const Chunking k = chunking(S, C);
    hipStream_t st = mvsgi::as_stream(stream);
    hipLaunchKernelGGL(instnorm_stats, dim3((unsigned)k.nch, (unsigned)B), dim3(kThreads), 0, st, x, ws, S, C, k.rs, k.nch);
    if (mvsgi::check_launch("mvsgi_instance_norm_f32 (statistics)")) return 1;
    const size_t lds = (size_t)(3 * C + 2 * kThreads) * sizeof(float);
    hipLaunchKernelGGL(instnorm_apply, dim3((unsigned)k.nap, (unsigned)B), dim3(kThreads), lds, st, x, res, gamma, beta, y, ws, S, C,
                       k.rs, k.nch, k.ra, eps, neg_slope);
    return mvsgi::check_launch("mvsgi_instance_norm_f32 (apply)");
}
