// Packed point cloud (include/mvsgi.h, "packed point cloud"): the prediction, filtered and compacted into
// a list of records [x, y, z, colour .., attributes ..] per frame, in the order of the pixels.  Three launches, no atomics and no
// workgroup that waits for another:
//
//   cloud_flags_kernel    grid (tiles, B).  A tile is 1024 consecutive linear pixels; 256 threads take four coalesced passes of 256,
//                         so the __ballot of wave w in pass q is the 64-bit word of the pixels [64 (4 q + w), + 64) of the tile.
//                         Writes the 16 words of the tile (1 bit per pixel) and the sum of their popcounts.  The predicate is
//                         evaluated here and nowhere else.
//   cloud_scan_kernel     grid (B).  Exclusive scan of a frame's tile counts through LDS, 256 tiles per pass with a carry from
//                         pass to pass; writes the tile offsets and counts[b] = (min(kept, capacity), kept).
//   cloud_scatter_kernel  grid (tiles, B).  Reads the tile's 16 words; a set lane's position in the tile is the popcounts of the
//                         earlier words + mbcnt(word & lanes below).  The set lanes write their pixel into a list in LDS at that
//                         position, and the threads then walk the LIST: entry k, at tile offset + k < capacity, recomputes d and
//                         xyz (back_project of camera_models.hpp: the arithmetic of reproject.hip), picks the colour of the first valid
//                         camera, reads the attributes and stores its R floats.  Nothing of a dropped pixel is fetched.  (Working
//                         from the list and not from the lanes' own bits keeps the waves full when few pixels are kept and puts
//                         neighbouring records into neighbouring lanes: 128 frames of 160 x 640 with 10 % kept 215 -> 148 us,
//                         with everything kept unchanged)
//
// Every load and store is a 4-byte (or 1-byte, 8-byte for the words) access of its own element: no alignment beyond the element's.
// Offsets into points / index are 64-bit (B * capacity * R may pass 2^31).
#include "common.hpp"

namespace {

#include "camera_models.hpp"

using mvsgi::kMaxCams;
constexpr int kTile = 1024;                 // pixels per tile
constexpr int kThreads = 256;
constexpr int kWords = kTile / 64;          // 64-bit words per tile
constexpr int kMaxGates = 4;
constexpr int kMaxRecord = 16;
constexpr int kMaxAttrs = kMaxRecord - 3;
constexpr int kMaxChannels = 4;

struct CloudArgs {
    const float* inv;
    const float* rays;
    const unsigned char* mask;
    const float* gate[kMaxGates];
    const float* warped;
    const unsigned char* valid;
    const float* attr[kMaxAttrs];
    float lo[kMaxGates], hi[kMaxGates];
    long long mask_stride;                  // 0: one mask for every frame, H * W: one per frame
    long long capacity;
    int n_gates, N, C, A, require_colour;
    int H, W, sy, sx, tiles;
    float bf, d_min, d_max, no_colour;
};

// workspace: [B][tiles][16] words, then [B][tiles] tile counts, then [B][tiles] tile offsets (each part a multiple of 16 bytes)
struct CloudWs {
    unsigned long long* words;
    int* tile_count;
    int* tile_offset;
};
inline size_t round16(size_t n) { return (n + 15) / 16 * 16; }
inline size_t ws_words_bytes(long long B, long long tiles) { return round16((size_t)B * tiles * kWords * 8); }
inline size_t ws_ints_bytes(long long B, long long tiles) { return round16((size_t)B * tiles * 4); }

__device__ __forceinline__ bool cloud_keep(const CloudArgs& a, long long b, int p, long long HW) {
#pragma clang fp contract(off)
    const int i = p / a.W, j = p - i * a.W;
    if (i % a.sy != 0 || j % a.sx != 0) return false;
    if (a.mask && a.mask[b * a.mask_stride + p] == 0) return false;
    const float d = a.bf / a.inv[b * HW + p];
    if (!(fabsf(d) < __builtin_inff()) || !(d >= a.d_min) || !(d <= a.d_max)) return false;
#pragma unroll
    for (int k = 0; k < kMaxGates; ++k) {                               // unrolled: the tables stay in the kernel's arguments
        if (k >= a.n_gates) break;
        const float g = a.gate[k][b * HW + p];
        if (!(g >= a.lo[k]) || !(g <= a.hi[k])) return false;
    }
    if (a.require_colour) {
        bool any = false;
        for (int n = 0; n < a.N && !any; ++n) any = a.valid[(b * a.N + n) * HW + p] != 0;
        if (!any) return false;
    }
    return true;
}

__global__ __launch_bounds__(kThreads) void cloud_flags_kernel(CloudArgs a, CloudWs ws) {
    __shared__ int wave_sum[kThreads / 64];
    const int tile = (int)blockIdx.x;
    const long long b = blockIdx.y;
    const long long HW = (long long)a.H * a.W;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    unsigned long long* words = ws.words + (b * a.tiles + tile) * kWords;
    int sum = 0;                                                        // wave-uniform
#pragma unroll
    for (int q = 0; q < kTile / kThreads; ++q) {
        const long long p = (long long)tile * kTile + q * kThreads + threadIdx.x;
        const bool keep = p < HW && cloud_keep(a, b, (int)p, HW);
        const unsigned long long word = __ballot(keep);
        if (lane == 0) words[q * (kThreads / 64) + wave] = word;
        sum += __popcll(word);
    }
    if (lane == 0) wave_sum[wave] = sum;
    __syncthreads();
    if (threadIdx.x == 0) ws.tile_count[b * a.tiles + tile] = wave_sum[0] + wave_sum[1] + wave_sum[2] + wave_sum[3];
}

__global__ __launch_bounds__(kThreads) void cloud_scan_kernel(CloudWs ws, int* __restrict__ counts, int tiles, long long capacity) {
    __shared__ int buf[2][kThreads];
    const long long b = blockIdx.x;
    const int* cnt = ws.tile_count + b * tiles;
    int* off = ws.tile_offset + b * tiles;
    const int t = threadIdx.x;
    long long carry = 0;                                                // kept pixels of the passes before this one (< 2^31)
    for (int base = 0; base < tiles; base += kThreads) {
        const int c = base + t < tiles ? cnt[base + t] : 0;
        int cur = 0;
        buf[0][t] = c;
        __syncthreads();
#pragma unroll
        for (int s = 1; s < kThreads; s <<= 1) {                         // Hillis-Steele inclusive scan, double-buffered
            const int v = buf[cur][t] + (t >= s ? buf[cur][t - s] : 0);
            buf[cur ^ 1][t] = v;
            cur ^= 1;
            __syncthreads();
        }
        const int incl = buf[cur][t];
        const int total = buf[cur][kThreads - 1];
        if (base + t < tiles) off[base + t] = (int)(carry + incl - c);
        carry += total;
        __syncthreads();                                                // buf is rewritten by the next pass
    }
    if (t == 0) {
        counts[b * 2] = (int)(carry < capacity ? carry : capacity);
        counts[b * 2 + 1] = (int)carry;
    }
}

__global__ __launch_bounds__(kThreads) void cloud_scatter_kernel(CloudArgs a, CloudWs ws, float* __restrict__ points,
                                                                 int* __restrict__ index) {
    __shared__ unsigned long long word_s[kWords];
    __shared__ int before_s[kWords + 1];                                // popcounts of the tile's earlier words; [kWords]: of all
    __shared__ unsigned short list_s[kTile];                            // the tile's kept pixels (offsets in the tile), ascending
    const int tile = (int)blockIdx.x;
    const long long b = blockIdx.y;
    const long long bt = b * a.tiles + tile;
    const long long first = ws.tile_offset[bt];                         // block-uniform
    if (ws.tile_count[bt] == 0 || first >= a.capacity) return;
    if (threadIdx.x < kWords) word_s[threadIdx.x] = ws.words[bt * kWords + threadIdx.x];
    __syncthreads();
    if (threadIdx.x <= kWords) {
        int n = 0;
        for (int k = 0; k < (int)threadIdx.x; ++k) n += __popcll(word_s[k]);
        before_s[threadIdx.x] = n;
    }
    __syncthreads();
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
#pragma unroll
    for (int q = 0; q < kTile / kThreads; ++q) {
        const int w = q * (kThreads / 64) + wave;
        const unsigned long long word = word_s[w];
        const unsigned long long below = word & ((1ull << lane) - 1ull);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(below >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)below, 0u));
        if ((word >> lane) & 1ull) list_s[before_s[w] + rank] = (unsigned short)(q * kThreads + threadIdx.x);
    }
    __syncthreads();
    // the list is dense: every lane of a wave but the last works, and lanes next to each other write records next to each other
    const long long room = a.capacity - first;
    const int n_tile = (int)(before_s[kWords] < room ? before_s[kWords] : room);
    const long long HW = (long long)a.H * a.W;
    const int R = 3 + a.C + a.A;
    for (int k = threadIdx.x; k < n_tile; k += kThreads) {
        const int p = tile * kTile + list_s[k];                         // < H * W: its bit is set
        const long long dest = first + k;                               // < capacity
        float* o = points + (b * a.capacity + dest) * R;
        float x, y, z;
        back_project(a.bf, a.inv[b * HW + p], a.rays[p], a.rays[HW + p], a.rays[2 * HW + p], x, y, z);
        o[0] = x, o[1] = y, o[2] = z;
        if (a.C) {
            int cam = -1;
            for (int n = 0; n < a.N && cam < 0; ++n)
                if (a.valid[(b * a.N + n) * HW + p] != 0) cam = n;
            for (int c = 0; c < a.C; ++c) o[3 + c] = cam < 0 ? a.no_colour : a.warped[((b * a.N + cam) * a.C + c) * HW + p];
        }
#pragma unroll
        for (int m = 0; m < kMaxAttrs; ++m) {
            if (m >= a.A) break;
            o[3 + a.C + m] = a.attr[m][b * HW + p];
        }
        if (index) index[b * a.capacity + dest] = p;
    }
}

}  // namespace

extern "C" size_t mvsgi_cloud_ws_bytes(long long B, int H, int W) {
    if (B < 1 || B > 65535 || H < 1 || W < 1 || (long long)H * W >= (1ll << 31)) return 0;
    const long long tiles = mvsgi::cdiv((long long)H * W, kTile);
    return ws_words_bytes(B, tiles) + 2 * ws_ints_bytes(B, tiles);
}

extern "C" int mvsgi_cloud_pack_f32(const float* inv, const float* rays, const unsigned char* mask, int mask_per_frame,
                                    const float* const* gates_host, const float* gate_lo_host, const float* gate_hi_host, int n_gates,
                                    const float* warped, const unsigned char* valid, int N, int C, int require_colour, float no_colour,
                                    const float* const* attrs_host, int A, float* points, int* counts, int* index, long long capacity,
                                    void* ws, size_t ws_bytes, long long B, int H, int W, int sy, int sx, float bf, float d_min,
                                    float d_max, mvsgi_stream_t stream) {
    const char* what = "mvsgi_cloud_pack_f32";
    MVSGI_REQUIRE(inv && rays && points && counts && ws, "%s: null pointer (inv, rays, points, counts and ws are required)", what);
    MVSGI_REQUIRE(B >= 1 && H >= 1 && W >= 1, "%s: non-positive dimension (B = %lld, H = %d, W = %d)", what, B, H, W);
    MVSGI_REQUIRE((long long)H * W < (1ll << 31) && B <= 65535, "%s: map %d x %d or batch %lld too large (H * W < 2^31, B <= 65535)", what,
                  H, W, B);
    MVSGI_REQUIRE(sy >= 1 && sx >= 1, "%s: step (%d, %d) (need >= 1)", what, sy, sx);
    MVSGI_REQUIRE(capacity >= 1 && capacity < (1ll << 31), "%s: capacity %lld (need 1 <= capacity < 2^31)", what, capacity);
    MVSGI_REQUIRE(n_gates >= 0 && n_gates <= kMaxGates, "%s: %d gates (at most %d)", what, n_gates, kMaxGates);
    MVSGI_REQUIRE(n_gates == 0 || (gates_host && gate_lo_host && gate_hi_host), "%s: null pointer (gates without their tables)", what);
    MVSGI_REQUIRE((warped != nullptr) == (valid != nullptr), "%s: warped and valid are given together or not at all", what);
    if (!warped) N = 0, C = 0;
    if (warped) {
        MVSGI_REQUIRE(N >= 1 && N <= kMaxCams, "%s: N = %d cameras (need 1 <= N <= %d)", what, N, kMaxCams);
        MVSGI_REQUIRE(C >= 1 && C <= kMaxChannels, "%s: C = %d colour channels (need 1 <= C <= %d)", what, C, kMaxChannels);
    }
    MVSGI_REQUIRE(!require_colour || valid, "%s: require_colour without warped / valid", what);
    MVSGI_REQUIRE(A >= 0 && (A == 0 || attrs_host), "%s: A = %d attribute planes (need A >= 0 and their table)", what, A);
    MVSGI_REQUIRE(3 + C + A <= kMaxRecord, "%s: record of %d floats (3 + C + A, at most %d)", what, 3 + C + A, kMaxRecord);
    const size_t need = mvsgi_cloud_ws_bytes(B, H, W);
    MVSGI_REQUIRE(need && ws_bytes >= need, "%s: workspace of %zu bytes (need %zu)", what, ws_bytes, need);
    MVSGI_REQUIRE((uintptr_t)ws % 16 == 0, "%s: ws must be 16-byte aligned", what);
    MVSGI_REQUIRE((uintptr_t)inv % 4 == 0 && (uintptr_t)rays % 4 == 0 && (uintptr_t)points % 4 == 0 && (uintptr_t)counts % 4 == 0 &&
                      (uintptr_t)index % 4 == 0 && (uintptr_t)warped % 4 == 0,
                  "%s: fp32 / int32 buffers must be 4-byte aligned", what);
    CloudArgs a;
    memset(&a, 0, sizeof(a));
    for (int k = 0; k < n_gates; ++k) {
        MVSGI_REQUIRE(gates_host[k] && (uintptr_t)gates_host[k] % 4 == 0, "%s: gate %d: null or misaligned plane", what, k);
        a.gate[k] = gates_host[k], a.lo[k] = gate_lo_host[k], a.hi[k] = gate_hi_host[k];
    }
    for (int m = 0; m < A; ++m) {
        MVSGI_REQUIRE(attrs_host[m] && (uintptr_t)attrs_host[m] % 4 == 0, "%s: attribute %d: null or misaligned plane", what, m);
        a.attr[m] = attrs_host[m];
    }
    const long long tiles = mvsgi::cdiv((long long)H * W, kTile);
    a.inv = inv, a.rays = rays, a.mask = mask, a.warped = warped, a.valid = valid;
    a.mask_stride = mask && mask_per_frame ? (long long)H * W : 0;
    a.capacity = capacity;
    a.n_gates = n_gates, a.N = N, a.C = C, a.A = A, a.require_colour = require_colour ? 1 : 0;
    a.H = H, a.W = W, a.sy = sy, a.sx = sx, a.tiles = (int)tiles;
    a.bf = bf, a.d_min = d_min, a.d_max = d_max, a.no_colour = no_colour;
    CloudWs w;
    unsigned char* base = static_cast<unsigned char*>(ws);
    w.words = reinterpret_cast<unsigned long long*>(base);
    w.tile_count = reinterpret_cast<int*>(base + ws_words_bytes(B, tiles));
    w.tile_offset = reinterpret_cast<int*>(base + ws_words_bytes(B, tiles) + ws_ints_bytes(B, tiles));
    hipStream_t st = mvsgi::as_stream(stream);
    const dim3 grid((unsigned)tiles, (unsigned)B);
    hipLaunchKernelGGL(cloud_flags_kernel, grid, dim3(kThreads), 0, st, a, w);
    hipLaunchKernelGGL(cloud_scan_kernel, dim3((unsigned)B), dim3(kThreads), 0, st, w, counts, (int)tiles, capacity);
    hipLaunchKernelGGL(cloud_scatter_kernel, grid, dim3(kThreads), 0, st, a, w, points, index);
    return mvsgi::check_launch(what);
}
