// The small device idioms every kernel here uses, defined once: the vector types, the XCD-aware block remap, the window
// descriptor of the buffer loads / stores / LDS-DMA, and the 16-byte LDS-DMA piece.
// Include inside the translation unit's anonymous namespace (behind <hip/hip_runtime.h>, i.e. common.hpp).
#pragma once

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef float f32x16 __attribute__((ext_vector_type(16)));
typedef unsigned u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned short u16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef _Float16 f16x2 __attribute__((ext_vector_type(2)));
typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));

// Bijective XCD-aware remap of a flat block id (cdna_hip_programming.md T1).  The hardware deals blocks round-robin over the
// 8 XCDs, each with a private L2: blocks b, b + 8, ... share one.  The remap gives XCD x a contiguous run of the logical
// index space 0 .. n - 1 (the first n % 8 XCDs one element more), so that neighbours in the logical order -- halos of adjacent
// bricks, the cout blocks of a brick, the candidates of a sweep row -- meet in one L2.
__device__ __forceinline__ int xcd_remap(int bid, int n) {
    const int q = n >> 3, r = n & 7, x = bid & 7, i = bid >> 3;
    return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + i;
}

// ---- window descriptors ----
// A kernel addresses a tensor through a raw buffer descriptor whose BASE is the origin of the window it works on (a halo
// brick, a patch, an output brick), so that lanes carry 32-bit offsets within the window and the hardware's range check
// drops what falls behind the tensor's end (loads return 0, stores vanish; 0xffffff00 is the offset lanes use to opt out).
//   kRawBufferFlags   word 3 of the descriptor: DATA_FORMAT = 32 bit, no swizzle, no stride -- a raw byte buffer
//   kWindowMaxBytes   num_records is 32 bits wide and offsets up to 0xffffff00 plus a 16-byte access must not wrap: a window
//                     never claims more than 2^31 - 256 bytes, however much of the tensor lies behind its origin (tensors
//                     beyond 2 GiB: the launchers bound a window's OWN extent by the same number)
// WINDOW_RECORDS is the clamp; the two descriptor forms differ in what they promise about OFF:
//   WINDOW_DESC(BASE, OFF, TOTAL, LIVE)   any OFF: a window that is not LIVE or starts at / behind the tensor's end (the
//                     walk's look-ahead past the last brick) gets zero records, every access through it is dropped
//   window_desc(base, off, total[, live]) 0 <= off < total is the caller's: no test of its own (a site that already holds the
//                     window's origin and the bytes behind it passes them as base and total, off = 0)
// Both are straight-line scalar code.  WINDOW_DESC is a statement expression, not a function, for the hand-scheduled
// kernels: as a call hipcc allocates the scalar registers of their phase bodies differently, and those are placed around
// inline-asm MFMAs whose hazards it cannot see.  The order of the statements is part of the contract too -- hipcc's schedule
// follows it -- and tools/isa_diff.py is how a change here, or a new form at a site, is judged.
constexpr int kRawBufferFlags = 0x00020000;
constexpr int kWindowMaxBytes = 0x7fffff00;
#define WINDOW_RECORDS(LEFT) ((LEFT) > (long long)kWindowMaxBytes ? kWindowMaxBytes : (int)(LEFT))
#define WINDOW_DESC(BASE, OFF, TOTAL, LIVE)                                                                       \
    ({                                                                                                            \
        const long long off_ = (OFF);                                                                             \
        const long long left_ = (TOTAL) - off_;                                                                   \
        const int rec_ = WINDOW_RECORDS(left_);                                                                   \
        const int ok_ = (int)(LIVE) & (int)(left_ > 0);                                                           \
        __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(BASE) + off_, 0, ok_ ? rec_ : 0, kRawBufferFlags); \
    })
__device__ __forceinline__ __amdgpu_buffer_rsrc_t window_desc(const unsigned char* base, const long long off, const long long total,
                                                              const bool live = true) {
    const long long left = total - off;
    const int rec = WINDOW_RECORDS(left);
    return __builtin_amdgcn_make_buffer_rsrc(const_cast<unsigned char*>(base) + off, 0, live ? rec : 0, kRawBufferFlags);
}

// One LDS-DMA piece: 64 lanes x 16 B from per-lane offsets VOFF (+ the scalar SOFF) of a window into 1 KiB of LDS at DST.
#define LDS_DMA16(DSC, DST, VOFF, SOFF, AUX) \
    __builtin_amdgcn_raw_ptr_buffer_load_lds(DSC, (__attribute__((address_space(3))) void*)(DST), 16, VOFF, SOFF, 0, AUX)
// (A plain function for kernel TEMPLATES whose operands would be value-dependent inside the template: hipcc's host pass then
// drops the kernel's stub without a diagnostic.)
__device__ __forceinline__ void lds_dma16(const __amdgpu_buffer_rsrc_t dsc, unsigned char* lds_dst, const unsigned voff) {
    LDS_DMA16(dsc, lds_dst, voff, 0, 0);
}
