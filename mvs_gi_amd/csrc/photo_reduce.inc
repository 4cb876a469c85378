// The text of photo.hip's reduce kernel, included once per value of the flag MVSGI_PHOTO_SEEN:
//   0  photo_reduce<IN, VEC, NT>       the kernel as it was before the flag existed: same signature, same text, same code
//   1  photo_reduce_seen<IN, VEC, NT>  one more argument, cam_seen [B][N][H][W] (bytes): a camera sees a pixel only where it is != 0
// Two texts of one file rather than a template flag: with the flag as a template parameter of a shared __forceinline__ body under two
// __global__s the existing instances came out with another register allocation and another schedule (DESIGN.md 20); included
// like this they are the parent's code instruction for instruction.
// IN: layout of the camera images.  VEC: W % 4 == 0; otherwise element-wise with a row tail.  NT: cameras held in registers, N <= NT.
template <int IN, bool VEC, int NT>
#if MVSGI_PHOTO_SEEN
__global__ __launch_bounds__(kThreads) void photo_reduce_seen(const float* __restrict__ inv, const float* __restrict__ rays,
                                                              const void* __restrict__ imgs, const float* __restrict__ cam_masks,
                                                              const unsigned char* __restrict__ mask, PhotoOut o, ViewRig rig,
                                                              PhotoDims s, float bf, float thresh, float pi_f,
                                                              const unsigned char* __restrict__ cam_seen) {
#else
__global__ __launch_bounds__(kThreads) void photo_reduce(const float* __restrict__ inv, const float* __restrict__ rays,
                                                         const void* __restrict__ imgs, const float* __restrict__ cam_masks,
                                                         const unsigned char* __restrict__ mask, PhotoOut o, ViewRig rig, PhotoDims s,
                                                         float bf, float thresh, float pi_f) {
#endif
#pragma clang fp contract(off)
    __shared__ float lut[IN == U8HWC3 ? 256 : 1];
    stage_u8_table<IN>(lut);
    const int t = threadIdx.x, G = gridDim.x;
    const long long b = blockIdx.y;
    const long long HW = (long long)s.H * s.W;
    const long long HWr = (long long)s.Hr * s.Wr;
    const float* invb = inv + b * HW;
    const unsigned char* mb = mask ? mask + (s.mask_per_frame ? b * HW : 0) : nullptr;
    const float fC = (float)s.C;

    double sh = 0.0, sl = 0.0, vh = 0.0, vl = 0.0;
    unsigned nbad = 0, nsc = 0, nmask = 0, hist[kViews];
#pragma unroll
    for (int k = 0; k < kViews; ++k) hist[k] = 0;

    for (int q = blockIdx.x * kThreads + t; q < s.nq; q += G * kThreads) {
        const int i = q / s.Wq;
        const int j = (q - i * s.Wq) * 4;
        const int n = VEC ? 4 : min(4, s.W - j);                          // pixels of this thread inside the row
        const long long pix = (long long)i * s.W + j;                     // first pixel of this thread inside a plane

        // steps 1, 2 of the back-projection: d = bf / v, p = r * d.  The text of view_rig.hpp's quad_points, kept here: called as that
        // function the row-tail instances of this kernel came out as other, slower code (DESIGN.md 20); so is n_views' store below
        float px[4], py[4], pz[4];
        {
            float v[4], rx[4], ry[4], rz[4];
            if (VEC) {
                const f32x4 v4 = *reinterpret_cast<const f32x4*>(invb + pix);
                const f32x4 x4 = *reinterpret_cast<const f32x4*>(rays + pix);
                const f32x4 y4 = *reinterpret_cast<const f32x4*>(rays + HW + pix);
                const f32x4 z4 = *reinterpret_cast<const f32x4*>(rays + 2 * HW + pix);
#pragma unroll
                for (int k = 0; k < 4; ++k) v[k] = v4[k], rx[k] = x4[k], ry[k] = y4[k], rz[k] = z4[k];
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const bool in = k < n;
                    v[k] = in ? invb[pix + k] : 1.0f;
                    rx[k] = in ? rays[pix + k] : 0.0f;
                    ry[k] = in ? rays[HW + pix + k] : 0.0f;
                    rz[k] = in ? rays[2 * HW + pix + k] : 0.0f;
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) back_project(bf, v[k], rx[k], ry[k], rz[k], px[k], py[k], pz[k]);
        }

        // steps 3-5 per camera, and the definition's step 1: seen = valid (& the camera's mask sampled at the same grid > 0)
        float gx[NT][4], gy[NT][4];
        unsigned valid = 0, seen = 0;                                     // bit 4 * cam + k
        float cnt[4] = {0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int cam = 0; cam < NT; ++cam) {
            if (cam < s.N) {
                const ViewCam& c = rig.cam[cam];
#if MVSGI_PHOTO_SEEN
                // cam_seen of the thread's four pixels, a byte each
                const unsigned sw = load_byte_quad<VEC>(cam_seen + (b * s.N + cam) * HW + pix, n);
#endif
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    float x, y, z;
                    const bool in_fov = camera_view(c, px[k], py[k], pz[k], pi_f, x, y, z, gx[cam][k], gy[cam][k]);
                    const bool ok = grid_valid(in_fov, gx[cam][k], gy[cam][k]) && k < n;
                    bool sn = ok;
                    if (ok && cam_masks) {                                // an invalid camera's taps are not fetched
                        const Bilin bt = bilin_setup(gx[cam][k], gy[cam][k], s.Wr, s.Hr);
                        sn = bilin_fetch(cam_masks + cam * HWr, bt) > 0.0f;
                    }
#if MVSGI_PHOTO_SEEN
                    sn = sn && ((sw >> (8 * k)) & 0xffu) != 0u;
#endif
                    valid |= (ok ? 1u : 0u) << (4 * cam + k);
                    seen |= (sn ? 1u : 0u) << (4 * cam + k);
                    cnt[k] = cnt[k] + (sn ? 1.0f : 0.0f);                 // the definition's step 2, in camera order
                }
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) gx[cam][k] = gy[cam][k] = 0.0f;
            }
        }
        bool ok[4];
        float kdiv[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            ok[k] = cnt[k] > 1.0f;
            kdiv[k] = ok[k] ? cnt[k] : 1.0f;
        }

        // steps 3-5 of the definition, channel by channel; the samples of the channel stay in registers between the two passes
        float vsum[4] = {0.0f, 0.0f, 0.0f, 0.0f};
        auto channel = [&](int ch) {
            float w[NT][4], acc[4] = {0.0f, 0.0f, 0.0f, 0.0f};
            // the kept coordinates pass through an empty statement the compiler cannot see through, once per channel and ahead of
            // its loads: without it the tap set-up is hoisted out of the channel loop and its eight values per camera and pixel spill
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) asm volatile("" : "+v"(gx[cam][k]), "+v"(gy[cam][k]));
            }
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    w[cam][k] = 0.0f;                                     // what the back-projection writes for an invalid camera
                    if (cam < s.N && ((valid >> (4 * cam + k)) & 1u)) {
                        const Bilin bt = bilin_setup(gx[cam][k], gy[cam][k], s.Wr, s.Hr);
                        const long long m = b * s.N + cam;
                        if (IN == U8HWC3)
                            w[cam][k] = bilin_fetch_u8(static_cast<const unsigned char*>(imgs) + m * HWr * 3, ch, lut, bt);
                        else
                            w[cam][k] = bilin_fetch(static_cast<const float*>(imgs) + (m * s.C + ch) * HWr, bt);
                    }
                    if (cam < s.N) acc[k] = acc[k] + w[cam][k] * (((seen >> (4 * cam + k)) & 1u) ? 1.0f : 0.0f);
                }
            }
            float avg[4], var[4];
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                avg[k] = acc[k] / kdiv[k];
                var[k] = 0.0f;
            }
#pragma unroll
            for (int cam = 0; cam < NT; ++cam) {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    if (cam < s.N) {
                        const float x = ((seen >> (4 * cam + k)) & 1u) ? w[cam][k] : avg[k];
                        const float d = x - avg[k];
                        var[k] = var[k] + d * d;
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                var[k] = ok[k] ? var[k] / kdiv[k] : 0.0f;
                vsum[k] = vsum[k] + var[k];
            }
            if (o.mean) {
                float* m = o.mean + (b * s.C + ch) * HW + pix;
                if (VEC) {
                    *reinterpret_cast<f32x4*>(m) = f32x4{avg[0], avg[1], avg[2], avg[3]};
                } else {
#pragma unroll
                    for (int k = 0; k < 4; ++k)
                        if (k < n) m[k] = avg[k];
                }
            }
        };
        if (IN == U8HWC3) {
            channel(0), channel(1), channel(2);
        } else {
#pragma unroll 1
            for (int ch = 0; ch < s.C; ++ch) channel(ch);
        }

        // steps 5, 6 and the per-pixel outputs
        float pv[4], ps[4];
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            pv[k] = vsum[k] / fC;
            ps[k] = sqrtf(pv[k]);
        }
        if (VEC) {
            if (o.var) *reinterpret_cast<f32x4*>(o.var + b * HW + pix) = f32x4{pv[0], pv[1], pv[2], pv[3]};
            if (o.std) *reinterpret_cast<f32x4*>(o.std + b * HW + pix) = f32x4{ps[0], ps[1], ps[2], ps[3]};
            if (o.n_views)
                *reinterpret_cast<unsigned*>(o.n_views + b * HW + pix) =
                    (unsigned)cnt[0] | ((unsigned)cnt[1] << 8) | ((unsigned)cnt[2] << 16) | ((unsigned)cnt[3] << 24);
        } else {
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                if (k < n) {
                    if (o.var) o.var[b * HW + pix + k] = pv[k];
                    if (o.std) o.std[b * HW + pix + k] = ps[k];
                    if (o.n_views) o.n_views[b * HW + pix + k] = (unsigned char)cnt[k];
                }
            }
        }

        // step 7: the scores
        if (o.recs) {
            unsigned mw = 0x01010101u;
            if (mb) mw = load_byte_quad<VEC>(mb + pix, n);
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                const bool masked = k < n && ((mw >> (8 * k)) & 0xffu) != 0u;
                const int c = (int)cnt[k];
#pragma unroll
                for (int h = 0; h < kViews; ++h) hist[h] += (masked && c == h) ? 1u : 0u;
                nmask += masked ? 1u : 0u;
                if (masked && ok[k]) {                                    // a select: an unscored pixel never reaches a sum
                    sum_add(sh, sl, (double)ps[k]);
                    sum_add(vh, vl, (double)pv[k]);
                    nbad += ps[k] > thresh ? 1u : 0u;
                    nsc += 1u;
                }
            }
        }
    }
    if (!o.recs) return;

    double r[kRec];
    r[F_SH] = sh, r[F_SL] = sl, r[F_VH] = vh, r[F_VL] = vl;
    r[F_NB] = (double)nbad, r[F_N] = (double)nsc, r[F_NM] = (double)nmask;
#pragma unroll
    for (int h = 0; h < kViews; ++h) r[F_V0 + h] = (double)hist[h];
    block_reduce_store<kRec>(r, o.recs, b, G, RecMerge());
}
