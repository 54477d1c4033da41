// kernels_roi.hip -- gfx950 kernel of the batched crop-and-resize (iqo_hip_resize_rois_device): N boxes
// of N sizes out of device-resident frames, each to dstW x dstH, in one launch.
//
//   roi_kernel<LZ, C, NORM>   LZ: Lanczos (signed 16-bit work) or Area / Linear (unsigned)
//                             C: 1, 3 or 4 interleaved bytes per pixel
//                             NORM: interleaved bytes out, or the normalised planar float epilogue
//
// Everything a workgroup needs comes from the call's ARENA (roi.hpp): it finds its box and band of
// output rows by the boxes' first-workgroup indices, then reads THAT box's X and Y tables -- the
// one-window-per-coordinate form of the tile kernels (plan.hpp axis_windows), so identity, replicated
// and masked borders are all one formula per axis.  Two passes through LDS, as packed_tile_kernel:
//   1. vertical: a task is (output row of the band, 8 consecutive bytes of the box's packed row).  The
//      8 bytes come from the 2 or 3 aligned words they lie in (v_alignbyte_b32) where those words are
//      inside the frame's row, and from single clamped byte loads at the row's two ends, so no byte
//      outside the frame's rows is ever read; rows are clamped to the box.  Four v_pk_mad_u16 per tap
//      (the low 16 bits are the reference's wrap), the exact division on masked border rows, and the 8
//      values go to the work row de-interleaved per channel.  Work columns left and right of the box are then
//      filled with the box's edge column (never with the frame's pixels there).
//   2. horizontal: a thread owns one output pixel of all C channels: its coefficient pairs are loaded
//      once (coalesced: the arena keeps them pair-major) and each pair is one v_dot2 on an aligned
//      dword of the channel's work row; then the rounding shift or the exact border division, the
//      clamp, and the store (mirrored when the box is flagged).
#include "kernels_dev.hpp"
#include "roi.hpp"

namespace iqo_amd {
namespace {

struct RoiArgs {
    const uint32_t *arena;
    const uint8_t *src;
    uint8_t *dst;
    int srcSt;                  // bytes (frameH * srcSt < 2^31, roi_layout)
    int64_t dstSt, dstRoiSt;    // bytes
};
struct RoiNormArgs : RoiArgs {
    NormDev n;
};

template <bool LZ, int C, bool NORM>
__global__ __launch_bounds__(256) void roi_kernel(std::conditional_t<NORM, RoiNormArgs, RoiArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t roi_lds[];
    const uint32_t *const A = a.arena;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const uint32_t wg = blockIdx.x;
    const int dstW = sld(A, kHDstW), dstH = sld(A, kHDstH), frameRowB = sld(A, kHRowBytes);
    const uint32_t *const rec0 = A + kRoiHdrWords;

    // the workgroup's box: the last record whose first workgroup is <= wg, by a 64-way search (every
    // wave runs it; a batch of 4096 boxes takes two rounds)
    int roi = 0;
    {
        int n = sld(A, kHRois);
        while (n > 1) {
            const int step = (n + 63) >> 6;
            const int i = lane * step;
            const bool le = i < n && rec0[static_cast<size_t>(roi + i) * kRoiRecWords + kRFirst] <= wg;
            const int k = __popcll(__ballot(le)) - 1;  // lane 0 always holds: first(roi) <= wg
            roi = __builtin_amdgcn_readfirstlane(roi + k * step);
            n = __builtin_amdgcn_readfirstlane(min(step, n - k * step));
        }
    }
    const uint32_t *const r = rec0 + static_cast<size_t>(roi) * kRoiRecWords;
    const int w = sld(r, kRW), bx = sld(r, kRX), flip = sld(r, kRFlags) & 1;
    const int rows = sld(r, kRRows);
    const int y0 = static_cast<int>(wg - static_cast<uint32_t>(sld(r, kRFirst))) * rows;
    const int nRows = min(rows, dstH - y0);
    const uint8_t *const box =
        a.src + ((static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kROffHi))) << 32) | static_cast<uint32_t>(sld(r, kROffLo)));
    const uint32_t *const xt = A + static_cast<uint32_t>(sld(r, kRXTab));
    const uint32_t *const yt = A + static_cast<uint32_t>(sld(r, kRYTab));
    const int NP = sld(xt, 0), padL = sld(xt, 1), pitchDw = sld(xt, 2);
    const int nYp = sld(yt, 0);
    const int32_t *const rowRec = reinterpret_cast<const int32_t *>(yt + 4);
    const uint32_t *const cy = yt + 4 + 4 * dstH;

    // LDS: tap records [rows][nYp] {coefficient splat, byte offset of the clamped row} | work rows
    // [rows][C][pitchDw]
    uint2 *const taps = reinterpret_cast<uint2 *>(roi_lds);
    uint32_t *const work = roi_lds + 2 * rows * nYp;
    uint16_t *const work16 = reinterpret_cast<uint16_t *>(work);

    for (int t = tid; t < nRows * nYp; t += 256) {
        const int j = t / nYp, k = t - j * nYp, y = y0 + j;
        const int rr = max(rowRec[4 * y + 1], min(rowRec[4 * y] + k, rowRec[4 * y + 2]));
        const uint32_t c = (cy[y * (nYp >> 1) + (k >> 1)] >> (16 * (k & 1))) & 0xffffu;
        taps[t] = make_uint2(c | (c << 16), static_cast<uint32_t>(rr * a.srcSt));
    }
    lds_barrier();

    // 1. vertical pass: a task is (row of the band, 8 consecutive bytes of the box's packed row)
    {
        const int nB = w * C, nG = (nB + 7) >> 3;
        const int xB = bx * C;  // byte of the box's first pixel in the frame's row
        // rows a multiple of 4 bytes apart: a task's misalignment, and whether its aligned words lie inside
        // the frame's row, are the same for every tap
        const bool rowsAligned = !(a.srcSt & 3);
        // 8 bytes at p (box byte 8 g of some row) as two words.  fast: the 2 (mis == 0) or 3 aligned words
        // they lie in are inside the frame's row; otherwise single bytes, clamped to the box's last byte
        auto fetch = [&](const uint8_t *p, int mis, bool fast, int g, uint32_t &v0, uint32_t &v1) {
            if (fast) {
                const uint32_t *q = reinterpret_cast<const uint32_t *>(p - mis);
                const uint32_t w0 = q[0], w1 = q[1], w2 = q[mis ? 2 : 1];
                v0 = __builtin_amdgcn_alignbyte(w1, w0, static_cast<uint32_t>(mis));
                v1 = __builtin_amdgcn_alignbyte(w2, w1, static_cast<uint32_t>(mis));
            } else {
                const int last = nB - 1 - 8 * g;
                v0 = v1 = 0;
#pragma unroll
                for (int b = 0; b < 4; ++b) {
                    v0 |= static_cast<uint32_t>(p[min(b, last)]) << (8 * b);
                    v1 |= static_cast<uint32_t>(p[min(b + 4, last)]) << (8 * b);
                }
            }
        };
        auto inside = [&](int g, int mis) {  // the aligned words of box bytes [8 g, 8 g + 8) of a row
            const int s = xB + 8 * g - mis;
            return s >= 0 && s + (mis ? 12 : 8) <= frameRowB;
        };
        for (int t = tid; t < nRows * nG; t += 256) {
            const int j = t / nG, g = t - j * nG;
            const uint8_t *const p0 = box + 8 * g;
            const uint2 *tj = taps + j * nYp;
            uint32_t acc[4] = {0, 0, 0, 0};
            auto tap = [&](uint32_t v0, uint32_t v1, uint32_t c) {
                uint32_t u[4];
                unpack4(v0, u[0], u[1]);
                unpack4(v1, u[2], u[3]);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[m] = pk_mad(u[m], c, acc[m]);
            };
            if (rowsAligned) {
                const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(p0) & 3);
                const bool fast = inside(g, mis);
                for (int k = 0; k < nYp; ++k) {
                    const uint2 tp = tj[k];
                    uint32_t v0, v1;
                    fetch(p0 + tp.y, mis, fast, g, v0, v1);
                    tap(v0, v1, tp.x);
                }
            } else {
                for (int k = 0; k < nYp; ++k) {
                    const uint2 tp = tj[k];
                    const uint8_t *p = p0 + tp.y;
                    const int mis = static_cast<int>(reinterpret_cast<uintptr_t>(p) & 3);
                    uint32_t v0, v1;
                    fetch(p, mis, inside(g, mis), g, v0, v1);
                    tap(v0, v1, tp.x);
                }
            }
            if constexpr (LZ) {
                const int deno = rowRec[4 * (y0 + j) + 3];
                if (deno != 0) {  // masked + renormalised border row: int16(nume * 64 / deno)
                    auto dv = [&](uint32_t pr) {
                        const int l = exact_div(static_cast<int>(static_cast<int16_t>(pr & 0xffffu)) * 64, deno);
                        const int h = exact_div(static_cast<int>(static_cast<int16_t>(pr >> 16)) * 64, deno);
                        return (static_cast<uint32_t>(l) & 0xffffu) | (static_cast<uint32_t>(h) << 16);
                    };
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        acc[m] = dv(acc[m]);
                }
            }
            if (C == 1 && 8 * g + 8 <= nB) {  // one channel: the pairs are the work row's dwords (padL is even)
                uint32_t *wd = work + j * pitchDw + ((padL + 8 * g) >> 1);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    wd[m] = acc[m];
            } else {
#pragma unroll
                for (int b = 0; b < 8; ++b) {
                    const int q = 8 * g + b;
                    if (q < nB) {
                        const int px = q / C, ch = q - px * C;
                        work16[2 * (j * C + ch) * pitchDw + padL + px] = static_cast<uint16_t>(acc[b >> 1] >> (16 * (b & 1)));
                    }
                }
            }
        }
    }
    lds_barrier();
    // work columns outside the box: its clamped edge column
    {
        const int ent = 2 * pitchDw, nPad = ent - w;
        for (int t = tid; t < nRows * C * nPad; t += 256) {
            const int rc = t / nPad, k = t - rc * nPad;
            uint16_t *wr = work16 + rc * ent;
            wr[k < padL ? k : w + k] = wr[k < padL ? padL : padL + w - 1];
        }
    }
    lds_barrier();

    // 2. horizontal pass
    const int32_t *const col = reinterpret_cast<const int32_t *>(xt + 4);
    const uint32_t *const cx = xt + 4 + 2 * dstW;
    for (int t = tid; t < nRows * dstW; t += 256) {
        const int j = t / dstW, x = t - j * dstW;
        const int2 cr = *reinterpret_cast<const int2 *>(col + 2 * x);  // {even window start, divisor}
        const uint32_t *wp = work + j * C * pitchDw + ((cr.x + padL) >> 1);
        int s[C];
#pragma unroll
        for (int c = 0; c < C; ++c)
            s[c] = LZ ? (1 << 19) : (1 << 22);
        for (int p = 0; p < NP; ++p) {
            const uint32_t cf = cx[p * dstW + x];
#pragma unroll
            for (int c = 0; c < C; ++c)
                s[c] = LZ ? sdot2(wp[c * pitchDw + p], cf, s[c])
                          : static_cast<int>(udot2(wp[c * pitchDw + p], cf, static_cast<uint32_t>(s[c])));
        }
        uint32_t bt[C];
#pragma unroll
        for (int c = 0; c < C; ++c) {
            if (LZ) {
                int v = s[c] >> 20;
                if (cr.y != 0)
                    v = static_cast<int16_t>(exact_div(s[c], cr.y));
                bt[c] = static_cast<uint32_t>(min(max(v, 0), 255));
            } else {
                bt[c] = min((static_cast<uint32_t>(s[c]) >> 23) & 0xffffu, 255u);
            }
        }
        const int xo = flip ? dstW - 1 - x : x;
        uint8_t *const o = a.dst + static_cast<int64_t>(roi) * a.dstRoiSt + static_cast<int64_t>(y0 + j) * a.dstSt;
        if constexpr (NORM) {
            const NormDev &n = a.n;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= n.planes)
                    break;
                const int oc = n.order[p];
                uint32_t v = bt[0];
#pragma unroll
                for (int c = 1; c < C; ++c)
                    v = oc == c ? bt[c] : v;
                const float f = norm_affine(v, n.scale[p], n.bias[p]);
                uint8_t *const e = o + static_cast<int64_t>(p) * n.planeSt;
                if (n.dtype == 1)
                    reinterpret_cast<float *>(e)[xo] = f;
                else
                    reinterpret_cast<uint16_t *>(e)[xo] = static_cast<uint16_t>(n.dtype == 2 ? f16_bits(f) : bf16_bits(f));
            }
        } else {
            uint8_t *const e = o + xo * C;
            bool stored = false;
            if constexpr (C == 4) {
                if (!(reinterpret_cast<uintptr_t>(e) & 3)) {
                    // (opaque: keeps the combiner from packing two clamps into v_ashr_pk_u8_i32's undefined half)
                    *reinterpret_cast<uint32_t *>(e) = opaque(bt[0] | (bt[1] << 8)) | (bt[2] << 16) | (bt[3] << 24);
                    stored = true;
                }
            }
            if (!stored) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    e[c] = static_cast<uint8_t>(bt[c]);
            }
        }
    }
}

template <bool NORM>
const void *roi_fn(bool lanczos, int channels)
{
#define IQO_ROI(LZ_, C_) reinterpret_cast<const void *>(roi_kernel<LZ_, C_, NORM>)
    switch (channels) {
    case 1:
        return lanczos ? IQO_ROI(true, 1) : IQO_ROI(false, 1);
    case 3:
        return lanczos ? IQO_ROI(true, 3) : IQO_ROI(false, 3);
    case 4:
        return lanczos ? IQO_ROI(true, 4) : IQO_ROI(false, 4);
    default:
        return nullptr;
    }
#undef IQO_ROI
}

} // namespace

hipError_t launch_roi(const RoiDev &d, const NormDev *norm, hipStream_t s)
{
    if (d.groups == 0)
        return hipSuccess;
    if (d.ldsBytes > static_cast<size_t>(kRoiLdsMax) || d.srcSt >= (int64_t(1) << 31))
        return hipErrorInvalidValue;
    const void *kern = norm ? roi_fn<true>(d.lanczos, d.channels) : roi_fn<false>(d.lanczos, d.channels);
    if (!kern)
        return hipErrorInvalidValue;
    RoiNormArgs a;
    a.arena = d.arena;
    a.src = d.src;
    a.dst = d.dst;
    a.srcSt = static_cast<int>(d.srcSt);
    a.dstSt = d.dstSt;
    a.dstRoiSt = d.dstRoiSt;
    RoiArgs u = a;
    void *args[] = {&u};
    if (norm) {
        a.n = *norm;
        args[0] = &a;
    }
    return hipLaunchKernel(kern, dim3(d.groups), dim3(256), args, d.ldsBytes, s);
}

} // namespace iqo_amd
