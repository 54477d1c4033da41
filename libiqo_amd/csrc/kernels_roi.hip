// kernels_roi.hip -- gfx950 kernel of the batched crop-and-resize (iqo_hip_resize_rois_device): N boxes
// of N sizes out of device-resident frames, each to dstW x dstH, in one launch.
//
//   roi_kernel<LZ, C, NORM>   LZ: Lanczos (signed 16-bit work) or Area / Linear (unsigned)
//                             C: 1, 3 or 4 interleaved bytes per pixel
//                             NORM: interleaved bytes out, or the normalised planar float epilogue
//
// The band pipeline is kernels_roi_dev.hpp's: one vertical pass over the box's packed rows, whose 8 values go
// to the work rows de-interleaved per channel (one channel: as whole dwords), and a horizontal pass in which a
// thread owns one output pixel of all C channels; then the store (mirrored when the box is flagged).
//
//   roi_fit_kernel<LZ, C, NORM>   the same pipeline on the fit arena (iqo_hip_resize_rois_fit_device): a box goes to
//                                 rectangle (ox, oy, iw, ih) of its dstW x dstH canvas, by the tables of (w -> iw) and
//                                 (h -> ih); a band workgroup also writes the pad columns left and right of its rows,
//                                 and pad workgroups write the rows above and below the rectangle (roi.hpp).
// It is a sibling of roi_kernel over the same helpers, not a template switch of it: the stretch kernels' source,
// and so their code, stays what it was.
#include "kernels_roi_dev.hpp"

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
struct RoiFitArgs : RoiArgs {
    uint32_t pad;               // the pad pixel: byte c is channel c's
};
struct RoiFitNormArgs : RoiFitArgs {
    NormDev n;
};

// The pad runs of canvas rows [ya, yb) of output `o`, columns [xa, xb)
template <int C, bool NORM, typename Args>
__device__ __forceinline__ void roi_pad_block(const Args &a, uint8_t *o, int ya, int yb, int xa, int xb, int tid)
{
    uint8_t *const row = o + static_cast<int64_t>(ya) * a.dstSt;
    if constexpr (NORM) {
        const NormDev &n = a.n;
        const int elem = n.dtype == 1 ? 4 : 2;
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p >= n.planes)
                break;
            const RoiPadPat pat = roi_pad_pattern_norm(n, p, (a.pad >> (8 * n.order[p])) & 0xffu);
            roi_pad_rows(row + static_cast<int64_t>(p) * n.planeSt + xa * elem, a.dstSt, yb - ya, (xb - xa) * elem, pat, elem, tid);
        }
    } else {
        roi_pad_rows(row + xa * C, a.dstSt, yb - ya, (xb - xa) * C, roi_pad_pattern(a.pad, C), 1, tid);
    }
}

template <bool LZ, int C, bool NORM>
__global__ __launch_bounds__(256) void roi_kernel(std::conditional_t<NORM, RoiNormArgs, RoiArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t roi_lds[];
    const uint32_t *const A = a.arena;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const uint32_t wg = blockIdx.x;
    const int dstW = sld(A, kHDstW), dstH = sld(A, kHDstH), frameRowB = sld(A, kHRowBytes);
    const uint32_t *const rec0 = A + kRoiHdrWords;

    const int roi = roi_find_box<kRoiRecWords, kRFirst>(rec0, sld(A, kHRois), wg, lane);
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

    // LDS: tap records [rows][nYp] | work rows [rows][C][pitchDw]
    uint2 *const taps = reinterpret_cast<uint2 *>(roi_lds);
    uint32_t *const work = roi_lds + 2 * rows * nYp;
    uint16_t *const work16 = reinterpret_cast<uint16_t *>(work);

    roi_stage_taps(taps, yt, dstH, y0, nRows, a.srcSt, tid);
    lds_barrier();

    // 1. vertical pass over the box's packed rows (bx * C: the byte of its first pixel in the frame's row)
    using Store = std::conditional_t<C == 1, RoiStorePlanar, RoiStoreInterleaved<C>>;
    roi_vertical<LZ, Store>(box, a.srcSt, w * C, bx * C, frameRowB, taps, yt, y0, nRows, work, C * pitchDw, pitchDw, padL, tid);
    lds_barrier();
    // work columns outside the box: its clamped edge column
    {
        const int ent = 2 * pitchDw, nPad = ent - w;
        for (int t = tid; t < nRows * C * nPad; t += 256) {
            const int rc = t / nPad;
            roi_edge_fill(work16 + rc * ent, t - rc * nPad, padL, w);
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
        uint32_t bt[C];
        roi_horizontal<LZ, C>(wp, pitchDw, cx, NP, dstW, x, cr.y, bt);
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
                roi_store_norm(n, p, v, xo, o);
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

template <bool LZ, int C, bool NORM>
__global__ __launch_bounds__(256) void roi_fit_kernel(std::conditional_t<NORM, RoiFitNormArgs, RoiFitArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t roi_lds[];
    const uint32_t *const A = a.arena;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const uint32_t wg = blockIdx.x;
    const int dstW = sld(A, kHDstW), dstH = sld(A, kHDstH), frameRowB = sld(A, kHRowBytes);
    const uint32_t *const rec0 = A + kRoiHdrWords;

    const int roi = roi_find_box<kRoiFitRecWords, kRFirst>(rec0, sld(A, kHRois), wg, lane);
    const uint32_t *const r = rec0 + static_cast<size_t>(roi) * kRoiFitRecWords;
    const int w = sld(r, kRW), bx = sld(r, kRX), flip = sld(r, kRFlags) & 1;
    const int rows = sld(r, kRRows);
    // the workgroup within its box: a pad workgroup writes whole canvas rows and is done
    const uint32_t *const ext = r + kRoiFitExt;
    uint8_t *const canvas = a.dst + static_cast<int64_t>(roi) * a.dstRoiSt;
    int y0, y1;
    if (!roi_fit_role(ext, static_cast<int>(wg - static_cast<uint32_t>(sld(r, kRFirst))), sld(r, kRGroups), rows, dstH, &y0, &y1)) {
        roi_pad_block<C, NORM>(a, canvas, y0, y1, 0, dstW, tid);
        return;
    }
    // a band of rectangle (ox, oy, iw, ih): first the pad columns left and right of its rows
    const int iw = sld(ext, kFIW), ih = sld(ext, kFIH), ox = sld(ext, kFOX), oy = sld(ext, kFOY);
    const int nRows = y1 - y0;
    roi_pad_block<C, NORM>(a, canvas, oy + y0, oy + y1, 0, ox, tid);
    roi_pad_block<C, NORM>(a, canvas, oy + y0, oy + y1, ox + iw, dstW, tid);
    const uint8_t *const box =
        a.src + ((static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kROffHi))) << 32) | static_cast<uint32_t>(sld(r, kROffLo)));
    const uint32_t *const xt = A + static_cast<uint32_t>(sld(r, kRXTab));
    const uint32_t *const yt = A + static_cast<uint32_t>(sld(r, kRYTab));
    const int NP = sld(xt, 0), padL = sld(xt, 1), pitchDw = sld(xt, 2);
    const int nYp = sld(yt, 0);

    // LDS: tap records [rows][nYp] | work rows [rows][C][pitchDw]
    uint2 *const taps = reinterpret_cast<uint2 *>(roi_lds);
    uint32_t *const work = roi_lds + 2 * rows * nYp;
    uint16_t *const work16 = reinterpret_cast<uint16_t *>(work);

    roi_stage_taps(taps, yt, ih, y0, nRows, a.srcSt, tid);
    lds_barrier();

    // 1. vertical pass over the box's packed rows (bx * C: the byte of its first pixel in the frame's row)
    using Store = std::conditional_t<C == 1, RoiStorePlanar, RoiStoreInterleaved<C>>;
    roi_vertical<LZ, Store>(box, a.srcSt, w * C, bx * C, frameRowB, taps, yt, y0, nRows, work, C * pitchDw, pitchDw, padL, tid);
    lds_barrier();
    // work columns outside the box: its clamped edge column
    {
        const int ent = 2 * pitchDw, nPad = ent - w;
        for (int t = tid; t < nRows * C * nPad; t += 256) {
            const int rc = t / nPad;
            roi_edge_fill(work16 + rc * ent, t - rc * nPad, padL, w);
        }
    }
    lds_barrier();

    // 2. horizontal pass
    const int32_t *const col = reinterpret_cast<const int32_t *>(xt + 4);
    const uint32_t *const cx = xt + 4 + 2 * iw;
    for (int t = tid; t < nRows * iw; t += 256) {
        const int j = t / iw, x = t - j * iw;
        const int2 cr = *reinterpret_cast<const int2 *>(col + 2 * x);  // {even window start, divisor}
        const uint32_t *wp = work + j * C * pitchDw + ((cr.x + padL) >> 1);
        uint32_t bt[C];
        roi_horizontal<LZ, C>(wp, pitchDw, cx, NP, iw, x, cr.y, bt);
        const int xo = ox + (flip ? iw - 1 - x : x);
        uint8_t *const o = canvas + static_cast<int64_t>(oy + y0 + j) * a.dstSt;
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
                roi_store_norm(n, p, v, xo, o);
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

template <bool NORM, bool FIT>
const void *roi_fn(bool lanczos, int channels)
{
#define IQO_ROI(LZ_, C_) \
    (FIT ? reinterpret_cast<const void *>(roi_fit_kernel<LZ_, C_, NORM>) : reinterpret_cast<const void *>(roi_kernel<LZ_, C_, NORM>))
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
    const void *kern = d.fit ? (norm ? roi_fn<true, true>(d.lanczos, d.channels) : roi_fn<false, true>(d.lanczos, d.channels))
                             : (norm ? roi_fn<true, false>(d.lanczos, d.channels) : roi_fn<false, false>(d.lanczos, d.channels));
    if (!kern)
        return hipErrorInvalidValue;
    RoiFitNormArgs a;
    a.arena = d.arena;
    a.src = d.src;
    a.dst = d.dst;
    a.srcSt = static_cast<int>(d.srcSt);
    a.dstSt = d.dstSt;
    a.dstRoiSt = d.dstRoiSt;
    a.pad = static_cast<uint32_t>(d.pad[0]) | (static_cast<uint32_t>(d.pad[1]) << 8) | (static_cast<uint32_t>(d.pad[2]) << 16) |
            (static_cast<uint32_t>(d.pad[3]) << 24);
    if (d.fit)
        return roi_launch<RoiFitArgs>(kern, a, norm, d.groups, d.ldsBytes, s);
    RoiNormArgs b;
    static_cast<RoiArgs &>(b) = a;
    return roi_launch<RoiArgs>(kern, b, norm, d.groups, d.ldsBytes, s);
}

} // namespace iqo_amd
