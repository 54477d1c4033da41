// kernels_roi_yuv.hip -- gfx950 kernel of the batched crop-and-resize of NV12 / I420 frames straight to RGB
// (iqo_hip_resize_rois_yuv_rgb_device / _norm_device): N boxes of N sizes, each to dstW x dstH, in one launch.
//
//   roi_yuv_kernel<LZ, UV2, NORM>   LZ: Lanczos (signed 16-bit work) or Area / Linear (unsigned)
//                                   UV2: interleaved UV plane (NV12) or separate U and V planes (I420)
//                                   NORM: packed bytes out, or the normalised planar float epilogue
//
// The band pipeline of kernels_roi_dev.hpp three times over in one workgroup: a band of output rows of one box
// of the call's ARENA (roi.hpp, the YUV format) gets a Y work row from the box's luma tables
// (w -> dstW, h -> dstH) and a U and a V work row from its chroma tables (w/2 -> dstW, h/2 -> dstH), so all
// three components arrive on the output grid.
//   1. vertical: the planar pass on Y, and on U and on V (I420), or the pairs pass on the UV plane (NV12), where
//      a task's 8 bytes are 4 (U, V) pairs and each v_pk_mad_u16 accumulates one pair: its halves go to the U
//      and the V row.  Aligned words are fetched where they lie inside THAT PLANE's row.
//   2. horizontal: a thread owns one output pixel: NP dot products on the Y row, NPc on each of the U and V
//      rows, each component's own shift or border division and clamp, then colorspace.hpp's integer matrix
//      and the store (mirrored when the box is flagged).
// The three work rows of a band row lie one after the other, pitchY + 2 pitchC dwords: odd, as each pitch is.
//
//   roi_yuv_fit_kernel<LZ, UV2, NORM>   the same pipeline on the YUV fit arena (iqo_hip_resize_rois_yuv_fit_*_device):
//                                       a box goes to rectangle (ox, oy, iw, ih) of its canvas by the tables of
//                                       (w -> iw, h -> ih) and (w/2 -> iw, h/2 -> ih); pad columns by the band
//                                       workgroups, pad rows by pad workgroups, as roi_fit_kernel.
// A sibling of roi_yuv_kernel over the same helpers, not a template switch of it: the stretch kernels' source, and so
// their code, stays what it was.
#include "kernels_roi_dev.hpp"

namespace iqo_amd {
namespace {

struct RoiYuvArgs {
    const uint32_t *arena;
    const uint8_t *y, *u, *v;
    uint8_t *dst;
    int64_t dstSt, dstRoiSt;    // bytes
    YuvRgbCoef k;
    uint32_t sel;               // v_perm selector: byte c of a stored pixel out of (R, G, B, 255)
    int channels;               // 3 or 4 bytes per stored pixel
};
struct RoiYuvNormArgs : RoiYuvArgs {
    NormDev n;
};
struct RoiYuvFitArgs : RoiYuvArgs {
    uint32_t pad;               // the pad pixel as the matrix gives one: R | G << 8 | B << 16 | 255 << 24
};
struct RoiYuvFitNormArgs : RoiYuvFitArgs {
    NormDev n;
};

// The pad runs of canvas rows [ya, yb) of output `o`, columns [xa, xb)
template <bool NORM, typename Args>
__device__ __forceinline__ void roi_yuv_pad_block(const Args &a, uint8_t *o, int ya, int yb, int xa, int xb, int tid)
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
        const RoiPadPat pat = roi_pad_pattern(__builtin_amdgcn_perm(0u, a.pad, a.sel), a.channels);
        roi_pad_rows(row + xa * a.channels, a.dstSt, yb - ya, (xb - xa) * a.channels, pat, 1, tid);
    }
}

template <bool LZ, bool UV2, bool NORM>
__global__ __launch_bounds__(256) void roi_yuv_kernel(std::conditional_t<NORM, RoiYuvNormArgs, RoiYuvArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t roi_yuv_lds[];
    const uint32_t *const A = a.arena;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const uint32_t wg = blockIdx.x;
    const int dstW = sld(A, kHDstW), dstH = sld(A, kHDstH);
    const int rowBY = sld(A, kHYRowBytes), rowBC = sld(A, kHYRowBytesC), stY = sld(A, kHYStY), stC = sld(A, kHYStC);
    const uint32_t *const rec0 = A + kRoiHdrWords;

    const int roi = roi_find_box<kRoiYuvRecWords, kYFirst>(rec0, sld(A, kHRois), wg, lane);
    const uint32_t *const r = rec0 + static_cast<size_t>(roi) * kRoiYuvRecWords;
    const int w = sld(r, kYW), bx = sld(r, kYX), flip = sld(r, kYFlags) & 1;
    const int rows = sld(r, kYRows);
    const int y0 = static_cast<int>(wg - static_cast<uint32_t>(sld(r, kYFirst))) * rows;
    const int nRows = min(rows, dstH - y0);
    const uint64_t off = (static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kYOffHi))) << 32) | static_cast<uint32_t>(sld(r, kYOffLo));
    const uint64_t offC = (static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kYOffCHi))) << 32) | static_cast<uint32_t>(sld(r, kYOffCLo));
    const uint32_t *const xt = A + static_cast<uint32_t>(sld(r, kYXTab));
    const uint32_t *const yt = A + static_cast<uint32_t>(sld(r, kYYTab));
    const uint32_t *const xtC = A + static_cast<uint32_t>(sld(r, kYXTabC));
    const uint32_t *const ytC = A + static_cast<uint32_t>(sld(r, kYYTabC));
    const int NP = sld(xt, 0), padL = sld(xt, 1), pitchY = sld(xt, 2);
    const int NPc = sld(xtC, 0), padLc = sld(xtC, 1), pitchC = sld(xtC, 2);
    const int nYp = sld(yt, 0), nYpC = sld(ytC, 0);
    const int rowPitch = pitchY + 2 * pitchC;  // a band row's Y, U and V work rows, dwords

    // LDS: luma tap records [rows][nYp] | chroma tap records [rows][nYpC] | work rows [rows][rowPitch]
    uint2 *const taps = reinterpret_cast<uint2 *>(roi_yuv_lds);
    uint2 *const tapsC = taps + rows * nYp;
    uint32_t *const work = roi_yuv_lds + 2 * rows * (nYp + nYpC);
    uint16_t *const work16 = reinterpret_cast<uint16_t *>(work);

    roi_stage_taps(taps, yt, dstH, y0, nRows, stY, tid);
    roi_stage_taps(tapsC, ytC, dstH, y0, nRows, stC, tid);
    lds_barrier();

    // 1. vertical pass: Y, then the chroma plane(s)
    const int wc = w >> 1;
    roi_vertical<LZ, RoiStorePlanar>(a.y + off, stY, w, bx, rowBY, taps, yt, y0, nRows, work, rowPitch, 0, padL, tid);
    if constexpr (UV2) {
        roi_vertical<LZ, RoiStorePairs>(a.u + offC, stC, w, bx, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, pitchC,
                                        padLc, tid);
    } else {
        roi_vertical<LZ, RoiStorePlanar>(a.u + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, 0,
                                         padLc, tid);
        roi_vertical<LZ, RoiStorePlanar>(a.v + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY + pitchC,
                                         rowPitch, 0, padLc, tid);
    }
    lds_barrier();
    // work columns outside the box: its clamped edge column, in each of the three rows
    {
        const int nPadY = 2 * pitchY - w, nPadC = 2 * pitchC - wc, nPad = nPadY + 2 * nPadC;
        for (int t = tid; t < nRows * nPad; t += 256) {
            const int j = t / nPad;
            int k = t - j * nPad;
            uint16_t *wr = work16 + 2 * j * rowPitch;
            int pl = padL, n = w;
            if (k >= nPadY) {
                k -= nPadY;
                wr += 2 * pitchY;
                pl = padLc;
                n = wc;
                if (k >= nPadC) {
                    k -= nPadC;
                    wr += 2 * pitchC;
                }
            }
            roi_edge_fill(wr, k, pl, n);
        }
    }
    lds_barrier();

    // 2. horizontal pass
    const int2 *const col = reinterpret_cast<const int2 *>(xt + 4);     // {even window start, divisor}
    const int2 *const colC = reinterpret_cast<const int2 *>(xtC + 4);
    const uint32_t *const cx = xt + 4 + 2 * dstW;
    const uint32_t *const cxC = xtC + 4 + 2 * dstW;
    for (int t = tid; t < nRows * dstW; t += 256) {
        const int j = t / dstW, x = t - j * dstW;
        const int2 cr = col[x], cc = colC[x];
        const uint32_t *const wj = work + j * rowPitch;
        const uint32_t *const wpC = wj + pitchY + ((cc.x + padLc) >> 1);
        int Y, U, V;
        roi_horizontal<LZ, 1>(wj + ((cr.x + padL) >> 1), 0, cx, NP, dstW, x, cr.y, &Y);
        roi_horizontal<LZ, 1>(wpC, 0, cxC, NPc, dstW, x, cc.y, &U);
        roi_horizontal<LZ, 1>(wpC + pitchC, 0, cxC, NPc, dstW, x, cc.y, &V);
        // (R, G, B, 255): the shift and both clamps of yuv_to_rgb in two v_ashr_pk_u8_i32, as yuv_rgb_kernel's
        // rgb_word.  (Written as shifts and clamps, the combiner folds a pair into that instruction and leaves its
        // undefined half in the word: kernels_dev.hpp opaque)
        int sr, sg, sb;
        yuv_sums(a.k, Y, yuv_chroma_terms(a.k, U, V), sr, sg, sb);
        const uint32_t px = ashr_pk_hi<kYuvRgbShift>(ashr_pk_lo<kYuvRgbShift>(sr, sg), sb, 255 << kYuvRgbShift);
        const int xo = flip ? dstW - 1 - x : x;
        uint8_t *const o = a.dst + static_cast<int64_t>(roi) * a.dstRoiSt + static_cast<int64_t>(y0 + j) * a.dstSt;
        if constexpr (NORM) {
            const NormDev &n = a.n;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= n.planes)
                    break;
                roi_store_norm(n, p, (px >> (8 * n.order[p])) & 0xffu, xo, o);
            }
        } else {
            const uint32_t out = __builtin_amdgcn_perm(0u, px, a.sel);
            uint8_t *const e = o + xo * a.channels;
            if (a.channels == 4 && !(reinterpret_cast<uintptr_t>(e) & 3)) {
                *reinterpret_cast<uint32_t *>(e) = out;
            } else {
                e[0] = static_cast<uint8_t>(out);
                e[1] = static_cast<uint8_t>(out >> 8);
                e[2] = static_cast<uint8_t>(out >> 16);
                if (a.channels == 4)
                    e[3] = static_cast<uint8_t>(out >> 24);
            }
        }
    }
}

template <bool LZ, bool UV2, bool NORM>
__global__ __launch_bounds__(256) void roi_yuv_fit_kernel(std::conditional_t<NORM, RoiYuvFitNormArgs, RoiYuvFitArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t roi_yuv_lds[];
    const uint32_t *const A = a.arena;
    const int tid = static_cast<int>(threadIdx.x), lane = tid & 63;
    const uint32_t wg = blockIdx.x;
    const int dstW = sld(A, kHDstW), dstH = sld(A, kHDstH);
    const int rowBY = sld(A, kHYRowBytes), rowBC = sld(A, kHYRowBytesC), stY = sld(A, kHYStY), stC = sld(A, kHYStC);
    const uint32_t *const rec0 = A + kRoiHdrWords;

    const int roi = roi_find_box<kRoiYuvFitRecWords, kYFirst>(rec0, sld(A, kHRois), wg, lane);
    const uint32_t *const r = rec0 + static_cast<size_t>(roi) * kRoiYuvFitRecWords;
    const int w = sld(r, kYW), bx = sld(r, kYX), flip = sld(r, kYFlags) & 1;
    const int rows = sld(r, kYRows);
    // the workgroup within its box: a pad workgroup writes whole canvas rows and is done
    const uint32_t *const ext = r + kRoiYuvFitExt;
    uint8_t *const canvas = a.dst + static_cast<int64_t>(roi) * a.dstRoiSt;
    int y0, y1;
    if (!roi_fit_role(ext, static_cast<int>(wg - static_cast<uint32_t>(sld(r, kYFirst))), sld(r, kYGroups), rows, dstH, &y0, &y1)) {
        roi_yuv_pad_block<NORM>(a, canvas, y0, y1, 0, dstW, tid);
        return;
    }
    // a band of rectangle (ox, oy, iw, ih): first the pad columns left and right of its rows
    const int iw = sld(ext, kFIW), ih = sld(ext, kFIH), ox = sld(ext, kFOX), oy = sld(ext, kFOY);
    const int nRows = y1 - y0;
    roi_yuv_pad_block<NORM>(a, canvas, oy + y0, oy + y1, 0, ox, tid);
    roi_yuv_pad_block<NORM>(a, canvas, oy + y0, oy + y1, ox + iw, dstW, tid);
    const uint64_t off = (static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kYOffHi))) << 32) | static_cast<uint32_t>(sld(r, kYOffLo));
    const uint64_t offC = (static_cast<uint64_t>(static_cast<uint32_t>(sld(r, kYOffCHi))) << 32) | static_cast<uint32_t>(sld(r, kYOffCLo));
    const uint32_t *const xt = A + static_cast<uint32_t>(sld(r, kYXTab));
    const uint32_t *const yt = A + static_cast<uint32_t>(sld(r, kYYTab));
    const uint32_t *const xtC = A + static_cast<uint32_t>(sld(r, kYXTabC));
    const uint32_t *const ytC = A + static_cast<uint32_t>(sld(r, kYYTabC));
    const int NP = sld(xt, 0), padL = sld(xt, 1), pitchY = sld(xt, 2);
    const int NPc = sld(xtC, 0), padLc = sld(xtC, 1), pitchC = sld(xtC, 2);
    const int nYp = sld(yt, 0), nYpC = sld(ytC, 0);
    const int rowPitch = pitchY + 2 * pitchC;  // a band row's Y, U and V work rows, dwords

    // LDS: luma tap records [rows][nYp] | chroma tap records [rows][nYpC] | work rows [rows][rowPitch]
    uint2 *const taps = reinterpret_cast<uint2 *>(roi_yuv_lds);
    uint2 *const tapsC = taps + rows * nYp;
    uint32_t *const work = roi_yuv_lds + 2 * rows * (nYp + nYpC);
    uint16_t *const work16 = reinterpret_cast<uint16_t *>(work);

    roi_stage_taps(taps, yt, ih, y0, nRows, stY, tid);
    roi_stage_taps(tapsC, ytC, ih, y0, nRows, stC, tid);
    lds_barrier();

    // 1. vertical pass: Y, then the chroma plane(s)
    const int wc = w >> 1;
    roi_vertical<LZ, RoiStorePlanar>(a.y + off, stY, w, bx, rowBY, taps, yt, y0, nRows, work, rowPitch, 0, padL, tid);
    if constexpr (UV2) {
        roi_vertical<LZ, RoiStorePairs>(a.u + offC, stC, w, bx, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, pitchC,
                                        padLc, tid);
    } else {
        roi_vertical<LZ, RoiStorePlanar>(a.u + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, 0,
                                         padLc, tid);
        roi_vertical<LZ, RoiStorePlanar>(a.v + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY + pitchC,
                                         rowPitch, 0, padLc, tid);
    }
    lds_barrier();
    // work columns outside the box: its clamped edge column, in each of the three rows
    {
        const int nPadY = 2 * pitchY - w, nPadC = 2 * pitchC - wc, nPad = nPadY + 2 * nPadC;
        for (int t = tid; t < nRows * nPad; t += 256) {
            const int j = t / nPad;
            int k = t - j * nPad;
            uint16_t *wr = work16 + 2 * j * rowPitch;
            int pl = padL, n = w;
            if (k >= nPadY) {
                k -= nPadY;
                wr += 2 * pitchY;
                pl = padLc;
                n = wc;
                if (k >= nPadC) {
                    k -= nPadC;
                    wr += 2 * pitchC;
                }
            }
            roi_edge_fill(wr, k, pl, n);
        }
    }
    lds_barrier();

    // 2. horizontal pass
    const int2 *const col = reinterpret_cast<const int2 *>(xt + 4);     // {even window start, divisor}
    const int2 *const colC = reinterpret_cast<const int2 *>(xtC + 4);
    const uint32_t *const cx = xt + 4 + 2 * iw;
    const uint32_t *const cxC = xtC + 4 + 2 * iw;
    for (int t = tid; t < nRows * iw; t += 256) {
        const int j = t / iw, x = t - j * iw;
        const int2 cr = col[x], cc = colC[x];
        const uint32_t *const wj = work + j * rowPitch;
        const uint32_t *const wpC = wj + pitchY + ((cc.x + padLc) >> 1);
        int Y, U, V;
        roi_horizontal<LZ, 1>(wj + ((cr.x + padL) >> 1), 0, cx, NP, iw, x, cr.y, &Y);
        roi_horizontal<LZ, 1>(wpC, 0, cxC, NPc, iw, x, cc.y, &U);
        roi_horizontal<LZ, 1>(wpC + pitchC, 0, cxC, NPc, iw, x, cc.y, &V);
        // (R, G, B, 255): the shift and both clamps of yuv_to_rgb in two v_ashr_pk_u8_i32, as yuv_rgb_kernel's
        // rgb_word.  (Written as shifts and clamps, the combiner folds a pair into that instruction and leaves its
        // undefined half in the word: kernels_dev.hpp opaque)
        int sr, sg, sb;
        yuv_sums(a.k, Y, yuv_chroma_terms(a.k, U, V), sr, sg, sb);
        const uint32_t px = ashr_pk_hi<kYuvRgbShift>(ashr_pk_lo<kYuvRgbShift>(sr, sg), sb, 255 << kYuvRgbShift);
        const int xo = ox + (flip ? iw - 1 - x : x);
        uint8_t *const o = canvas + static_cast<int64_t>(oy + y0 + j) * a.dstSt;
        if constexpr (NORM) {
            const NormDev &n = a.n;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= n.planes)
                    break;
                roi_store_norm(n, p, (px >> (8 * n.order[p])) & 0xffu, xo, o);
            }
        } else {
            const uint32_t out = __builtin_amdgcn_perm(0u, px, a.sel);
            uint8_t *const e = o + xo * a.channels;
            if (a.channels == 4 && !(reinterpret_cast<uintptr_t>(e) & 3)) {
                *reinterpret_cast<uint32_t *>(e) = out;
            } else {
                e[0] = static_cast<uint8_t>(out);
                e[1] = static_cast<uint8_t>(out >> 8);
                e[2] = static_cast<uint8_t>(out >> 16);
                if (a.channels == 4)
                    e[3] = static_cast<uint8_t>(out >> 24);
            }
        }
    }
}

template <bool NORM, bool FIT>
const void *roi_yuv_fn(bool lanczos, bool uv2)
{
#define IQO_ROI_YUV(LZ_, UV2_)                                                         \
    (FIT ? reinterpret_cast<const void *>(roi_yuv_fit_kernel<LZ_, UV2_, NORM>) \
         : reinterpret_cast<const void *>(roi_yuv_kernel<LZ_, UV2_, NORM>))
    if (lanczos)
        return uv2 ? IQO_ROI_YUV(true, true) : IQO_ROI_YUV(true, false);
    return uv2 ? IQO_ROI_YUV(false, true) : IQO_ROI_YUV(false, false);
#undef IQO_ROI_YUV
}

} // namespace

hipError_t launch_roi_yuv(const RoiYuvDev &d, const NormDev *norm, hipStream_t s)
{
    if (d.groups == 0)
        return hipSuccess;
    if (d.ldsBytes > static_cast<size_t>(kRoiLdsMax) || (d.channels != 3 && d.channels != 4))
        return hipErrorInvalidValue;
    RoiYuvFitNormArgs a;
    a.arena = d.arena;
    a.y = d.y;
    a.u = d.u;
    a.v = d.v;
    a.dst = d.dst;
    a.dstSt = d.dstSt;
    a.dstRoiSt = d.dstRoiSt;
    a.k = d.k;
    a.channels = d.channels;
    a.sel = 0;
    for (int c = 0; c < 4; ++c) {
        if (c < d.channels && (d.order[c] < 0 || d.order[c] > 3))
            return hipErrorInvalidValue;
        a.sel |= (c < d.channels ? static_cast<uint32_t>(d.order[c]) : 0x0cu) << (8 * c);
    }
    if (norm)
        for (int p = 0; p < norm->planes; ++p)
            if (norm->order[p] < 0 || norm->order[p] > 2)
                return hipErrorInvalidValue;
    a.pad = static_cast<uint32_t>(d.pad[0]) | (static_cast<uint32_t>(d.pad[1]) << 8) | (static_cast<uint32_t>(d.pad[2]) << 16) |
            0xff000000u;
    if (d.fit) {
        const void *kern = norm ? roi_yuv_fn<true, true>(d.lanczos, d.interleavedUV) : roi_yuv_fn<false, true>(d.lanczos, d.interleavedUV);
        return roi_launch<RoiYuvFitArgs>(kern, a, norm, d.groups, d.ldsBytes, s);
    }
    const void *kern = norm ? roi_yuv_fn<true, false>(d.lanczos, d.interleavedUV) : roi_yuv_fn<false, false>(d.lanczos, d.interleavedUV);
    RoiYuvNormArgs b;
    static_cast<RoiYuvArgs &>(b) = a;
    return roi_launch<RoiYuvArgs>(kern, b, norm, d.groups, d.ldsBytes, s);
}

} // namespace iqo_amd
