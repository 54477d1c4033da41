// kernels_roi_yuv.hip -- gfx950 kernel of the batched crop-and-resize of NV12 / I420 frames straight to RGB
// (iqo_hip_resize_rois_yuv_rgb_device / _norm_device): N boxes of N sizes, each to dstW x dstH, in one launch.
//
//   roi_yuv_kernel<LZ, UV2, NORM>   LZ: Lanczos (signed 16-bit work) or Area / Linear (unsigned)
//                                   UV2: interleaved UV plane (NV12) or separate U and V planes (I420)
//                                   NORM: packed bytes out, or the normalised planar float epilogue
//
// roi_kernel (kernels_roi.hip) three times over in one workgroup: a band of output rows of one box, found by
// the same search in the call's ARENA (roi.hpp, the YUV format), gets a Y work row from the box's luma tables
// (w -> dstW, h -> dstH) and a U and a V work row from its chroma tables (w/2 -> dstW, h/2 -> dstH), so all
// three components arrive on the output grid.
//   1. vertical: roi_kernel's C = 1 task -- (row of the band, 8 consecutive bytes of a plane's row), fetched
//      as aligned words where those lie inside THAT PLANE's row and as clamped single bytes at its ends --
//      on Y, and on U and on V (I420), or on the UV plane (NV12), where the 8 bytes are 4 (U, V) pairs and
//      each v_pk_mad_u16 accumulates one pair: its halves go to the U and the V row.
//   2. horizontal: a thread owns one output pixel: NP dot products on the Y row, NPc on each of the U and V
//      rows, each component's own shift or border division and clamp, then colorspace.hpp's integer matrix
//      and the store (mirrored when the box is flagged).
// The three work rows of a band row lie one after the other, pitchY + 2 pitchC dwords: odd, as each pitch is.
#include "kernels_dev.hpp"
#include "roi.hpp"

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

// Tap records of a band: [nRows][nYp] {coefficient splat, byte offset of the clamped row}
__device__ __forceinline__ void stage_taps(uint2 *taps, const uint32_t *yt, int dstH, int y0, int nRows, int st, int tid)
{
    const int nYp = sld(yt, 0);
    const int32_t *const rowRec = reinterpret_cast<const int32_t *>(yt + 4);
    const uint32_t *const cy = yt + 4 + 4 * dstH;
    for (int t = tid; t < nRows * nYp; t += 256) {
        const int j = t / nYp, k = t - j * nYp, y = y0 + j;
        const int rr = max(rowRec[4 * y + 1], min(rowRec[4 * y] + k, rowRec[4 * y + 2]));
        const uint32_t c = (cy[y * (nYp >> 1) + (k >> 1)] >> (16 * (k & 1))) & 0xffffu;
        taps[t] = make_uint2(c | (c << 16), static_cast<uint32_t>(rr * st));
    }
}

// Vertical pass over one plane of the box: nB bytes per row from `box` (byte xB of the plane's rows of rowB
// bytes, st apart).  PAIRS: the bytes are (U, V) pairs, sample s of U goes to work16 entry padL + s of row
// `work`, of V to that of row `work + vOff`; otherwise byte s is sample s of row `work`.  Band row j's rows lie
// j * rowPitch dwords on.
template <bool LZ, bool PAIRS>
__device__ __forceinline__ void vertical(const uint8_t *box, int st, int nB, int xB, int rowB, const uint2 *taps,
                                         const uint32_t *yt, int y0, int nRows, uint32_t *work, int rowPitch, int vOff,
                                         int padL, int tid)
{
    const int nYp = sld(yt, 0);
    const int32_t *const rowRec = reinterpret_cast<const int32_t *>(yt + 4);
    const int nG = (nB + 7) >> 3;
    // rows a multiple of 4 bytes apart: a task's misalignment, and whether its aligned words lie inside the
    // plane's row, are the same for every tap
    const bool rowsAligned = !(st & 3);
    // 8 bytes at p (box byte 8 g of some row) as two words.  fast: the 2 (mis == 0) or 3 aligned words they
    // lie in are inside the plane's row; otherwise single bytes, clamped to the box's last byte
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
        return s >= 0 && s + (mis ? 12 : 8) <= rowB;
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
        uint32_t *const wr = work + j * rowPitch;
        uint16_t *const wr16 = reinterpret_cast<uint16_t *>(wr);
        const bool whole = 8 * g + 8 <= nB;
        if constexpr (PAIRS) {
            if (whole) {  // 4 pairs: two dwords of the U row and two of the V row (padL is even)
                uint32_t *wd = wr + ((padL + 4 * g) >> 1);
                wd[0] = __builtin_amdgcn_perm(acc[1], acc[0], 0x05040100u);
                wd[1] = __builtin_amdgcn_perm(acc[3], acc[2], 0x05040100u);
                wd[vOff] = __builtin_amdgcn_perm(acc[1], acc[0], 0x07060302u);
                wd[vOff + 1] = __builtin_amdgcn_perm(acc[3], acc[2], 0x07060302u);
            } else {
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    if (8 * g + 2 * m < nB) {  // (nB is even: a pair is whole)
                        wr16[padL + 4 * g + m] = static_cast<uint16_t>(acc[m]);
                        wr16[2 * vOff + padL + 4 * g + m] = static_cast<uint16_t>(acc[m] >> 16);
                    }
            }
        } else {
            if (whole) {  // the pairs are the work row's dwords (padL is even)
                uint32_t *wd = wr + ((padL + 8 * g) >> 1);
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    wd[m] = acc[m];
            } else {
#pragma unroll
                for (int b = 0; b < 8; ++b)
                    if (8 * g + b < nB)
                        wr16[padL + 8 * g + b] = static_cast<uint16_t>(acc[b >> 1] >> (16 * (b & 1)));
            }
        }
    }
}

// A component's byte of one output pixel: NP dot products on its work row from dword `wp`, then the rounding
// shift or the exact border division, and the clamp.
template <bool LZ>
__device__ __forceinline__ int horizontal(const uint32_t *wp, const uint32_t *cx, int NP, int dstW, int x, int div)
{
    int s = LZ ? (1 << 19) : (1 << 22);
    for (int p = 0; p < NP; ++p) {
        const uint32_t cf = cx[p * dstW + x];
        s = LZ ? sdot2(wp[p], cf, s) : static_cast<int>(udot2(wp[p], cf, static_cast<uint32_t>(s)));
    }
    if (LZ) {
        int v = s >> 20;
        if (div != 0)
            v = static_cast<int16_t>(exact_div(s, div));
        return min(max(v, 0), 255);
    }
    return static_cast<int>(min((static_cast<uint32_t>(s) >> 23) & 0xffffu, 255u));
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

    // the workgroup's box: the last record whose first workgroup is <= wg, by a 64-way search (every
    // wave runs it; a batch of 4096 boxes takes two rounds)
    int roi = 0;
    {
        int n = sld(A, kHRois);
        while (n > 1) {
            const int step = (n + 63) >> 6;
            const int i = lane * step;
            const bool le = i < n && rec0[static_cast<size_t>(roi + i) * kRoiYuvRecWords + kYFirst] <= wg;
            const int k = __popcll(__ballot(le)) - 1;  // lane 0 always holds: first(roi) <= wg
            roi = __builtin_amdgcn_readfirstlane(roi + k * step);
            n = __builtin_amdgcn_readfirstlane(min(step, n - k * step));
        }
    }
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

    stage_taps(taps, yt, dstH, y0, nRows, stY, tid);
    stage_taps(tapsC, ytC, dstH, y0, nRows, stC, tid);
    lds_barrier();

    // 1. vertical pass: Y, then the chroma plane(s)
    const int wc = w >> 1;
    vertical<LZ, false>(a.y + off, stY, w, bx, rowBY, taps, yt, y0, nRows, work, rowPitch, 0, padL, tid);
    if constexpr (UV2) {
        vertical<LZ, true>(a.u + offC, stC, w, bx, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, pitchC, padLc, tid);
    } else {
        vertical<LZ, false>(a.u + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY, rowPitch, 0, padLc, tid);
        vertical<LZ, false>(a.v + offC, stC, wc, bx >> 1, rowBC, tapsC, ytC, y0, nRows, work + pitchY + pitchC, rowPitch, 0,
                            padLc, tid);
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
            wr[k < pl ? k : n + k] = wr[k < pl ? pl : pl + n - 1];
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
        const int Y = horizontal<LZ>(wj + ((cr.x + padL) >> 1), cx, NP, dstW, x, cr.y);
        const int U = horizontal<LZ>(wpC, cxC, NPc, dstW, x, cc.y);
        const int V = horizontal<LZ>(wpC + pitchC, cxC, NPc, dstW, x, cc.y);
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
                const float f = norm_affine((px >> (8 * n.order[p])) & 0xffu, n.scale[p], n.bias[p]);
                uint8_t *const e = o + static_cast<int64_t>(p) * n.planeSt;
                if (n.dtype == 1)
                    reinterpret_cast<float *>(e)[xo] = f;
                else
                    reinterpret_cast<uint16_t *>(e)[xo] = static_cast<uint16_t>(n.dtype == 2 ? f16_bits(f) : bf16_bits(f));
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

template <bool NORM>
const void *roi_yuv_fn(bool lanczos, bool uv2)
{
#define IQO_ROI_YUV(LZ_, UV2_) reinterpret_cast<const void *>(roi_yuv_kernel<LZ_, UV2_, NORM>)
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
    RoiYuvNormArgs a;
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
    const void *kern = norm ? roi_yuv_fn<true>(d.lanczos, d.interleavedUV) : roi_yuv_fn<false>(d.lanczos, d.interleavedUV);
    RoiYuvArgs u = a;
    void *args[] = {&u};
    if (norm) {
        a.n = *norm;
        args[0] = &a;
    }
    return hipLaunchKernel(kern, dim3(d.groups), dim3(256), args, d.ldsBytes, s);
}

} // namespace iqo_amd
