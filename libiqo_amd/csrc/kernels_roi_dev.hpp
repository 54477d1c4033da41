// kernels_roi_dev.hpp -- the band pipeline of both box kernels (kernels_roi.hip roi_kernel, kernels_roi_yuv.hip
// roi_yuv_kernel): a workgroup finds its box and band of output rows in the call's ARENA (roi.hpp), stages the
// band's tap records, and runs two passes through LDS, as packed_tile_kernel:
//   1. vertical: a task is (output row of the band, 8 consecutive bytes of a row of the box in one plane).  The
//      8 bytes come from the 2 or 3 aligned words they lie in (v_alignbyte_b32) where those words are inside
//      the plane's row, and from single clamped byte loads at the row's two ends, so no byte outside the
//      plane's rows is ever read; rows are clamped to the box.  Four v_pk_mad_u16 per tap (the low 16 bits
//      are the reference's wrap), the exact division on masked border rows, and the 8 values go to the work
//      row(s) by the caller's STORE policy.  Work columns left and right of the box are then filled with the
//      box's edge column (never with the plane's bytes there).
//   2. horizontal: a thread owns one output pixel: its coefficient pairs are loaded once (coalesced: the arena
//      keeps them pair-major) and each pair is one v_dot2 on an aligned dword of each of its work rows; then
//      the rounding shift or the exact border division, and the clamp.
// Everything here is inlined into its kernel, and every value that is uniform over the workgroup is read
// with sld.
#pragma once

#include "kernels_dev.hpp"
#include "roi.hpp"

namespace iqo_amd {
namespace {

// The workgroup's box: the last record whose first workgroup (word FIRST_WORD of REC_WORDS) is <= wg, by a
// 64-way search (every wave runs it; a batch of 4096 boxes takes two rounds)
template <int REC_WORDS, int FIRST_WORD>
__device__ __forceinline__ int roi_find_box(const uint32_t *rec0, int n, uint32_t wg, int lane)
{
    int roi = 0;
    while (n > 1) {
        const int step = (n + 63) >> 6;
        const int i = lane * step;
        const bool le = i < n && rec0[static_cast<size_t>(roi + i) * REC_WORDS + FIRST_WORD] <= wg;
        const int k = __popcll(__ballot(le)) - 1;  // lane 0 always holds: first(roi) <= wg
        roi = __builtin_amdgcn_readfirstlane(roi + k * step);
        n = __builtin_amdgcn_readfirstlane(min(step, n - k * step));
    }
    return roi;
}

// Tap records of a band: [nRows][nYp] {coefficient splat, byte offset of the clamped row}
__device__ __forceinline__ void roi_stage_taps(uint2 *taps, const uint32_t *yt, int dstH, int y0, int nRows, int st, int tid)
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

// STORE policies of roi_vertical: where the 8 values acc[0..3] (two 16-bit halves each) of box bytes
// [8 g, 8 g + 8) of band row j go; nB: the row's bytes.  Band row j's work rows lie j * rowPitch dwords on from
// `work`, and a sample s is work16 entry padL + s of its row.
//
// planar: byte s is sample s of the row at `work`.
struct RoiStorePlanar {
    static __device__ __forceinline__ void put(int nB, uint32_t *work, int rowPitch, int, int padL, int j, int g,
                                               const uint32_t (&acc)[4])
    {
        uint32_t *const wr = work + j * rowPitch;
        uint16_t *const wr16 = reinterpret_cast<uint16_t *>(wr);
        if (8 * g + 8 <= nB) {  // the pairs are the work row's dwords (padL is even)
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
};
// pairs: the bytes are (U, V) pairs; sample s of U goes to the row at `work`, of V to the row vOff dwords on.
struct RoiStorePairs {
    static __device__ __forceinline__ void put(int nB, uint32_t *work, int rowPitch, int vOff, int padL, int j, int g,
                                               const uint32_t (&acc)[4])
    {
        uint32_t *const wr = work + j * rowPitch;
        uint16_t *const wr16 = reinterpret_cast<uint16_t *>(wr);
        if (8 * g + 8 <= nB) {  // 4 pairs: two dwords of the U row and two of the V row (padL is even)
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
    }
};
// interleaved: byte q is channel q % C of pixel q / C; a band row's C work rows lie vOff dwords apart.
template <int C>
struct RoiStoreInterleaved {
    static __device__ __forceinline__ void put(int nB, uint32_t *work, int rowPitch, int vOff, int padL, int j, int g,
                                               const uint32_t (&acc)[4])
    {
        uint16_t *const wr16 = reinterpret_cast<uint16_t *>(work + j * rowPitch);
#pragma unroll
        for (int b = 0; b < 8; ++b) {
            const int q = 8 * g + b;
            if (q < nB) {
                const int px = q / C, ch = q - px * C;
                wr16[2 * ch * vOff + padL + px] = static_cast<uint16_t>(acc[b >> 1] >> (16 * (b & 1)));
            }
        }
    }
};

// Vertical pass over one plane of the box: nB bytes per row from `box` (byte xB of the plane's rows of rowB
// bytes, st apart), by the tap records of the band and the row records of Y table yt; work, rowPitch, vOff and
// padL are Store's.
template <bool LZ, typename Store>
__device__ __forceinline__ void roi_vertical(const uint8_t *box, int st, int nB, int xB, int rowB, const uint2 *taps,
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
        Store::put(nB, work, rowPitch, vOff, padL, j, g, acc);
    }
}

// Work column k of the nPad outside a box of n columns behind pl left ones: its clamped edge column
__device__ __forceinline__ void roi_edge_fill(uint16_t *wr, int k, int pl, int n)
{
    wr[k < pl ? k : n + k] = wr[k < pl ? pl : pl + n - 1];
}

// Output column x of N work rows `stride` dwords apart, from dword `wp` of the first: NP dot products each, on
// coefficient pairs loaded once for all N, then the rounding shift or the exact border division, and the clamp.
template <bool LZ, int N, typename T>
__device__ __forceinline__ void roi_horizontal(const uint32_t *wp, int stride, const uint32_t *cx, int NP, int dstW, int x,
                                               int div, T *out)
{
    int s[N];
#pragma unroll
    for (int c = 0; c < N; ++c)
        s[c] = LZ ? (1 << 19) : (1 << 22);
    for (int p = 0; p < NP; ++p) {
        const uint32_t cf = cx[p * dstW + x];
#pragma unroll
        for (int c = 0; c < N; ++c)
            s[c] = LZ ? sdot2(wp[c * stride + p], cf, s[c])
                      : static_cast<int>(udot2(wp[c * stride + p], cf, static_cast<uint32_t>(s[c])));
    }
#pragma unroll
    for (int c = 0; c < N; ++c) {
        if (LZ) {
            int v = s[c] >> 20;
            if (div != 0)
                v = static_cast<int16_t>(exact_div(s[c], div));
            out[c] = static_cast<T>(min(max(v, 0), 255));
        } else {
            out[c] = static_cast<T>(min((static_cast<uint32_t>(s[c]) >> 23) & 0xffffu, 255u));
        }
    }
}

// Plane p of the float epilogue: byte v of the pixel at column xo of output row `o`
__device__ __forceinline__ void roi_store_norm(const NormDev &n, int p, uint32_t v, int xo, uint8_t *o)
{
    const float f = norm_affine(v, n.scale[p], n.bias[p]);
    uint8_t *const e = o + static_cast<int64_t>(p) * n.planeSt;
    if (n.dtype == 1)
        reinterpret_cast<float *>(e)[xo] = f;
    else
        reinterpret_cast<uint16_t *>(e)[xo] = static_cast<uint16_t>(n.dtype == 2 ? f16_bits(f) : bf16_bits(f));
}

// ---------------------------------------------------------------- the fit kernels' pad stores
//
// A pad run is a row of equal pixels (U8, 1, 3 or 4 bytes) or equal elements (fp32 / fp16 / bf16) that begins on
// a pixel: its byte k is byte k % period of the pixel.  The pattern is the run's first 8 bytes as one 64-bit value,
// uniform over the workgroup, so the 4 bytes at any k are a shift of it by k % period bytes (at most 3): plain
// register arithmetic, no table.
struct RoiPadPat {
    uint64_t d;  // bytes 0 .. 7 of a run
    int period;  // 1 .. 4
};

// The pattern of a pixel or element of `period` bytes (1 .. 4), the low bytes of px
__device__ __forceinline__ RoiPadPat roi_pad_pattern(uint32_t px, int period)
{
    uint64_t d;
    if (period == 3) {
        const uint64_t p = px & 0xffffffu;
        d = p | (p << 24) | (p << 48);
    } else {
        const uint32_t w = period == 1 ? (px & 0xffu) * 0x01010101u : period == 2 ? (px & 0xffffu) * 0x00010001u : px;
        d = w | (static_cast<uint64_t>(w) << 32);
    }
    return RoiPadPat{d, period};
}

// ... of plane p of the float epilogue: the element roi_store_norm stores for byte v
__device__ __forceinline__ RoiPadPat roi_pad_pattern_norm(const NormDev &n, int p, uint32_t v)
{
    const float f = norm_affine(v, n.scale[p], n.bias[p]);
    if (n.dtype == 1)
        return roi_pad_pattern(__float_as_uint(f), 4);
    return roi_pad_pattern(static_cast<uint32_t>(n.dtype == 2 ? f16_bits(f) : bf16_bits(f)) & 0xffffu, 2);
}

// nRows pad runs of nBytes each, rowSt apart from `base`, by the whole workgroup.  A task is one 16-byte aligned
// slot of one row: a slot wholly inside the run is one 16-byte store (a 3-byte pixel so sees a 48-byte pattern
// rotate through three slots), the two slots at a run's misaligned ends are stores of `unit` bytes (1: bytes; 2, 4: the
// element size, which base, rowSt and nBytes are multiples of).  Every byte of the runs is stored once, and no other.
__device__ __forceinline__ void roi_pad_rows(uint8_t *base, int64_t rowSt, int nRows, int nBytes, RoiPadPat pat, int unit,
                                             int tid)
{
    if (nRows <= 0 || nBytes <= 0)
        return;
    const uint64_t d = pat.d;
    const int period = pat.period;
    // bytes [k, k + 4) of the run, k >= 0
    auto word = [=](int k) {
        const int r = period == 3 ? k % 3 : k & (period - 1);
        return static_cast<uint32_t>(d >> (8 * r));
    };
    const int nSlots = ((nBytes + 15) >> 4) + 1;
    for (int t = tid; t < nRows * nSlots; t += 256) {
        const int j = t / nSlots, s = t - j * nSlots;
        uint8_t *const p = base + j * rowSt;
        const int b0 = 16 * s - static_cast<int>(reinterpret_cast<uintptr_t>(p) & 15);  // the slot's first run byte
        const int lo = max(b0, 0), hi = min(b0 + 16, nBytes);
        if (hi - lo == 16) {
            *reinterpret_cast<uint4 *>(p + b0) = make_uint4(word(b0), word(b0 + 4), word(b0 + 8), word(b0 + 12));
        } else {
            for (int k = lo; k < hi; k += unit) {
                const uint32_t v = word(k);
                if (unit == 4)
                    *reinterpret_cast<uint32_t *>(p + k) = v;
                else if (unit == 2)
                    *reinterpret_cast<uint16_t *>(p + k) = static_cast<uint16_t>(v);
                else
                    p[k] = static_cast<uint8_t>(v);
            }
        }
    }
}

// What a fit workgroup is to its box, from the fit words `ext` of the box's record (roi.hpp RoiFitRec): a band
// (true: *y0 is its first row of the rectangle), or a pad workgroup above or below the rectangle (false: it writes
// canvas rows [*y0, *y1)).  k: the workgroup's number within its box; g: the box's bands of `rows` rows.
__device__ __forceinline__ bool roi_fit_role(const uint32_t *ext, int k, int g, int rows, int dstH, int *y0, int *y1)
{
    const int above = sld(ext, kFPadAbove), oy = sld(ext, kFOY), ih = sld(ext, kFIH);
    if (k < above) {
        *y0 = k * kRoiPadRows;
        *y1 = min(*y0 + kRoiPadRows, oy);
        return false;
    }
    if (k >= above + g) {
        *y0 = oy + ih + (k - above - g) * kRoiPadRows;
        *y1 = min(*y0 + kRoiPadRows, dstH);
        return false;
    }
    *y0 = (k - above) * rows;
    *y1 = min(*y0 + rows, ih);
    return true;
}

// Launches `kern` over the arena's workgroups on its Args slice of `a`, or with `norm` on the whole of it.
template <typename Args, typename NormArgs>
hipError_t roi_launch(const void *kern, NormArgs &a, const NormDev *norm, unsigned groups, size_t ldsBytes, hipStream_t s)
{
    Args u = a;
    void *args[] = {&u};
    if (norm) {
        a.n = *norm;
        args[0] = &a;
    }
    return hipLaunchKernel(kern, dim3(groups), dim3(256), args, ldsBytes, s);
}

} // namespace
} // namespace iqo_amd
