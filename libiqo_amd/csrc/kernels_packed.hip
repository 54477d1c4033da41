// kernels_packed.hip -- gfx950 kernels for packed (interleaved) U8 pixels: C = 2 .. 4 bytes per
// pixel (UV of NV12, RGB, RGBA), every channel resized independently, so channel c of the output
// is byte-identical to the planar resize of channel c (kernels.hip, and through it the
// reference's Generic fixed point).
//
//   packed_general_kernel   any shape, any alignment: general_kernel (kernels.hip) per channel
//   packed_tile_kernel      the hot path: tile_kernel's two passes through LDS over the same
//                           host tables, with the work rows de-interleaved per channel
//
// Both also come with a float epilogue (NORM): instead of the interleaved bytes they store planar
// fp32 / fp16 / bf16 planes of (byte * scale + bias), channels picked and ordered by the caller
// (kernels.hpp NormDev).  The bytes are the U8 path's; only the end of the horizontal pass differs.
#include "kernels_dev.hpp"

namespace iqo_amd {
namespace {

// ================================================================ packed general kernel
//
// general_kernel with source byte (row, col * C + c) and output byte x * C + c: one workgroup per
// (output row, frame, channel).  y_value / x_value restate kernels.hip:29-123 (the reference lines
// are cited there).

enum { KMAIN = 0, KLO = 1, KHI = 2, KID = 3 };

struct PackedGeneralArgs {
    GeneralDev g;
    Io io;
    int rowBegin;
    int C;
};

__device__ __forceinline__ int src_px(const PackedGeneralArgs &a, const uint8_t *srcC, int row, int col)
{
    return srcC[static_cast<int64_t>(row - a.io.srcRow0) * a.io.srcSt + col * a.C];
}

// Vertical value at (row record yi, source pixel col) of the channel srcC points at.
__device__ int y_value(const PackedGeneralArgs &a, const uint8_t *srcC, int4 yi, int col)
{
    const GeneralDev &g = a.g;
    if (g.method == 0) {  // Lanczos, int16 work row
        if (yi.z == KID)
            return static_cast<int16_t>(static_cast<uint16_t>(src_px(a, srcC, yi.x, col) * 64));
        if (yi.z == KMAIN) {
            int16_t acc = 0;
            for (int i = 0; i < g.nY; ++i)
                acc = static_cast<int16_t>(acc + src_px(a, srcC, yi.x + i, col) * g.tabY[yi.y + i]);
            return acc;
        }
        int16_t nume = 0;
        for (int i = 0; i < g.nY; ++i) {
            int r = yi.x + i;
            if (r >= 0 && r < g.srcH)
                nume = static_cast<int16_t>(nume + src_px(a, srcC, r, col) * g.tabY[yi.y + i]);
        }
        return static_cast<int16_t>(exact_div(static_cast<int>(nume) * 64, yi.w));
    }
    if (yi.z == KID)
        return static_cast<uint16_t>(src_px(a, srcC, yi.x, col) * 256);
    if (g.method == 1) {  // Area, u16 work row; weight-0 tap past the end clamped
        uint16_t acc = 0;
        for (int i = 0; i < g.nY; ++i) {
            int r = min(yi.x + i, g.srcH - 1);
            acc = static_cast<uint16_t>(acc + src_px(a, srcC, r, col) * g.tabY[yi.y + i]);
        }
        return acc;
    }
    // Linear
    if (yi.z == KLO)
        return static_cast<uint16_t>(src_px(a, srcC, 0, col) * 256);
    if (yi.z == KHI)
        return static_cast<uint16_t>(src_px(a, srcC, g.srcH - 1, col) * 256);
    int r0 = max(0, min(yi.x, g.srcH - 1)), r1 = max(0, min(yi.x + 1, g.srcH - 1));
    uint16_t acc = static_cast<uint16_t>(src_px(a, srcC, r0, col) * g.tabY[yi.y]);
    acc = static_cast<uint16_t>(acc + src_px(a, srcC, r1, col) * g.tabY[yi.y + 1]);
    return acc;
}

// Horizontal value of one output pixel (record xi) from the LDS work row covering pixels [lo, hi).
__device__ int x_value(const GeneralDev &g, const int *w, int lo, int hi, int4 xi)
{
    auto W = [&](int col) { return w[max(0, min(col, hi - 1) - lo)]; };
    if (g.method == 0) {
        if (xi.z == KID)
            return clamp255(static_cast<int16_t>((W(xi.x) + 32) >> 6));
        if (xi.z == KMAIN) {
            int sum = 0;
            for (int i = 0; i < g.nX; ++i)
                sum += W(xi.x + i) * g.tabX[xi.y + i];
            return clamp255(static_cast<int16_t>((sum + (1 << 19)) >> 20));
        }
        int nume = 0;
        for (int i = 0; i < g.nX; ++i) {
            int col = xi.x + i;
            if (col >= 0 && col < g.srcW)
                nume += W(col) * g.tabX[xi.y + i];
        }
        return clamp255(static_cast<int16_t>(exact_div(nume + (1 << 19), xi.w * 64)));
    }
    if (xi.z == KID)
        return clamp255(static_cast<int16_t>((W(xi.x) + 128) >> 8));
    auto u16clamp = [](int v) {  // uint8(clamp<uint16_t>(0, 255, int16(v)))
        uint16_t u = static_cast<uint16_t>(static_cast<int16_t>(v));
        return static_cast<int>(u > 255 ? 255 : u);
    };
    if (g.method == 1) {
        int sum = 0;
        for (int i = 0; i < g.nX; ++i)
            sum += W(min(xi.x + i, g.srcW - 1)) * g.tabX[xi.y + i];
        return u16clamp((sum + (1 << 22)) >> 23);
    }
    if (xi.z == KLO)
        return u16clamp((W(0) + 128) >> 8);
    if (xi.z == KHI)
        return u16clamp((W(g.srcW - 1) + 128) >> 8);
    int c0 = max(0, min(xi.x, g.srcW - 1)), c1 = max(0, min(xi.x + 1, g.srcW - 1));
    int sum = W(c0) * g.tabX[xi.y] + W(c1) * g.tabX[xi.y + 1];
    return u16clamp((sum + (1 << 22)) >> 23);
}

// ---- float epilogue (NORM)

struct PackedGeneralNormArgs : PackedGeneralArgs {
    NormDev n;
};

// (norm_affine, f16_bits, bf16_bits and pick4 are in kernels_dev.hpp: kernels_color.hip shares them)

// One workgroup per (output row, frame, channel); NORM: per (output row, frame, output plane),
// whose channel is order[plane].
template <bool NORM, typename Args>
__device__ __forceinline__ void packed_general_body(const Args &a, int *wrow)
{
    const int y = a.rowBegin + static_cast<int>(blockIdx.x);
    int c = static_cast<int>(blockIdx.z);  // the workgroup's channel
    int64_t dstOff = c;
    float scale = 0.f, bias = 0.f;
    int dtype = 0;
    if constexpr (NORM) {
        const int p = c;
        c = pick4(a.n.order, p);
        scale = pick4(a.n.scale, p);
        bias = pick4(a.n.bias, p);
        dtype = a.n.dtype;
        dstOff = static_cast<int64_t>(p) * a.n.planeSt;
    }
    const uint8_t *srcC = a.io.src + static_cast<int64_t>(blockIdx.y) * a.io.srcFrameSt + c;
    uint8_t *dstRow = a.io.dst + static_cast<int64_t>(blockIdx.y) * a.io.dstFrameSt +
                      static_cast<int64_t>(y - a.io.dstRow0) * a.io.dstSt + dstOff;
    const int4 yi = a.g.yInfo[y];
    for (int k = 0; k < a.g.nChunks; ++k) {
        const int4 ch = a.g.chunks[k];
        for (int col = ch.z + static_cast<int>(threadIdx.x); col < ch.w; col += static_cast<int>(blockDim.x))
            wrow[col - ch.z] = y_value(a, srcC, yi, col);
        lds_barrier();
        const int x = ch.x + static_cast<int>(threadIdx.x);
        if (x < ch.y) {
            const int v = x_value(a.g, wrow, ch.z, ch.w, a.g.xInfo[x]);
            if constexpr (NORM) {
                const float f = norm_affine(static_cast<uint32_t>(v), scale, bias);
                uint8_t *o = dstRow + x * (dtype == 1 ? 4 : 2);
                if (dtype == 1)
                    *reinterpret_cast<float *>(o) = f;
                else
                    *reinterpret_cast<uint16_t *>(o) = static_cast<uint16_t>(dtype == 2 ? f16_bits(f) : bf16_bits(f));
            } else {
                dstRow[x * a.C] = static_cast<uint8_t>(v);
            }
        }
        lds_barrier();
    }
}

__global__ __launch_bounds__(256) void packed_general_kernel(PackedGeneralArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int wrow[];
    packed_general_body<false>(a, wrow);
}

__global__ __launch_bounds__(256) void packed_general_norm_kernel(PackedGeneralNormArgs a)
{
    extern __shared__ __attribute__((aligned(16))) int wrow_n[];
    packed_general_body<true>(a, wrow_n);
}

// ================================================================ packed tile kernel
//
// tile_kernel (kernels.hip) for C interleaved channels.  A workgroup computes TH output rows x CT
// output PIXELS of one frame:
//   0. stage: the tile's source rows x pixels [lo8, lo8 + 8 * groups) as packed bytes.  A packed
//      row is a planar row of srcW * C bytes, so the interior is the same burst of 8-byte loads
//      (any alignment: 12 dword-aligned bytes and a byte shift).  Only the edges know about
//      pixels: a staged byte left of pixel 0 or right of pixel srcW - 1 is the byte of the SAME
//      channel of that edge pixel, fetched as single clamped bytes.
//   1. vertical: one task = (output row, 8 pixels): per tap 8 * C staged bytes, and for every
//      channel four v_perm that pick the channel's pixel pairs out of two adjacent dwords (bytes
//      C apart; the selectors are compile-time constants) and four v_pk_mad_u16 -- the arithmetic
//      per byte of tile_kernel.  The channel's 8 work values go to ITS segment of the work row
//      (one 16-byte LDS store), so the work row is de-interleaved: [row][channel][pixel].
//   2. horizontal: a thread owns 4 adjacent output pixels of all C channels; its coefficient pairs
//      and window offsets are loaded once and shared by the channels.  Per channel the planar
//      pass runs on the channel's segment (NP v_dot2 per pixel); the 4 * C output bytes leave as
//      one 8 / 12 / 16-byte store (single bytes at the right edge or on an unaligned destination).

struct PackedTileArgs {
    TileDev t;
    Io io;
    int rowBegin, rowEnd;
    int srcBytes, dstBytes;
    int nTx, nTy;
    unsigned nTiles;
};

// v_perm selector of pixel pair m (pixels 2m, 2m + 1 of a group of 8) of channel c: the pair's
// bytes b0 = 2m C + c and b0 + C lie in dword b0 / 4 or the next one
template <int C>
__device__ __forceinline__ constexpr uint32_t pair_sel(int m, int c)
{
    const int b0 = 2 * m * C + c, k = b0 >> 2;
    return static_cast<uint32_t>(b0 - 4 * k) | (static_cast<uint32_t>(b0 + C - 4 * k) << 16) | 0x0c000c00u;
}

struct PackedTileNormArgs : PackedTileArgs {  // dstBytes: the float frame's byte range
    NormDev n;
};

// NORM = false is the U8 kernel, argument layout included.  NORM = true ends the horizontal pass
// with the float epilogue: the thread's 4 pixels of every channel are in registers, so output plane
// p is 4 consecutive elements, one 16-byte (fp32) or 8-byte (fp16 / bf16) store.  order, scale, bias,
// the plane stride and the element type are kernel arguments (wave-uniform: SGPRs, a uniform branch
// around the conversion); every channel is still computed, order / planes only pick what is stored.
template <int C, int NP, bool LZ, bool NORM>
__global__ __launch_bounds__(256) void packed_tile_kernel(std::conditional_t<NORM, PackedTileNormArgs, PackedTileArgs> a)
{
    extern __shared__ __attribute__((aligned(16))) uint32_t ptile_lds[];
    const TileDev &t = a.t;
    const int tid = static_cast<int>(threadIdx.x);
    // XCD x takes a contiguous range of tiles, row tiles fastest (as tile_kernel)
    int tileX, tileY, frame;
    {
        const unsigned lg = xcd_chunks(blockIdx.x, a.nTx * a.nTy, a.nTiles);
        const unsigned rest = lg / static_cast<unsigned>(a.nTy);
        tileY = static_cast<int>(lg - rest * static_cast<unsigned>(a.nTy));
        frame = static_cast<int>(rest / static_cast<unsigned>(a.nTx));
        tileX = static_cast<int>(rest - static_cast<unsigned>(frame) * static_cast<unsigned>(a.nTx));
    }
    const int y0 = a.rowBegin + tileY * t.TH;
    const int nRows = min(t.TH, a.rowEnd - y0);
    // LDS: work rows [TH][C][pitchDw] | row records [TH] | tap records [TH][nYp] | border divisors
    // [CT] | source tile [srcRows][spitch].  Every section is a multiple of 16 bytes.
    uint32_t *const work = ptile_lds;
    int4 *const recs = reinterpret_cast<int4 *>(ptile_lds + t.TH * C * t.pitchDw);
    uint2 *const taps = reinterpret_cast<uint2 *>(recs + t.TH);
    int *const DL = reinterpret_cast<int *>(taps + t.TH * t.nYp);
    uint8_t *const srcL = reinterpret_cast<uint8_t *>(DL + t.CT);

    const uint8_t *srcFrame = a.io.src + static_cast<int64_t>(frame) * a.io.srcFrameSt;
    uint8_t *dstFrame = a.io.dst + static_cast<int64_t>(frame) * a.io.dstFrameSt;
    const int srcMis = static_cast<int>(reinterpret_cast<uintptr_t>(srcFrame) & 3);
    const bool srcA4 = srcMis == 0 && !(a.io.srcSt & 3);
    const bool dstA4 = !(reinterpret_cast<uintptr_t>(dstFrame) & 3) && !(a.io.dstSt & 3);
    const __amdgpu_buffer_rsrc_t srcR = __builtin_amdgcn_make_buffer_rsrc(
        const_cast<uint8_t *>(srcFrame - srcMis), 0, a.srcBytes + srcMis, 0x00020000);
    const __amdgpu_buffer_rsrc_t dstR = __builtin_amdgcn_make_buffer_rsrc(dstFrame, 0, a.dstBytes, 0x00020000);
    const int srcW = t.srcW, srcSt = static_cast<int>(a.io.srcSt), srcRow0 = a.io.srcRow0;
    const int4 sp = t.spans[tileX];  // {lo8 (pixel), 8-pixel groups, any border column}
    const int spitch = t.spitch;
    const int rmin = t.rows[y0].y;
    const int nR = t.rows[y0 + nRows - 1].z - rmin + 1;  // row windows are monotone

    // 0. stage source rows [rmin, rmin + nR) x packed bytes [lo8 * C, (lo8 + 8 groups) * C) in
    //    8-byte chunks.  Chunks [kLo, kHi) lie inside the row with 12 loadable bytes: whole-word
    //    loads; the others (left of pixel 0, the row's last bytes, right of it) byte by byte,
    //    replicating the edge PIXEL's channels.
    {
        const int nK = sp.y * C;         // chunks per staged row
        const int gb0 = sp.x * C;        // packed byte of staged byte 0 (negative at the left edge)
        const int rowB = srcW * C;
        const int kLo = gb0 < 0 ? min((-gb0 + 7) >> 3, nK) : 0;
        const int kNum = rowB - 12 - gb0;  // chunks with gb0 + 8 k + 12 <= rowB (floor division)
        const int kHi = kNum < 0 ? kLo : max(kLo, min(kNum / 8 + 1, nK));
        const int nF = kHi - kLo;
        const int total = nR * nF;
        const uint32_t mF = nF > 1 ? 0xffffffffu / static_cast<uint32_t>(nF) + 1u : 0u;  // n / nF = umulhi(n, mF)
        for (int t0 = tid; t0 < total; t0 += 256 * 8) {
            u32x2 v[8];
            int dstOff[8];
#pragma unroll
            for (int b = 0; b < 8; ++b) {
                const int tt = t0 + 256 * b;
                const bool valid = tt < total;
                const int rr = valid ? (nF > 1 ? static_cast<int>(__umulhi(static_cast<uint32_t>(tt), mF)) : tt) : 0;
                const int kk = valid ? kLo + tt - rr * nF : 0;
                const int o = static_cast<int>(__umul24(rmin + rr - srcRow0, srcSt)) + srcMis + gb0 + 8 * kk;
                if (srcA4) {
                    v[b] = __builtin_amdgcn_raw_buffer_load_b64(srcR, valid ? o : kOobOffset, 0, 0);
                } else {
                    const int d = o & 3;
                    const u32x3 w = __builtin_amdgcn_raw_buffer_load_b96(srcR, valid ? o - d : kOobOffset, 0, 0);
                    v[b] = u32x2{__builtin_amdgcn_alignbyte(w.y, w.x, d), __builtin_amdgcn_alignbyte(w.z, w.y, d)};
                }
                dstOff[b] = valid ? rr * spitch + 8 * kk : -1;
            }
#pragma unroll
            for (int b = 0; b < 8; ++b)
                if (dstOff[b] >= 0)
                    *reinterpret_cast<u32x2 *>(srcL + dstOff[b]) = v[b];
        }
        const int nEdge = nK - nF;
        for (int tt = tid; tt < nR * nEdge; tt += 256) {
            const int rr = tt / nEdge, e = tt - rr * nEdge;
            const int kk = e < kLo ? e : kHi + (e - kLo);
            const int o = static_cast<int>(__umul24(rmin + rr - srcRow0, srcSt)) + srcMis;
            uint32_t w0 = 0, w1 = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const int sb = 8 * kk + i;  // staged byte: pixel lo8 + sb / C, channel sb % C
                const int px = min(max(sp.x + sb / C, 0), srcW - 1);
                const uint32_t bt = __builtin_amdgcn_raw_buffer_load_b8(srcR, o + px * C + sb % C, 0, 0);
                if (i < 4)
                    w0 |= bt << (8 * i);
                else
                    w1 |= bt << (8 * (i - 4));
            }
            *reinterpret_cast<u32x2 *>(srcL + rr * spitch + 8 * kk) = u32x2{w0, w1};
        }
    }
    // row records, tap records, border divisors
    for (int i = tid; i < nRows; i += 256)
        recs[i] = t.rows[y0 + i];
    for (int i = tid; i < nRows * t.nYp; i += 256) {
        const uint2 rt = t.rowTap[static_cast<int64_t>(y0) * t.nYp + i];  // (coefficient, clamped row)
        taps[i] = make_uint2(rt.x, static_cast<uint32_t>((static_cast<int>(rt.y) - rmin) * spitch));
    }
    const bool borderTile = LZ && sp.z;
    if (borderTile)
        for (int i = tid; i < t.CT; i += 256)
            DL[i] = tileX * t.CT + i < t.dstW ? t.cols[tileX * t.CT + i].y : 0;

    // horizontal ownership: 4 adjacent output pixels per thread, rows jStart, jStart + jStep, ...
    const int nQ = t.CT >> 2;
    const int q = tid & (nQ - 1), jStart = tid >> t.log2nQ, jStep = 256 >> t.log2nQ;
    const int x0 = tileX * t.CT + 4 * q;
    uint32_t cf[4][NP];
    int woff[4];
    const int Q = x0 >> 2;  // coalesced: lane-consecutive quads
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        // (pixels past the row's end keep zero coefficients; their window is the segment's start)
        woff[k] = x0 + k < t.dstW ? (t.colA[k * t.nQp + Q] - sp.x) >> 1 : 0;
#pragma unroll
        for (int p = 0; p < NP; ++p)
            cf[k][p] = t.colCoef[(p * 4 + k) * t.nQp + Q];
    }
    lds_barrier();

    // 1. vertical pass: tasks (row j, group g of 8 pixels), g fastest
    {
        const int nG = sp.y;
        const int dj = 256 / nG, dg = 256 - dj * nG;
        int j = tid / nG, g = tid - (tid / nG) * nG;
        while (j < nRows) {
            const uint8_t *colL = srcL + g * (8 * C);
            const uint2 *tj = taps + j * t.nYp;
            uint32_t acc[C][4];
#pragma unroll
            for (int c = 0; c < C; ++c)
#pragma unroll
                for (int m = 0; m < 4; ++m)
                    acc[c][m] = 0;
            for (int i = 0; i < t.nYp; i += 2) {
                const uint4 c2 = *reinterpret_cast<const uint4 *>(tj + i);  // (coef, offset) x 2
                uint32_t d0[2 * C], d1[2 * C];
#pragma unroll
                for (int u = 0; u < C; ++u) {
                    const u32x2 v0 = *reinterpret_cast<const u32x2 *>(colL + c2.y + 8 * u);
                    const u32x2 v1 = *reinterpret_cast<const u32x2 *>(colL + c2.w + 8 * u);
                    d0[2 * u] = v0.x;
                    d0[2 * u + 1] = v0.y;
                    d1[2 * u] = v1.x;
                    d1[2 * u + 1] = v1.y;
                }
                // tap-outer, pair-inner: 4 C independent v_pk_mad_u16 chains per tap
#pragma unroll
                for (int h = 0; h < 2; ++h)
#pragma unroll
                    for (int c = 0; c < C; ++c)
#pragma unroll
                        for (int m = 0; m < 4; ++m) {
                            constexpr int last = 2 * C - 1;
                            const int k = (2 * m * C + c) >> 2, k1 = k < last ? k + 1 : last;
                            const uint32_t sel = pair_sel<C>(m, c);
                            acc[c][m] = h == 0 ? pk_mad(__builtin_amdgcn_perm(d0[k1], d0[k], sel), c2.x, acc[c][m])
                                               : pk_mad(__builtin_amdgcn_perm(d1[k1], d1[k], sel), c2.z, acc[c][m]);
                        }
            }
            const int4 r = recs[j];
            if (LZ && r.w != 0) {  // masked + renormalised border row: int16(nume * 64 / deno)
                auto dv = [&](uint32_t pr) {
                    const int lo = exact_div(static_cast<int>(static_cast<int16_t>(pr & 0xffffu)) * 64, r.w);
                    const int hi = exact_div(static_cast<int>(static_cast<int16_t>(pr >> 16)) * 64, r.w);
                    return (static_cast<uint32_t>(lo) & 0xffffu) | (static_cast<uint32_t>(hi) << 16);
                };
#pragma unroll
                for (int c = 0; c < C; ++c)
#pragma unroll
                    for (int m = 0; m < 4; ++m)
                        acc[c][m] = dv(acc[c][m]);
            }
#pragma unroll
            for (int c = 0; c < C; ++c)
                *reinterpret_cast<uint4 *>(work + (j * C + c) * t.pitchDw + 4 * g) =
                    make_uint4(acc[c][0], acc[c][1], acc[c][2], acc[c][3]);
            j += dj;
            g += dg;
            if (g >= nG) {
                g -= nG;
                ++j;
            }
        }
    }
    lds_barrier();

    // 2. horizontal pass
    const int dstSt = static_cast<int>(a.io.dstSt);
    for (int j = jStart; j < nRows; j += jStep) {
        uint32_t bt[4 * C];  // the 4 * C output bytes: pixel k's channel c is byte k * C + c
#pragma unroll
        for (int c = 0; c < C; ++c) {
            const uint32_t *w = work + (j * C + c) * t.pitchDw;
#pragma unroll
            for (int k = 0; k < 4; ++k) {
                int s = LZ ? (1 << 19) : (1 << 22);
#pragma unroll
                for (int p = 0; p < NP; ++p)
                    s = LZ ? sdot2(w[woff[k] + p], cf[k][p], s)
                           : static_cast<int>(udot2(w[woff[k] + p], cf[k][p], static_cast<uint32_t>(s)));
                uint32_t &ob = bt[k * C + c];
                if (LZ) {
                    int v = s >> 20;  // within int16: the reference's int16 cast is the identity here
                    if (borderTile) {
                        const int Dk = DL[4 * q + k];
                        if (Dk != 0)
                            v = static_cast<int16_t>(exact_div(s, Dk));
                    }
                    ob = static_cast<uint32_t>(min(max(v, 0), 255));
                } else {
                    ob = min((static_cast<uint32_t>(s) >> 23) & 0xffffu, 255u);
                }
            }
        }
        if constexpr (NORM) {
            // float epilogue: per output plane the 4 bytes of channel order[p] (uniform selects),
            // the affine map, one vector store (single elements at the row's right end, or where the
            // frame, row or plane start is not 4-byte aligned: 2-byte elements only)
            const NormDev &n = a.n;
            const bool full = x0 + 4 <= t.dstW;
            const bool vec = full && dstA4 && !(n.planeSt & 3);
            const int rowOff = (y0 + j - a.io.dstRow0) * dstSt;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= n.planes)
                    break;
                const int oc = n.order[p];
                float f[4];
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    uint32_t v = bt[k * C];
#pragma unroll
                    for (int c = 1; c < C; ++c)
                        v = oc == c ? bt[k * C + c] : v;
                    f[k] = norm_affine(v, n.scale[p], n.bias[p]);
                }
                if (n.dtype == 1) {
                    const int off = p * n.planeSt + rowOff + x0 * 4;
                    if (vec) {
                        __builtin_amdgcn_raw_buffer_store_b128(
                            u32x4{__float_as_uint(f[0]), __float_as_uint(f[1]), __float_as_uint(f[2]),
                                  __float_as_uint(f[3])},
                            dstR, off, 0, 0);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (x0 + k < t.dstW)
                                __builtin_amdgcn_raw_buffer_store_b32(__float_as_uint(f[k]), dstR, off + 4 * k, 0, 0);
                    }
                } else {
                    uint32_t h[4];
                    if (n.dtype == 2) {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            h[k] = f16_bits(f[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            h[k] = bf16_bits(f[k]);
                    }
                    const int off = p * n.planeSt + rowOff + x0 * 2;
                    if (vec) {
                        __builtin_amdgcn_raw_buffer_store_b64(u32x2{h[0] | (h[1] << 16), h[2] | (h[3] << 16)}, dstR, off,
                                                              0, 0);
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (x0 + k < t.dstW)
                                __builtin_amdgcn_raw_buffer_store_b16(static_cast<uint16_t>(h[k]), dstR, off + 2 * k, 0,
                                                                      0);
                    }
                }
            }
            continue;
        }
        // packed after every LDS read of the row is issued (opaque() is a volatile asm, which the
        // reads do not move across), one per dword as in tile_kernel: it keeps the combiner from
        // packing two clamps with v_ashr_pk_u8_i32 and OR-ing into its undefined half (kernels_dev.hpp)
        uint32_t o[C];
#pragma unroll
        for (int d = 0; d < C; ++d)
            o[d] = opaque(bt[4 * d] | (bt[4 * d + 1] << 8)) | (bt[4 * d + 2] << 16) | (bt[4 * d + 3] << 24);
        const int off = (y0 + j - a.io.dstRow0) * dstSt + x0 * C;
        if (dstA4 && x0 + 4 <= t.dstW) {
            if constexpr (C == 2)
                __builtin_amdgcn_raw_buffer_store_b64(u32x2{o[0], o[1]}, dstR, off, 0, 0);
            else if constexpr (C == 3)
                __builtin_amdgcn_raw_buffer_store_b96(u32x3{o[0], o[1], o[2]}, dstR, off, 0, 0);
            else
                __builtin_amdgcn_raw_buffer_store_b128(u32x4{o[0], o[1], o[2], o[3]}, dstR, off, 0, 0);
        } else {
#pragma unroll
            for (int b = 0; b < 4 * C; ++b)
                if (x0 + b / C < t.dstW)
                    __builtin_amdgcn_raw_buffer_store_b8(static_cast<uint8_t>(o[b >> 2] >> (8 * (b & 3))), dstR,
                                                         off + b, 0, 0);
        }
    }
}

template <int C, bool LZ, bool NORM>
const void *packed_tile_np(int NP)
{
#define IQO_PTILE(NP_)                                                                               \
    case NP_:                                                                                        \
        return reinterpret_cast<const void *>(packed_tile_kernel<C, NP_, LZ, NORM>);
    switch (NP) {
        IQO_PTILE(1)
        IQO_PTILE(2)
        IQO_PTILE(3)
        IQO_PTILE(4)
        IQO_PTILE(5)
        IQO_PTILE(6)
        IQO_PTILE(7)
        IQO_PTILE(8)
        IQO_PTILE(10)
        IQO_PTILE(12)
        IQO_PTILE(16)
    default:
        return nullptr;
    }
#undef IQO_PTILE
}

template <int C, bool NORM>
const void *packed_tile_fn(bool lanczos, int NP)
{
    return lanczos ? packed_tile_np<C, true, NORM>(NP) : packed_tile_np<C, false, NORM>(NP);
}

template <bool NORM>
const void *packed_tile_any(int channels, bool lanczos, int NP)
{
    return channels == 2 ? packed_tile_fn<2, NORM>(lanczos, NP)
                         : channels == 3 ? packed_tile_fn<3, NORM>(lanczos, NP) : packed_tile_fn<4, NORM>(lanczos, NP);
}

bool norm_ok(const NormDev &n, int channels)
{
    if (n.dtype < 1 || n.dtype > 3 || n.planes < 1 || n.planes > 4 || n.planeSt < 0)
        return false;
    for (int p = 0; p < n.planes; ++p)
        if (n.order[p] < 0 || n.order[p] >= channels)
            return false;
    return true;
}

} // namespace

// ================================================================ launchers

hipError_t launch_packed_general(const GeneralDev &g, int channels, const Io &io, int rowBegin, int rowEnd,
                                 hipStream_t s, LaunchGrid *query)
{
    if (channels < 2 || channels > 4)
        return hipErrorInvalidValue;
    if (rowEnd <= rowBegin || io.frames <= 0)
        return hipSuccess;
    PackedGeneralArgs a{g, io, rowBegin, channels};
    dim3 grid(static_cast<unsigned>(rowEnd - rowBegin), static_cast<unsigned>(io.frames), static_cast<unsigned>(channels));
    if (query) {
        *query = plain_grid(kFamPackedGeneral, grid, 256, 0, 0);
        return hipSuccess;
    }
    size_t lds = static_cast<size_t>(g.ldsInts) * sizeof(int);
    hipLaunchKernelGGL(packed_general_kernel, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

hipError_t launch_packed_general_norm(const GeneralDev &g, int channels, const Io &io, const NormDev &n, int rowBegin,
                                      int rowEnd, hipStream_t s, LaunchGrid *query)
{
    if (channels < 2 || channels > 4 || !norm_ok(n, channels))
        return hipErrorInvalidValue;
    if (rowEnd <= rowBegin || io.frames <= 0)
        return hipSuccess;
    PackedGeneralNormArgs a;
    static_cast<PackedGeneralArgs &>(a) = PackedGeneralArgs{g, io, rowBegin, channels};
    a.n = n;
    dim3 grid(static_cast<unsigned>(rowEnd - rowBegin), static_cast<unsigned>(io.frames), static_cast<unsigned>(n.planes));
    if (query) {
        *query = plain_grid(kFamPackedGeneral, grid, 256, 0, 0);
        return hipSuccess;
    }
    size_t lds = static_cast<size_t>(g.ldsInts) * sizeof(int);
    hipLaunchKernelGGL(packed_general_norm_kernel, grid, dim3(256), lds, s, a);
    return hipGetLastError();
}

namespace {

// norm == nullptr: the U8 kernel; else its NORM instantiation on the float frame io.dst
hipError_t launch_ptile(const TileDev &t, int channels, const Io &io, const NormDev *norm, int rowBegin, int rowEnd,
                        hipStream_t s, LaunchGrid *query)
{
    if (channels < 2 || channels > 4 || (norm && !norm_ok(*norm, channels)))
        return hipErrorInvalidValue;
    if (rowEnd <= rowBegin || io.frames <= 0)
        return hipSuccess;
    const int rows = rowEnd - rowBegin;
    // stores are relative to dstRow0; a float frame: the last plane's last row
    const int64_t rowB = norm ? static_cast<int64_t>(t.dstW) * (norm->dtype == 1 ? 4 : 2) : static_cast<int64_t>(t.dstW) * channels;
    int64_t sb, db;
    if (!layout_ok(kFamPackedTile, io, rowEnd, static_cast<int64_t>(t.srcW) * channels,
                   rowB + (norm ? static_cast<int64_t>(norm->planes - 1) * norm->planeSt : 0), &sb, &db) ||
        t.srcH >= (1 << 24))
        return hipErrorInvalidValue;
    const int nTx = (t.dstW + t.CT - 1) / t.CT, nTy = (rows + t.TH - 1) / t.TH;
    const uint64_t nTiles = static_cast<uint64_t>(nTx) * static_cast<uint64_t>(nTy) * static_cast<uint64_t>(io.frames);
    if (nTiles >= (uint64_t(1) << 31))
        return hipErrorInvalidValue;
    PackedTileArgs a{t, io, rowBegin, rowEnd, static_cast<int>(sb), static_cast<int>(db), nTx, nTy,
                     static_cast<unsigned>(nTiles)};
    // plan.cpp packed_lds_bytes
    const size_t lds = static_cast<size_t>(t.TH) * (static_cast<size_t>(channels) * t.pitchDw * 4 + 16 +
                                                    static_cast<size_t>(t.nYp) * 8) +
                       4u * static_cast<size_t>(t.CT) + static_cast<size_t>(t.srcRows) * t.spitch;
    if (lds > 64 * 1024)
        return hipErrorInvalidValue;
    const void *kern = norm ? packed_tile_any<true>(channels, t.lanczos, t.NP) : packed_tile_any<false>(channels, t.lanczos, t.NP);
    if (!kern)
        return hipErrorInvalidValue;
    if (query) {
        *query = block_grid(kFamPackedTile, kMapChunks, static_cast<unsigned>(nTx * nTy), static_cast<unsigned>(nTiles), 256, nTy);
        return hipSuccess;
    }
    PackedTileNormArgs an;
    void *args[] = {&a};
    if (norm) {
        static_cast<PackedTileArgs &>(an) = a;
        an.n = *norm;
        args[0] = &an;
    }
    return hipLaunchKernel(kern, dim3(static_cast<unsigned>(nTiles)), dim3(256), args, lds, s);
}

} // namespace

hipError_t launch_packed_tile(const TileDev &t, int channels, const Io &io, int rowBegin, int rowEnd, hipStream_t s,
                              LaunchGrid *query)
{
    return launch_ptile(t, channels, io, nullptr, rowBegin, rowEnd, s, query);
}

hipError_t launch_packed_tile_norm(const TileDev &t, int channels, const Io &io, const NormDev &n, int rowBegin,
                                   int rowEnd, hipStream_t s, LaunchGrid *query)
{
    return launch_ptile(t, channels, io, &n, rowBegin, rowEnd, s, query);
}

} // namespace iqo_amd
