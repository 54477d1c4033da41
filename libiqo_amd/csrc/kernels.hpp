// kernels.hpp -- launch interface of the gfx950 resize kernels (kernels.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "colorspace.hpp"

namespace iqo_amd {

// A device-side view of one batched call: frame f reads src + f*srcFrameSt, whose row 0 is
// GLOBAL source row srcRow0, and writes dst + f*dstFrameSt, whose row 0 is global row dstRow0.
struct Io {
    const uint8_t *src;
    int64_t srcSt, srcFrameSt;
    int srcRow0;
    int srcRowEnd;  // one past the last global source row the call may read (end of the window)
    uint8_t *dst;
    int64_t dstSt, dstFrameSt;
    int dstRow0;
    int frames;
};

// --- the template instantiation a launch runs, by name.  Every family with more than one
// instantiation keeps ONE table of them (kernels.hip: tile, walk; kernels_ratio.hip: the ratio
// kernels) and one lookup over it, `<family>_instance(dev)`: the launch function runs the entry the
// lookup returns, and the C ABI reports that entry (iqo_hip.h iqo_hip_instance) -- a pure host
// function of the *Dev, no device query and no launch.  Parameters a family does not have are 0.
constexpr int kFamTile = 4, kFamWalk = 5, kFamUp2 = 6, kFamD32 = 7, kFamA32 = 8, kFamU23 = 9, kFamL23 = 10,
              kFamD31 = 11, kFamRyx = 12, kFamRyg = 13;  // iqo_hip.h IQO_KERNEL_* (abi.hip asserts it)
constexpr int kFamGeneral = 0, kFamLanczosStream = 1, kFamAreaInt = 2, kFamLinearUp2 = 3, kFamPackedTile = 14,
              kFamPackedGeneral = 15, kFamCount = 16;
constexpr int kSubRyu = 1;       // Instance::sub within kFamRyg: ryu_kernel (0: ryg_kernel)

// --- address-range limits: the ONE table of what layouts each family's launcher accepts.
// The buffer-addressed kernels drop an access (a store of a lane that produces nothing, a load of an
// off-image block that must read 0) by giving it the byte offset kOobOffset, which the hardware's range
// check refuses as long as the buffer range -- the span below -- does not reach it.  Twice the sentinel
// plus the largest row offset still fits 32 bits, so `sentinel + row offset` never wraps into the range.
constexpr int kOobOffset = 0x7ff00000;
// Largest accepted value of each quantity, 0: unlimited (the family addresses through 64-bit pointers).
// Span: bytes from the first byte of the source window / destination band to the last byte touched,
// (rows - 1) * stride + row bytes, the launchers' sb / db and the kernels' buffer range.
struct LayoutLimits {
    int64_t srcSpanMax, dstSpanMax, srcStMax, dstStMax;
};
constexpr LayoutLimits layout_limits(int family)
{
    constexpr int64_t kSentinel = kOobOffset - 1;          // a span the sentinel stays outside of
    constexpr int64_t kInt = (int64_t(1) << 31) - 1;       // 32-bit signed row offsets
    constexpr int64_t kMul24 = (int64_t(1) << 24) - 1;     // row * stride by a 24-bit multiply
    switch (family) {
    case kFamGeneral:
    case kFamAreaInt:        // (with linear_d2)
    case kFamPackedGeneral:
        return {0, 0, 0, 0};
    case kFamTile:           // the sentinel only on loads whose value is discarded
    case kFamPackedTile:
        return {kInt, kInt, kMul24, kInt};
    case kFamLanczosStream:  // every streamer body and lanczos_stack: dropped stores, zero-reading loads
    case kFamLinearUp2:
        return {kSentinel, kSentinel, kSentinel, kSentinel};
    case kFamWalk:
        return {kSentinel, kSentinel, kMul24, kSentinel};
    default:                 // the exact-ratio and ratio-row kernels (kernels_ratio.hip)
        return {kSentinel, kSentinel, kMul24, kMul24};
    }
}
// The check every launcher makes (and the C ABI, before a call's first launch): the spans of output rows
// [.., rowEnd) of `io`, whose rows hold srcRowBytes / dstRowBytes bytes, against the family's limits.
// The walker's source range ends at the dword that holds the window's last pixel.  *sb / *db: the spans.
inline bool layout_ok(int family, const Io &io, int rowEnd, int64_t srcRowBytes, int64_t dstRowBytes, int64_t *sb,
                      int64_t *db)
{
    const LayoutLimits m = layout_limits(family);
    if (family == kFamWalk)
        srcRowBytes = (srcRowBytes + 3) & ~int64_t(3);
    if ((m.srcStMax && (io.srcSt < 0 || io.srcSt > m.srcStMax)) || (m.dstStMax && (io.dstSt < 0 || io.dstSt > m.dstStMax)))
        return false;
    // (strides of a limited family are below 2^31 here, so the products cannot wrap)
    *sb = m.srcSpanMax ? static_cast<int64_t>(io.srcRowEnd - io.srcRow0 - 1) * io.srcSt + srcRowBytes : 0;
    *db = m.dstSpanMax ? static_cast<int64_t>(rowEnd - 1 - io.dstRow0) * io.dstSt + dstRowBytes : 0;  // stores are relative to dstRow0
    return *sb <= m.srcSpanMax && *db <= m.dstSpanMax;
}
// --- the grid of one launch, by number (iqo_hip.h iqo_hip_launch_grid).  Every launcher below takes a
// trailing `LaunchGrid *query`: non-null, it runs the arithmetic it launches with -- instantiation, lanes,
// bands, units, grid -- fills *query and launches nothing, so the report cannot drift from the launch.
// A "unit" is what the kernel decodes (column, band, frame) from: a wave (walker, exact-ratio kernels), a
// tile (tile, packed tile) or a workgroup (ryx / ryg / ryu, the block-shared and stacked streamers).
constexpr int kMapNone = 0, kMapSpread = 1, kMapChunks = 2, kMapXcdTail = 3;  // iqo_hip.h IQO_GRID_MAP_*
struct LaunchGrid {
    int family = 0;
    int map = kMapNone;          // how a flat block id becomes a logical one (kernels_dev.hpp xcd_*)
    unsigned gridX = 0, gridY = 1, gridZ = 1, block = 0;
    unsigned blocks = 0;         // n of the map: the flat ids it permutes (map none: gridX)
    unsigned chunk = 0;          // C of xcd_chunks (0: the map has none)
    unsigned unitsPerFrame = 0, unitsPerBlock = 0;
    unsigned units = 0;          // the kernel's nWaves / nTiles / nBlocks argument
    int bands = 0, wavesPerRow = 0;  // 0: the family has none
    unsigned framesPerBlock = 1; // stacked streamer: frames side by side in one workgroup
    int tailBands = 0;           // kMapXcdTail: bands of each XCD's last frame (the others: `bands`)
};
// Blocks of a grid-stride launch of the second-pass kernels (kernels_color.hip, kernels_norm.hip): a launch
// of more than kGridStrideBlocks * 256 items strides over the rest (iqo_hip.h IQO_HIP_GRID_STRIDE_BLOCKS).
constexpr unsigned kGridStrideBlocks = 2048;

struct Instance {
    int family, sub;
    int LZ, P, Q, T, NP, PD, ADJ, CPT, UC, NL, RUN, KM, VY, NV, NT, F, VARIANT;
    const void *kern;
};
struct InstanceList {
    const Instance *first;
    int count;
};
// Every instantiation of a family, in table order (ryg: ryg_kernel's, then ryu_kernel's); {nullptr, 0}
// for a family with a single kernel.
InstanceList instances(int family);
InstanceList tile_walk_instances(int family);  // (its tile / walk part, kernels.hip; the rest and the whole: kernels_ratio.hip)

// --- general kernel: one workgroup per output row; LDS work row built chunk by chunk.
struct GeneralDev {
    int method, srcW, srcH, dstW, nX, nY;
    const int4 *xInfo, *yInfo;   // {srcO, tabOff, kind, aux} per dst column / row
    const int *tabX, *tabY;      // quantised tables (int16 / u16 values widened)
    const int4 *chunks;          // {xs, xe, lo, hi}
    int nChunks;
    int ldsInts;                 // work-row capacity (ints) of the largest chunk
};
hipError_t launch_general(const GeneralDev &g, const Io &io, int rowBegin, int rowEnd, hipStream_t s, LaunchGrid *query = nullptr);
// --- separable tile kernel (general ratios): tables from plan.cpp build_tile_tables.
struct TileDev {
    bool lanczos;                // int16 work + signed dots (else u16 work, Area / Linear)
    int srcW, srcH, dstW;
    int NP, nYp, CT, TH, pitchDw, log2nQ;
    int srcRows, spitch;         // staged source tile: rows (max over any TH output rows), pitch
    const int4 *rows;            // TileRec {start, lo, hi, deno} per output row
    const uint2 *rowTap;         // dstH x nYp {(c, c) splat, clamped source row}
    const int2 *cols;            // TileCol {a, D} per output column
    const uint32_t *colCoef;     // [NP][4][nQp] pairs (pair, column in quad, quad)
    const int *colA;             // [4][nQp] even window starts
    int nQp;                     // quads of the padded tile width
    const int4 *spans;           // {lo8, groups, any border column, 0} per column tile
};
hipError_t launch_tile(const TileDev &t, const Io &io, int rowBegin, int rowEnd, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *tile_instance(const TileDev &t);      // null: no instantiation (launch_tile rejects it)


// --- packed (interleaved) pixels, C = 2 .. 4 bytes per pixel, every channel resized on its own
// (kernels_packed.hip).  Widths in GeneralDev / TileDev stay in PIXELS; Io strides are bytes.
// packed_general_kernel: general_kernel per channel.
hipError_t launch_packed_general(const GeneralDev &g, int channels, const Io &io, int rowBegin, int rowEnd,
                                 hipStream_t s, LaunchGrid *query = nullptr);
// packed_tile_kernel: the planar tile tables (rows, rowTap, cols, colCoef, colA, nQp) with the
// packed tiling of plan.hpp PackedTables in CT, TH, pitchDw (one channel segment), log2nQ, srcRows,
// spitch and spans ({lo8 pixel, 8-pixel groups, any border column, 0} per column tile).
hipError_t launch_packed_tile(const TileDev &t, int channels, const Io &io, int rowBegin, int rowEnd,
                              hipStream_t s, LaunchGrid *query = nullptr);

// --- normalised planar float output of the two packed kernels (their NORM instantiations): plane p
// of the output is cvt(fl32(fl32((float)u8(order[p]) * scale[p]) + bias[p])) of the byte the U8 path
// would store, two separately rounded fp32 operations.  Io::dst is the float buffer, Io::dstSt its
// row stride and Io::dstFrameSt its frame stride, in bytes; plane p starts planeSt * p bytes into the
// frame.  Every stride and the base are multiples of the element size (checked by the caller).
struct NormDev {
    int dtype;                   // 1 fp32, 2 fp16, 3 bf16 (iqo_hip.h IQO_OUT_*)
    int planes;                  // 1 .. 4
    int planeSt;                 // bytes, < 2^31
    int order[4];                // source channel of plane p
    float scale[4], bias[4];
};
hipError_t launch_packed_general_norm(const GeneralDev &g, int channels, const Io &io, const NormDev &n, int rowBegin,
                                      int rowEnd, hipStream_t s, LaunchGrid *query = nullptr);
hipError_t launch_packed_tile_norm(const TileDev &t, int channels, const Io &io, const NormDev &n, int rowBegin,
                                   int rowEnd, hipStream_t s, LaunchGrid *query = nullptr);

// --- batched crop-and-resize (kernels_roi.hip roi_kernel): one launch over the workgroups of a call's
// arena (roi.hpp), which lies in device memory at `arena` and names every box, its tables and its
// workgroups.  dst: interleaved bytes, rows dstSt and outputs dstRoiSt bytes apart; with `norm` the float
// planes of NormDev (rows dstSt, planes norm->planeSt, outputs dstRoiSt bytes apart).
struct RoiDev {
    const uint32_t *arena;
    const uint8_t *src;
    uint8_t *dst;
    int64_t srcSt, dstSt, dstRoiSt;
    bool lanczos;
    int channels;                // 1, 3 or 4
    unsigned groups;             // the arena's workgroup count
    size_t ldsBytes;             // the largest workgroup's LDS (roi.hpp RoiLayout)
    bool fit = false;            // the arena is the fit format (roi_fit_kernel), and
    uint8_t pad[4] = {0, 0, 0, 0};  // the pad colour: byte c of a pixel
};
hipError_t launch_roi(const RoiDev &d, const NormDev *norm, hipStream_t s);

// --- boxes of NV12 / I420 frames straight to RGB (kernels_roi_yuv.hip roi_yuv_kernel): as launch_roi over
// the YUV arena of roi.hpp, which also carries the layout and the planes' row strides.  y, u, v: frame 0's
// planes (interleaved UV: u, and v is not read).  dst: packed bytes, `channels` 3 or 4 per pixel, byte c =
// order[c] of {0 R, 1 G, 2 B, 3 the constant 255}; with `norm` the float planes of NormDev of (R, G, B).
struct RoiYuvDev {
    const uint32_t *arena;
    const uint8_t *y, *u, *v;
    uint8_t *dst;
    int64_t dstSt, dstRoiSt;
    bool lanczos, interleavedUV;
    YuvRgbCoef k;                // the standard's six integers
    int channels, order[4];
    unsigned groups;
    size_t ldsBytes;
    bool fit = false;            // the arena is the fit format (roi_yuv_fit_kernel), and
    uint8_t pad[4] = {0, 0, 0, 0};  // the pad colour: R, G, B
};
hipError_t launch_roi_yuv(const RoiYuvDev &d, const NormDev *norm, hipStream_t s);

// --- YUV 4:2:0 planes -> RGB (kernels_color.hip): the second pass of the NV12 / I420 "resize to RGB"
// entries.  Reads resized planes from a workspace (Y dstW x dstH; chroma cw x ch, replicated to the
// output grid: pixel (y, x) takes sample (min(y >> 1, ch - 1), min(x >> 1, cw - 1))), applies the
// integer matrix of colorspace.hpp and writes packed bytes or NormDev's planar floats.
// Workspace rows: the Y base and ySt are multiples of 8 with ySt >= 8 ceil(dstW / 8); the chroma
// bases and cSt are multiples of 8 (interleaved UV) / 4 (separate U, V) with
// cSt >= 8 / 4 ceil(dstW / 8) -- a thread loads 8 Y bytes and 4 chroma pairs whole; what it loads
// past the planes' widths is never used.  No alignment of dst beyond the element size.
// chroma444 (IQO_CHROMA_FULL): the chroma planes are on the output grid, cw x ch = dstW x dstH, and
// pixel (y, x) takes sample (y, x).  A thread then loads 8 chroma pairs whole: the chroma bases and cSt
// are multiples of 16 (interleaved UV; frameSt too) / 8 (separate U, V) with cSt >= 16 / 8 ceil(dstW / 8).
struct YuvRgbDev {
    int dstW, dstH, cw, ch;
    YuvRgbCoef k;                      // the standard's six integers
    const uint8_t *y, *u, *v;          // frame 0's planes; interleaved UV: u, and v is not read
    int ySt, cSt;                      // row strides, bytes
    int64_t frameSt;                   // workspace frame stride, bytes
    uint8_t *dst;
    int dstSt;                         // row stride, bytes (< 2^31; one frame's extent < 2^31)
    int64_t dstFrameSt;
    int frames;                        // frames x dstH x ceil(dstW / 4) < 2^31
};
// Packed bytes: `channels` 3 or 4 per pixel, byte c = order[c] of {0 R, 1 G, 2 B, 3 the constant 255}.
hipError_t launch_yuv_rgb_bytes(const YuvRgbDev &d, bool interleavedUV, bool chroma444, int channels,
                                const int (&order)[4], hipStream_t s);
// Planar floats as the packed kernels' NORM epilogue, of the 3-channel source (R, G, B).
hipError_t launch_yuv_rgb_norm(const YuvRgbDev &d, bool interleavedUV, bool chroma444, const NormDev &n, hipStream_t s);

// --- packed RGB(A) -> YUV 4:2:0 planes (kernels_color.hip): the second pass of the "resize to NV12 /
// I420" entries.  Reads resized packed pixels (C = 3 or 4 bytes each, dstW x dstH) from a workspace,
// applies the forward integer matrix of colorspace.hpp -- Y per pixel, U and V once per 2 x 2 block on the
// block's sums, cw x ch = dstW/2 x dstH/2 samples -- and writes a Y plane and an interleaved UV plane
// (NV12) or U and V planes (I420).  An odd dstW's last column and an odd dstH's last row give Y only.
// Workspace rows: base, srcSt and srcFrameSt are multiples of 16 with srcSt >= 8 C ceil(dstW / 8) -- a
// thread loads its 8 pixels of two rows whole; the pad pixels past dstW are never stored.  No alignment of
// the destinations beyond a byte.
struct RgbYuvDev {
    int dstW, dstH;
    RgbYuvCoef k;                      // the standard's ten integers
    int order[3];                      // the byte of a source pixel that holds R, G, B (distinct, < C)
    const uint8_t *src;                // frame 0 of the workspace
    int srcSt;                         // row stride, bytes (one frame < 2^31)
    int64_t srcFrameSt;
    uint8_t *y, *u, *v;                // frame 0's planes; interleaved UV: u, and v is not written
    int ySt, cSt;                      // row strides, bytes (each plane of one frame < 2^31)
    int64_t dstFrameSt;
    int frames;                        // frames x ceil(dstH / 2) x ceil(dstW / 8) < 2^31
};
hipError_t launch_rgb_yuv(const RgbYuvDev &d, int channels, bool interleavedUV, hipStream_t s);

// --- resized U8 planes -> normalised planar floats (kernels_norm.hip): the second pass of
// iqo_hip_resize_planes_norm_device.  Reads up to 4 resized planes (dstW x dstH each) per frame from a
// workspace and writes NormDev's planar floats, NormDev::order[p] being the workspace plane of output
// plane p: out = cvt(fl32(fl32((float)u8 * scale[p]) + bias[p])).
// Workspace: src, srcSt, srcPlaneSt and srcFrameSt are multiples of 8 with srcSt >= 8 ceil(dstW / 8) --
// a thread loads its 8 (fp32: 4) bytes of a plane whole; what it loads past dstW is never used.  No
// alignment of dst beyond the element size.
struct PlanesNormDev {
    int dstW, dstH;
    const uint8_t *src;                // plane 0 of frame 0 of the workspace
    int srcSt;                         // row stride, bytes
    int64_t srcPlaneSt, srcFrameSt;
    uint8_t *dst;
    int dstSt;                         // row stride, bytes (< 2^31; one frame's extent < 2^31)
    int64_t dstFrameSt;
    int frames;                        // frames x dstH x ceil(dstW / 4) < 2^31
};
hipError_t launch_planes_norm(const PlanesNormDev &d, const NormDev &n, hipStream_t s);

// --- general-ratio wave walker: every wave walks a 256-column strip of one band of rows through
// a private LDS ring of source rows widened to u16 (plan.hpp WalkTables; 4-byte aligned sources).
struct WalkDev {
    TileDev t;                   // column tables (cols, colCoef, colA, nQp), lanczos, srcW / dstW, NP
    int nS;                      // 256-output strips per row
    const int4 *spans;           // {lo8, units, interior, 0} per strip; a unit = 4 work columns
    int NV;                      // units per lane (1, 2)
    int R, pitch;                // ring rows, ring row pitch (bytes)
    int waveBytes;               // LDS per wave: ring + work row + sink
    const uint32_t *rowTap;      // (dstH + 1) x VY x {(c, c) splat, ring byte offset of the clamped row}
    const int4 *rows;            // {lo, hi, hi % R, deno} per output row
    const int4 *segs;            // 2 per row: {first, ring offset of first, border, first of row
                                 // + kWalkD}, {yM, yS, yNeg, 0} (plan.hpp WalkSeg; padded past the end)
};
// strips stripLo + i * stripStride (i < strips; strips < 0: all of them)
hipError_t launch_walk(const WalkDev &w, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s,
                       int stripLo = 0, int strips = -1, int stripStride = 1, LaunchGrid *query = nullptr);
const Instance *walk_instance(const WalkDev &w);

// --- exact 2x Lanczos-2/3 upscale, main rows x middle columns (plan.hpp Up2Tables).
struct Up2Dev {
    int srcW, srcH, dstW, dstH;
    int F;                       // factor: 2 or 3 (output y = F k + j takes phase j)
    int NT;                      // taps per axis (4 or 6)
    int np;                      // producing lanes per wave (0 = auto)
    uint32_t cy0;                // phase 0 rows: (c, c) splat of the single tap (the source row itself)
    uint32_t cy1[2][6];          // phase 1 .. F-1 rows: (c, c) splats of the NT taps
    uint32_t cx0;                // phase 0 columns: (c, 0) of the single tap
    uint32_t cx1[2][3];          // phase 1 .. F-1 columns: int16 coefficient pairs of the NT taps
    uint32_t xM[2][24];          // edge-lane exact divisions (left / right 8 F columns)
    int xT[2][24];
    int m0, m1;                  // main rows; the others are masked border rows divided by
    uint32_t yM[2][16];          //   magic_y (top: row y, bottom: row y - m1)
    int yS[2][16];
};
hipError_t launch_up2(const Up2Dev &u, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *up2_instance(const Up2Dev &u);

// Exact 3:2 Lanczos-3 downscale (plan.hpp D32Tables): main rows x all columns.
struct D32Dev {
    int srcW, srcH, dstW, dstH;
    int np;                      // producing lanes per wave (0 = auto)
    int pd;                      // row groups loaded ahead (1, 2, 4; 0 = default 1)
    int variant;                 // tap structure: 0 Lanczos-3 (10 taps), 1 Lanczos-2 (6 taps)
    uint32_t cy[2][8];           // (c, c) u16 splats: phase p's taps at group rows 2p .. 2p + 7
    uint32_t cx[2][5];           // phase p's (c_2q, c_2q+1) int16 pairs
    uint32_t xM[2][8];           // edge-lane exact divisions (left / right 8 columns)
    int xT[2][8];
    int m0, m1;                  // main rows; the others are masked border rows divided by
    uint32_t yM[2][8];           //   magic_y (top: row y, bottom: row y - m1)
    int yS[2][8];
};
hipError_t launch_d32(const D32Dev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *d32_instance(const D32Dev &d);

// Exact 3:1 Lanczos-2/3 downscale (plan.hpp D31Tables): every row and column.
struct D31Dev {
    int srcW, srcH, dstW, dstH;
    int np;                      // producing lanes per wave (0 = auto)
    int pd;                      // output rows loaded ahead (Lanczos-3: 1, 5; Lanczos-2: 1, 2, 4; 0 = 1)
    int variant;                 // tap structure: 0 Lanczos-3 (18 taps), 1 Lanczos-2 (12 taps)
    uint32_t cc, cp[5];          // (c, c) u16 splats: the centre tap, the symmetric pairs' taps
    uint32_t cxe[9], cxo[9];     // (c_2q, c_2q+1) / (c_2q+1, c_2q+2) int16 pairs: even / odd window starts
    uint32_t xM[2][4];           // edge-lane exact divisions (left / right 4 columns)
    int xT[2][4];
    int m0, m1;                  // main rows; the others are masked border rows divided by
    uint32_t yM[2][8];           //   magic_y (top: row y, bottom: row y - m1)
    int yS[2][8];
};
hipError_t launch_d31(const D31Dev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *d31_instance(const D31Dev &d);

// Exact vertical ratio, tabled columns (plan.hpp RyxTables): every row and column.
constexpr int kRyxPadK = 24;     // work-row padding (u16 entries) left of column 0: plan.hpp kRyxPad
struct RyxDev {
    bool lanczos;
    int srcW, srcH, dstW, dstH;
    int P, Q, taps, NP;
    int off;                     // group m's window starts at source row P m + off
    int m0, m1;                  // Lanczos main rows; the others are masked border rows (magic_y)
    uint32_t yM[2][16];
    int yS[2][16];
    const uint32_t *rowCoef;     // Q x taps (c, c) splats
    const int4 *cols;            // per column {work byte offset of the even start, magic, shift, 0}
    const uint32_t *colCoef;     // dstW x NP pairs
    // column split: `parts` workgroups per (band, frame), part k writes output columns
    // [xs[k], xs[k+1]) from source columns [cs[k], ce[k]) (multiples of 4); parts = 1: the whole row
    int parts;                   // 1 .. 16
    int threads;                 // threads per workgroup (4 source columns each, a multiple of 64)
    int xs[17], cs[16], ce[16];
    // 1: every thread's two columns are adjacent (xs[k] + 2i, + 1) with windows 1 or 2 pairs apart
    // (kernels.hip ryx_kernel ADJ); 0: columns i and half + i of the part
    int adj = 0;
    int cpt = 2;                 // output columns per thread (2; 4 at the Lanczos-3 4:9 upscale)
    // 1: every column has the same coefficient pairs (Lanczos 2:1 columns: one phase, windows all
    // starting on the same parity), so the kernel reads them once as scalars (kernels.hip UC)
    int uc = 0;
};
hipError_t launch_ryx(const RyxDev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *ryx_instance(const RyxDev &d);

// General-row variant (plan.hpp build_ryg; kernels.hip ryg_kernel): ryx's tabled columns and column
// parts, rows from a per-row record table instead of an exact P:Q.
#ifndef IQO_RYG_PD
#define IQO_RYG_PD 4  // (variant builds: 6; plan.hpp kRygRecPad must stay >= PD + 2)
#endif
constexpr int kRygPD = IQO_RYG_PD;  // ryg_kernel: output rows loaded ahead (the instantiations' PD)
struct RygDev {
    bool lanczos;
    int srcW, srcH, dstW, dstH;
    int taps, NP;
    int m0, m1;                  // Lanczos main rows; the others are masked border rows (magic_y)
    uint32_t yM[2][16];
    int yS[2][16];
    // per output row y (dstH + padding): {first window row s(y), offset of the row's taps in rowCoef,
    // s(y + kRygPD - 1), 0} -- the kernel fetches row y + 2's record with one scalar load per row
    const int4 *rowRec;
    const uint32_t *rowCoef;     // phases x taps (c, c) splats
    const int4 *cols;            // as RyxDev
    const uint32_t *colCoef;
    int parts, threads;
    int xs[17], cs[16], ce[16];
    int cpt;                     // output columns per thread: 2 .. 4 (abi.hip ryx_dev)
    int nl = 2;                  // rows loaded per output row: 2 (downscales, windows 1 or 2 rows apart),
                                 // 1 (upscales, windows 0 or 1 rows apart)
    // upscales whose window positions hold 1 .. posRows output rows each (kernels.hip ryu_kernel):
    // per window start s, record s - posBase = {first output row, rows, tap offsets of those rows},
    // 8 ints, padded by plan.hpp kRyuPosPad records; null: ryg_kernel's NL = 1 mode
    const int4 *posRec = nullptr;  // (8 ints per record: two int4)
    int posBase = 0;
    int posRows = 2;               // the most output rows a window position holds (2 or 3)
    // ryu_kernel run mode (cpt 4, parts on multiples of 4 columns): dstW x run pairs (plan.hpp colRun)
    const uint32_t *colRun = nullptr;
    int run = 0;
};
hipError_t launch_ryg(const RygDev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
// byPos: rows by window position (ryu_kernel) -- launch_ryg: d.nl == 1 && d.posRec; a host-only plan has no
// device tables and passes what ryg_dev decided (abi.hip plan_instance; a grid query of such a plan hands
// launch_ryg placeholder table pointers in their place, which a query never dereferences).  run: the run mode in use (0: none).
const Instance *ryg_instance(const RygDev &d, bool byPos, int run);

// Exact 2:3 Lanczos-3 upscale (plan.hpp U23Tables).
struct U23Dev {
    int srcW, srcH, dstW, dstH;
    int np;                      // producing lanes per wave (0 = auto)
    int pd;                      // row groups loaded ahead (1, 2; 0 = default 1)
    uint32_t cy0, cy[2][6];      // (c, c) u16 splats: phase 0's tap, phases 1 and 2
    uint32_t cx0, cx[2][3];      // (c, 0) / (c_2q, c_2q+1) int16 pairs
    uint32_t xM[2][12];          // edge-lane exact divisions (left / right 12 columns)
    int xT[2][12];
    int m0, m1;                  // main rows; the others are masked border rows
    uint32_t yM[2][8];
    int yS[2][8];
};
hipError_t launch_u23(const U23Dev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *u23_instance(const U23Dev &d);

// Exact 2:3 Linear upscale (plan.hpp L23Tables).
struct L23Dev {
    int srcW, srcH, dstW, dstH;
    int np;                      // producing lanes per wave (0 = auto)
    int pd;                      // row groups loaded ahead (1, 2; 0 = default 2)
    uint32_t cy[3][2];           // (c, c) u16 splats of phase j's two taps
    uint32_t cx[3];              // phase j's (c_0, c_1) u16 pair
};
hipError_t launch_l23(const L23Dev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *l23_instance(const L23Dev &d);

// Exact 3:2 Area downscale (plan.hpp A32Tables).
struct A32Dev {
    int srcW, srcH, dstW, dstH;
    int np;                      // producing lanes per wave (0 = auto)
    int pd;                      // row pairs loaded ahead (2, 4, 8; 0 = default 4)
    uint32_t cy[2][2];           // (c, c) u16 splats of phase p's two taps
    uint32_t cx[2];              // phase p's (c_0, c_1) u16 pair
};
hipError_t launch_a32(const A32Dev &d, const Io &io, int rowBegin, int rowEnd, int bands, hipStream_t s, LaunchGrid *query = nullptr);
const Instance *a32_instance(const A32Dev &d);

// --- Lanczos row-band streamer (integer ratio, single phase).
struct LanczosDev {
    int KY, KX, NY, NXP, offX;
    int srcW, srcH, dstW, dstH;
    int offY;
    uint32_t cy[16];             // (c, c) u16 pairs
    uint32_t cx[16];             // (c_2p, c_2p+1) int16 pairs
    int mainBeginY, mainEndY, mainBeginX, mainEndX;
    // exact border divisions by multiply-high (plan.hpp FastLanczos): kernel arguments, so they
    // arrive in SGPRs and cost no device table
    uint32_t yTopM[16], yBotM[16], xM[8];
    int yTopS[16], yBotS[16], xT[8];
    int yTopNeg, yBotNeg, xNeg;  // bit i: border row / column i has a negative denominator
    int dbg;                     // variant builds only (kernels.hip IQO_DBG); ignored otherwise
    int prefetch;                // prefetch depth in output rows (1..3)
    // symmetric streamer (plan.hpp FastLanczos::sym)
    int sym;                     // 1: block-shared symmetric, 2: per-wave symmetric, 0: accumulator ring
    int NX, offXO;               // unpadded X taps, odd first tap column
    uint32_t cxo[8];             // (c_2p, c_2p+1) int16 pairs of the unpadded X table (Lanczos-5: below)
    int np;                      // producing lanes per wave (0 = auto)
    int rounds;                  // block-shared streamer: target rounds of resident workgroups for the
                                 // auto band count (0 = default 6, -1 = one-round makespan model)
    int stack;                   // narrow frames: several frames per workgroup (lanczos_stack_kernel)
    int tail;                    // block-shared streamer: short bands for each XCD's last frame
                                 // (0 = auto, -1 = off, n = n bands of that frame)
    // Lanczos-5 2:1 (NX = 20, block-shared symmetric streamer only) reuses fields that streamer does
    // not read, so the argument layout of every instantiation stays as it is (growing it cost C2
    // 1.5 %): X pairs 8, 9 in cy[8], cy[9] (the symmetric streamer reads cy[0 .. NY/2)); the edge
    // lanes' 8 exact divisions per side (5 border columns: left lane k < 8, right lane k >= 8,
    // identity in the interior) as multipliers in cx[0 .. 16) (the ring streamer's padded table)
    // and shifts in xM[0 .. 8), xT[0 .. 8) (the 4-column scheme's constants)
#ifdef IQO_VARIANT_DEBUG
    // variant builds only: per-workgroup {start, end (100 MHz clock), HW_ID, XCC_ID} records of the
    // block-shared streamer (scripts/probes/wg_trace.py); 0 = off.  Not in the shipped layout.
    uint64_t trace;
#endif
};
// Block-shared symmetric streamer: whether the plan's own Y table lets two outer pair sums fold into
// one multiply-add (kernels.hip sym_vertical, FOLD): a tap that is twice its neighbour,
// compared as the u16 values the kernel multiplies by -- cy[2] == 2 cy[1] in the 10-row window
// (Lanczos-3: 1 -2 -4 9 28), cy[1] == 2 cy[0] in the 12-row one (Lanczos-4: 1 2 -3 -5 9 28).
// Nothing is taken from the degree; a table without the relation runs the unfolded pass.
inline bool symb_yfold(const LanczosDev &l)
{
    if (l.sym != 1 || (l.NY != 10 && l.NY != 12))
        return false;
    const int q = l.NY == 10 ? 1 : 0;
    return (l.cy[q + 1] & 0xffffu) == ((2u * (l.cy[q] & 0xffffu)) & 0xffffu);
}
bool lanczos_stream_supported(int KY, int KX, int NY, int NXP, int offX);
hipError_t launch_lanczos_stream(const LanczosDev &l, const Io &io, int rowBegin, int rowEnd, int bands,
                                 hipStream_t s, LaunchGrid *query = nullptr);
int lanczos_stream_block(int srcW);

// --- Area integer-ratio kernel.
struct AreaDev {
    int KY, KX, srcW, dstW, dstH;
    uint32_t cy[16];             // (c, c) u16 pairs
    uint32_t cx[8];              // (c_2p, c_2p+1) u16 pairs
    int lin;                     // 1: Linear at exactly 2:1 (linear_d2_body: taps 2i+1, 2i+2, edge
    int srcH;                    //    rows / columns replicated); cy[0..1] / cx[0] its two taps
};
hipError_t launch_area_int(const AreaDev &a, const Io &io, int rowBegin, int rowEnd, hipStream_t s, LaunchGrid *query = nullptr);

// --- exact 2x bilinear upsampler.
struct LinearDev {
    int srcW, srcH, dstW, dstH;
    int F;                       // exact factor, 2 or 3
    uint32_t cy[3];              // per phase (c0, c1) u16 pairs
    uint32_t cx[3];
    int dbg;                     // variant builds only: 16 = plain (not nontemporal) stores
    int np;                      // producing lanes per wave (0 = auto)
};
hipError_t launch_linear_up2(const LinearDev &l, const Io &io, int rowBegin, int rowEnd, int bands,
                             hipStream_t s, LaunchGrid *query = nullptr);

// --- YUV 4:2:0: the Y, U and V planes of a batch in ONE launch (grid.z = plane) when both plane
// kinds have a fused instantiation; hipErrorNotSupported otherwise (launch plane by plane).
// Frame f of each plane: Io as above; all three Io must hold the same frame count.
//
// Which fused instantiation a (Y, chroma) pair of plane descriptions takes: a pure host function
// (no device query, no launch), one overload per kernel family.  The launchers below run exactly
// the kernel it returns, and iqo_host_yuv420_fused reports its label.
enum Yuv420Fused {
    kYuvNone = 0,                          // no fused instantiation: plane by plane
    kYuvLzSymb10, kYuvLzSym10,             // Lanczos-3 2:1 Y (10 row taps): block-shared / per-wave symmetric
    kYuvLzSymb8, kYuvLzSym8,               // Lanczos-2 2:1 Y (8 row taps)
    kYuvArea44, kYuvArea22, kYuvArea2y, kYuvArea4y, kYuvArea8y, kYuvArea33, kYuvArea3y, kYuvArea6y,
    kYuvLinD2,                             // Area kinds 0 .. 8 (area_int_kernel<KX, KY or any>; Linear 2:1)
    kYuvLinUp2,                            // Linear 2x
    kYuvFusedCount
};
struct Yuv420Pick {
    Yuv420Fused label = kYuvNone;
    const void *kern = nullptr;            // null exactly when label == kYuvNone
};
Yuv420Pick yuv420_fused(const LanczosDev &y, const LanczosDev &c);
Yuv420Pick yuv420_fused(const AreaDev &y, const AreaDev &c);
Yuv420Pick yuv420_fused(const LinearDev &y, const LinearDev &c);

hipError_t launch_yuv420_lanczos(const LanczosDev &y, const Io &ioY, const LanczosDev &c, const Io &ioU,
                                 const Io &ioV, hipStream_t s);
hipError_t launch_yuv420_area(const AreaDev &y, const Io &ioY, const AreaDev &c, const Io &ioU, const Io &ioV,
                              hipStream_t s);
hipError_t launch_yuv420_linear(const LinearDev &y, const Io &ioY, const LinearDev &c, const Io &ioU,
                                const Io &ioV, hipStream_t s);

} // namespace iqo_amd
