// roi.hpp -- crop-and-resize of a batch of boxes to one output size, of packed frames
// (iqo_hip_resize_rois_device) and of NV12 / I420 frames to RGB (iqo_hip_resize_rois_yuv_*_device): the per-call
// ARENA a kernel (kernels_roi.hip roi_kernel, kernels_roi_yuv.hip roi_yuv_kernel) and its CPU twin (roi_walk,
// roi_yuv_walk) both read, the per-plan cache of axis tables that fills it, and the twins.  Pure C++ (no HIP).
// (roi.cpp includes the HIP runtime header only where the HIP compiler builds it, so that colorspace.hpp's
// __host__ __device__ markers parse in its device pass; a plain C++ compiler builds both files as they are.)
//
// Box i of a call is a rectangle (x, y, w, h) of frame `frame`; a component of its output is what the planar
// resize (w, h) -> (dstW, dstH) gives on that component of the cropped image.  Each axis is independent
// (plan.hpp build_axis), so a component needs the X table of (w -> dstW) and the Y table of (h -> dstH), both in
// the one-window-per-coordinate form of plan.hpp axis_windows, so identity, replicated and masked borders are
// all one formula per axis.  A packed box has one such pair for all its channels; a YUV box one for its luma and
// one for its half-size chroma (below).
//
// Rules of both formats, each in one function of roi.cpp:
//   - a box lies inside its frame, and flags has no bit but bit 0 (box_in_frame);
//   - a table is in the arena once, however many boxes and components use it (table_for);
//   - a workgroup takes as many output rows of a box as fit in kRoiLdsTarget bytes of tap records and work
//     rows, at most kRoiMaxRows, and one row fits in kRoiLdsMax (band_rows);
//   - a call has fewer than 2^31 workgroups and 2^30 arena words (over_caps), fewer than 2^24 boxes, and byte
//     offsets within a frame's plane fit in 32 bits.
//
// Arena: one flat buffer of 32-bit words.
//   header   kRoiHdrWords words    see RoiHdr (YUV: RoiYuvHdr)
//   records  nRois x kRoiRecWords  see RoiRec (YUV: kRoiYuvRecWords, RoiYuvRec)
//   tables   every distinct X table (one per distinct length) and Y table, once
// X table (word offsets from the table's start):
//   [0] NP  coefficient pairs per column      [1] padL  work columns left of column 0 (even)
//   [2] pitchDw  work-row pitch of one channel (dwords; >= (padL + w + padR + 1) / 2, odd)
//   [3] taps of the reference's table
//   [4 ..)  dstW x {a, D}: even window start, Lanczos border divisor * 64 (0: main)
//   then    NP x dstW coefficient pairs (c_2p, c_2p+1) from the even start, pair-major
// Y table:
//   [0] nYp taps per row, padded to even       [1] taps of the reference's table     [2], [3] 0
//   [4 ..)  dstH x {start, lo, hi, deno}
//   then    dstH x nYp / 2 words, two 16-bit coefficients each
#pragma once

#include "plan.hpp"

#include <cstddef>
#include <cstdint>
#include <list>
#include <memory>
#include <unordered_map>
#include <vector>

namespace iqo_amd {

constexpr int kRoiHdrWords = 16;
constexpr int kRoiRecWords = 16;
constexpr uint32_t kRoiMagic = 0x494f5231u;  // "IOR1"
constexpr int kRoiMaxTaps = 128;             // iqo_hip.h IQO_HIP_ROI_MAX_TAPS
constexpr int kRoiLdsMax = 64 * 1024;        // iqo_hip.h IQO_HIP_ROI_LDS_BYTES: one workgroup's LDS
constexpr int kRoiLdsTarget = 16 * 1024;     // rows per workgroup: as many as fit in this (at most kRoiMaxRows)
constexpr int kRoiMaxRows = 8;

// header words
enum RoiHdr { kHMagic = 0, kHRois, kHGroups, kHDstW, kHDstH, kHChannels, kHLanczos, kHRowBytes, kHRecOff, kHWords };
// record words
enum RoiRec {
    kRFrame = 0,
    kROffLo,   // byte offset of the box's first pixel from the source base: frame * frameSt + y * srcSt + x * C
    kROffHi,
    kRX,
    kRY,
    kRW,
    kRH,
    kRFlags,   // bit 0: mirror the output columns
    kRXTab,    // word offset of the box's X table
    kRYTab,
    kRRows,    // output rows per workgroup
    kRFirst,   // first workgroup of the box
    kRGroups,  // its workgroups: ceil(dstH / rows)
    kRPitch    // work-row pitch of one channel (dwords), the X table's
};

struct RoiBox {
    int frame, x, y, w, h, flags;
};

// Host cache of axis tables in arena form, keyed by (axis, srcLen, dstLen); method and degree are the
// owner's (the stretch calls ask for the owner's dstW / dstH, the fit calls for a box's iw / ih).  Least
// recently used tables are dropped beyond `cap` bytes (a table in use by the batch being assembled stays alive
// through its shared_ptr).
class RoiTableCache {
public:
    typedef std::shared_ptr<const std::vector<uint32_t>> Table;
    RoiTableCache(Method m, unsigned degree, int dstW, int dstH, size_t capBytes = size_t(64) << 20)
        : m_(m), degree_(degree), dstW_(dstW), dstH_(dstH), cap_(capBytes)
    {
    }
    // nullptr (with *why: 0 invalid shape, 1 over kRoiMaxTaps) when the axis has no table
    Table get(bool isX, int srcLen, int dstLen, int *why);
    size_t bytes() const { return bytes_; }
    size_t misses() const { return misses_; }
    void clear();
    Method method() const { return m_; }
    int dstW() const { return dstW_; }
    int dstH() const { return dstH_; }

private:
    struct Entry {
        uint64_t key;
        Table t;
    };
    Method m_;
    unsigned degree_;
    int dstW_, dstH_;
    size_t cap_, bytes_ = 0, misses_ = 0;
    std::list<Entry> lru_;  // front: most recent
    std::unordered_map<uint64_t, std::list<Entry>::iterator> map_;
};

struct RoiLayout {
    int nRois = 0, channels = 0;
    size_t words = 0;          // arena size
    int nXTables = 0, nYTables = 0;
    uint32_t groups = 0;       // total workgroups
    size_t ldsBytes = 0;       // dynamic LDS of the launch: the largest workgroup's
    // per distinct (srcLen, dstLen): table and its word offset in the arena
    std::vector<std::pair<RoiTableCache::Table, uint32_t>> tables;
    std::vector<uint32_t> rec;  // nRois x the format's record words
    std::vector<std::pair<uint64_t, int>> xIdx, yIdx;  // sorted (srcLen << 32 | dstLen, index in tables)
    void reset();               // empty, keeping the vectors' capacity from call to call
};

// Status of roi_layout: kRoiOk, or the first offending box in *bad (-1: an argument of the call)
enum { kRoiOk = 0, kRoiInvalid = 1, kRoiUnsupported = 2 };

// Validates the call and lays the arena out.  srcSt / frameSt in bytes.
int roi_layout(RoiTableCache *cache, int channels, size_t nRois, const RoiBox *rois, size_t nFrames, size_t frameW,
               size_t frameH, size_t srcSt, size_t frameSt, RoiLayout *out, int *bad);
// Writes the arena (out->words words) to `arena`.
void roi_fill(const RoiTableCache &cache, const RoiLayout &l, size_t frameW, uint32_t *arena);

// The float epilogue's parameters (kernels.hpp NormDev without HIP types)
struct RoiNorm {
    int dtype = 0, planes = 0;  // dtype 0: U8 output
    int order[4] = {0, 0, 0, 0};
    float scale[4] = {0, 0, 0, 0}, bias[4] = {0, 0, 0, 0};
};

// CPU twin of roi_kernel: walks the arena with the kernel's integer formulas.  U8: dst rows dstSt bytes
// apart, outputs dstRoiSt apart.  Norm (n.dtype != 0): element (i, p, y, x) at i * dstRoiSt + p * planeSt +
// y * dstSt + x * elem.
void roi_walk(const uint32_t *arena, const uint8_t *src, size_t srcSt, size_t dstSt, size_t planeSt, size_t dstRoiSt,
              void *dst, const RoiNorm &n);

// ---------------------------------------------------------------- boxes of NV12 / I420 frames to RGB
//
// Box i is a rectangle with even x, y, w, h of a 4:2:0 frame.  Its Y is the planar resize (w, h) -> (dstW, dstH)
// of the cropped luma, its U and V the planar resize (w/2, h/2) -> (dstW, dstH) of the cropped chroma (the
// full-grid chroma of IQO_CHROMA_FULL), and a pixel is colorspace.hpp yuv_to_rgb of the three.  A box so
// needs four of the tables above: X of w and of w/2, Y of h and of h/2, from the one RoiTableCache -- keyed
// by (axis, length), so a chroma axis shares the table of a luma axis of its length.  The arena has the same
// tables behind a header and records of its own:
constexpr int kRoiYuvRecWords = 24;
constexpr uint32_t kRoiYuvMagic = 0x494f5931u;  // "IOY1"
enum { kRoiNv12 = 0, kRoiI420 = 1 };            // iqo_hip.h IQO_ROI_NV12 / IQO_ROI_I420

// header words: kHMagic .. kHDstH, kHLanczos, kHRecOff and kHWords as RoiHdr, and
enum RoiYuvHdr {
    kHYLayout = 5,      // kRoiNv12 / kRoiI420
    kHYRowBytes = 7,    // bytes of a row of the Y plane: frameW
    kHYRowBytesC = 10,  // bytes of a row of a chroma plane: frameW (NV12) or frameW / 2 (I420)
    kHYStY = 11,        // row strides of the Y plane and of the chroma plane(s), bytes
    kHYStC = 12
};
enum RoiYuvRec {
    kYFrame = 0,
    kYOffLo,   // byte offset of the box's first luma sample from the Y base: frame * frameSt + y * srcStY + x
    kYOffHi,
    kYOffCLo,  // ... of its first chroma sample from the UV base (NV12: + x) or the U and V bases (I420: + x / 2):
    kYOffCHi,  //     frame * frameSt + (y / 2) * srcStUV + ...
    kYX,
    kYY,
    kYW,
    kYH,
    kYFlags,
    kYXTab,    // word offsets of the luma tables (w -> dstW, h -> dstH)
    kYYTab,
    kYXTabC,   // ... and of the chroma tables (w / 2 -> dstW, h / 2 -> dstH)
    kYYTabC,
    kYRows,
    kYFirst,
    kYGroups,
    kYPitch,   // work-row pitches of the Y row and of the U and V rows (dwords), the X tables'
    kYPitchC
};

// The source of a YUV call.  frameSt applies to every plane pointer.
struct RoiYuvSrc {
    int layout = kRoiNv12;
    size_t nFrames = 0, frameW = 0, frameH = 0, stY = 0, stUV = 0, frameSt = 0;
};

// roi_layout / roi_fill of the YUV arena.  out->channels holds the layout; out->nXTables / nYTables count
// every distinct table once, whether luma, chroma or both use it.
int roi_yuv_layout(RoiTableCache *cache, const RoiYuvSrc &s, size_t nRois, const RoiBox *rois, RoiLayout *out, int *bad);
void roi_yuv_fill(const RoiTableCache &cache, const RoiLayout &l, const RoiYuvSrc &s, uint32_t *arena);

// The output of a YUV call: a colorspace.hpp standard, then packed bytes (n.dtype == 0: `channels` 3 or 4,
// byte c = order[c] of {R, G, B, 255}) or the float planes of n (n.order[p] of {R, G, B}).
struct RoiYuvOut {
    int standard = 0, channels = 3;
    int order[4] = {0, 1, 2, 3};
    RoiNorm n;
};

// CPU twin of roi_yuv_kernel.  NV12: u is the UV plane and v is not read.  Destination as roi_walk.
void roi_yuv_walk(const uint32_t *arena, const uint8_t *y, const uint8_t *u, const uint8_t *v, const RoiYuvOut &o,
                  size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dst);

// ---------------------------------------------------------------- boxes into destination rectangles (fit)
//
// Output i of a fit call is a dstW x dstH canvas: rectangle (ox, oy, iw, ih) of it holds what the stretch call
// gives for box i with (iw, ih) in place of (dstW, dstH) -- so its tables are those of (w -> iw) and (h -> ih),
// from the same cache -- and every pixel outside it is the call's pad colour.  Both families have a fit format of
// their own, so the stretch arenas stay word for word what they were: the same header, and records that begin
// with the stretch record's words and carry RoiFitRec from word kRoiFitExt (YUV: kRoiYuvFitExt) on.
//
// Who writes which pad byte: a band workgroup (one of ceil(ih / rows), rows from band_rows(ih, ...)) writes the
// pad columns left and right of its own rows; the rows above and below the rectangle are written by pad
// workgroups of the same launch, kRoiPadRows whole rows each, ceil(oy / kRoiPadRows) above and
// ceil((dstH - oy - ih) / kRoiPadRows) below.  A box's workgroups are numbered from its kRFirst: pad above, bands,
// pad below.  The pad colour is an argument of the call, not of the arena.
constexpr int kRoiFitRecWords = 24, kRoiFitExt = 16;
constexpr int kRoiYuvFitRecWords = 32, kRoiYuvFitExt = 24;
constexpr uint32_t kRoiFitMagic = 0x494f5232u;     // "IOR2"
constexpr uint32_t kRoiYuvFitMagic = 0x494f5932u;  // "IOY2"
// Rows of the canvas one pad workgroup writes.  NOT MEASURED: 32 keeps a workgroup's share of a 640-wide fp16
// RGB canvas near 120 KB and gives a 140-row border five workgroups; nobody has timed other values.
constexpr int kRoiPadRows = 32;
enum RoiFitRec { kFIW = 0, kFIH, kFOX, kFOY, kFPadAbove, kFPadBelow };  // words from the format's Ext on

struct RoiRect {
    int x, y, w, h;
};

// roi_layout / roi_fill / roi_walk of the fit formats.  rects: nRois rectangles, or nullptr (every rectangle is
// the whole output).  A rectangle outside the output or with w or h below 1 is kRoiInvalid at its box; the
// stretch rules hold with (iw, ih) for (dstW, dstH).  pad: the bytes of the channels (packed) or R, G, B (YUV,
// stored through the output's order as a pixel is; the fourth byte of a 4-byte pixel stays 255).
int roi_fit_layout(RoiTableCache *cache, int channels, size_t nRois, const RoiBox *rois, const RoiRect *rects,
                   size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t frameSt, RoiLayout *out, int *bad);
void roi_fit_fill(const RoiTableCache &cache, const RoiLayout &l, size_t frameW, uint32_t *arena);
void roi_fit_walk(const uint32_t *arena, const uint8_t *src, size_t srcSt, size_t dstSt, size_t planeSt, size_t dstRoiSt,
                  void *dst, const RoiNorm &n, const uint8_t pad[4]);
int roi_yuv_fit_layout(RoiTableCache *cache, const RoiYuvSrc &s, size_t nRois, const RoiBox *rois, const RoiRect *rects,
                       RoiLayout *out, int *bad);
void roi_yuv_fit_fill(const RoiTableCache &cache, const RoiLayout &l, const RoiYuvSrc &s, uint32_t *arena);
void roi_yuv_fit_walk(const uint32_t *arena, const uint8_t *y, const uint8_t *u, const uint8_t *v, const RoiYuvOut &o,
                      size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dst, const uint8_t pad[4]);

// The rectangle of a w x h box in a dstW x dstH output, in 64-bit integers: if w * dstH >= h * dstW then
// iw = dstW, ih = max(1, (h * dstW + w / 2) / w), else ih = dstH, iw = max(1, (w * dstH + h / 2) / h); centred
// (ox = (dstW - iw) / 2, oy = (dstH - ih) / 2) or at the top left.  mode 0: the whole output.
enum { kFitStretch = 0, kFitLetterbox = 1, kFitLetterboxTopLeft = 2 };
bool fit_rect(int mode, uint64_t w, uint64_t h, uint64_t dstW, uint64_t dstH, RoiRect *out);

} // namespace iqo_amd
