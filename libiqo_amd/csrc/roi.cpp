// roi.cpp -- host side of the batched crop-and-resize (roi.hpp): axis tables in arena form and their
// cache, validation and layout of a call's arena, and the CPU twin of roi_kernel.
#include "roi.hpp"

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (the device half of colorspace.hpp, when the HIP compiler builds this file)
#endif
#include "colorspace.hpp"

#include <algorithm>
#include <cstring>
#include <string>

namespace iqo_amd {

namespace {

// One axis table in arena form (roi.hpp); empty when the axis has no defined result (*why = 0) or its
// reference table has more than kRoiMaxTaps taps (*why = 1).
std::vector<uint32_t> build_roi_table(Method m, unsigned degree, int srcLen, int dstLen, bool isX, int *why)
{
    std::vector<uint32_t> t;
    AxisPlan a;
    std::string err;
    *why = 0;
    if (!build_axis(m, degree, static_cast<size_t>(srcLen), static_cast<size_t>(dstLen), isX, &a, &err))
        return t;
    *why = 1;
    if (a.taps > kRoiMaxTaps)
        return t;
    std::vector<AxisWindow> w;
    axis_windows(m, a, isX, &w);
    size_t n = 1;
    for (const AxisWindow &v : w)
        n = std::max(n, v.c.size());
    if (isX) {
        const int NP = static_cast<int>((n + 1) / 2);
        int minA = 0, maxEnd = srcLen;
        for (const AxisWindow &v : w) {
            minA = std::min(minA, v.start);
            maxEnd = std::max(maxEnd, v.start + 2 * NP);
        }
        const int padL = (-minA + 1) & ~1;
        const int pitchDw = ((padL + maxEnd + 1) / 2) | 1;
        t.assign(4 + static_cast<size_t>(dstLen) * (2 + NP), 0u);
        t[0] = static_cast<uint32_t>(NP);
        t[1] = static_cast<uint32_t>(padL);
        t[2] = static_cast<uint32_t>(pitchDw);
        t[3] = static_cast<uint32_t>(a.taps);
        uint32_t *col = t.data() + 4, *coef = col + 2 * static_cast<size_t>(dstLen);
        for (int x = 0; x < dstLen; ++x) {
            const AxisWindow &v = w[static_cast<size_t>(x)];
            col[2 * x] = static_cast<uint32_t>(v.start);
            col[2 * x + 1] = static_cast<uint32_t>(v.div);
            for (size_t k = 0; k < v.c.size(); ++k)
                coef[(k / 2) * static_cast<size_t>(dstLen) + x] |= static_cast<uint32_t>(v.c[k]) << (16 * (k & 1));
        }
    } else {
        const int nYp = static_cast<int>((n + 1) & ~size_t(1));
        t.assign(4 + static_cast<size_t>(dstLen) * (4 + nYp / 2), 0u);
        t[0] = static_cast<uint32_t>(nYp);
        t[1] = static_cast<uint32_t>(a.taps);
        uint32_t *row = t.data() + 4, *coef = row + 4 * static_cast<size_t>(dstLen);
        for (int y = 0; y < dstLen; ++y) {
            const AxisWindow &v = w[static_cast<size_t>(y)];
            row[4 * y] = static_cast<uint32_t>(v.start);
            row[4 * y + 1] = static_cast<uint32_t>(v.lo);
            row[4 * y + 2] = static_cast<uint32_t>(v.hi);
            row[4 * y + 3] = static_cast<uint32_t>(v.div);
            for (size_t k = 0; k < v.c.size(); ++k)
                coef[static_cast<size_t>(y) * (nYp / 2) + k / 2] |= static_cast<uint32_t>(v.c[k]) << (16 * (k & 1));
        }
    }
    return t;
}

} // namespace

RoiTableCache::Table RoiTableCache::get(bool isX, int srcLen, int dstLen, int *why)
{
    // (srcLen <= 2^24, dstLen <= 2^20)
    const uint64_t key = (static_cast<uint64_t>(isX) << 63) | (static_cast<uint64_t>(static_cast<uint32_t>(srcLen)) << 32) |
                         static_cast<uint32_t>(dstLen);
    auto it = map_.find(key);
    if (it != map_.end()) {
        lru_.splice(lru_.begin(), lru_, it->second);
        return it->second->t;
    }
    std::vector<uint32_t> t = build_roi_table(m_, degree_, srcLen, dstLen, isX, why);
    if (t.empty())
        return nullptr;
    ++misses_;
    Table tab = std::make_shared<const std::vector<uint32_t>>(std::move(t));
    lru_.push_front(Entry{key, tab});
    map_[key] = lru_.begin();
    bytes_ += tab->size() * 4;
    while (bytes_ > cap_ && lru_.size() > 1) {
        const Entry &e = lru_.back();
        bytes_ -= e.t->size() * 4;
        map_.erase(e.key);
        lru_.pop_back();
    }
    return tab;
}

void RoiTableCache::clear()
{
    lru_.clear();
    map_.clear();
    bytes_ = 0;
}

void RoiLayout::reset()
{
    // (cleared member by member: a plan's layout keeps its capacity from call to call)
    nRois = channels = nXTables = nYTables = 0;
    words = ldsBytes = 0;
    groups = 0;
    tables.clear();
    rec.clear();
    xIdx.clear();
    yIdx.clear();
}

namespace {

struct TableRef {
    const uint32_t *t = nullptr;  // nullptr: the axis has no table, and *status says why
    uint32_t off = 0;             // its word offset in the arena
};

// The table of (axis, len -> dstLen) in the layout, appended at *words (from the cache) where the call has none yet.
TableRef table_for(RoiTableCache *cache, RoiLayout *l, bool isX, int len, int dstLen, size_t *words, int *status)
{
    std::vector<std::pair<uint64_t, int>> &idx = isX ? l->xIdx : l->yIdx;
    const uint64_t key = (static_cast<uint64_t>(static_cast<uint32_t>(len)) << 32) | static_cast<uint32_t>(dstLen);
    auto it = std::lower_bound(idx.begin(), idx.end(), std::make_pair(key, 0));
    if (it == idx.end() || it->first != key) {
        int why = 0;
        RoiTableCache::Table t = cache->get(isX, len, dstLen, &why);
        if (!t) {
            *status = why ? kRoiUnsupported : kRoiInvalid;
            return TableRef();
        }
        it = idx.insert(it, std::make_pair(key, static_cast<int>(l->tables.size())));
        l->tables.emplace_back(t, static_cast<uint32_t>(*words));
        *words += t->size();
        ++(isX ? l->nXTables : l->nYTables);
    }
    const auto &e = l->tables[static_cast<size_t>(it->second)];
    TableRef r;
    r.t = e.first->data();
    r.off = e.second;
    return r;
}

bool box_in_frame(const RoiBox &b, size_t nFrames, size_t frameW, size_t frameH)
{
    return b.w > 0 && b.h > 0 && b.x >= 0 && b.y >= 0 && static_cast<size_t>(b.x) + static_cast<size_t>(b.w) <= frameW &&
           static_cast<size_t>(b.y) + static_cast<size_t>(b.h) <= frameH && b.frame >= 0 &&
           static_cast<size_t>(b.frame) < nFrames && !(b.flags & ~1);
}

// Output rows per workgroup of a box whose band row takes rowBytes of LDS (tap records and work rows): as many
// as fit in kRoiLdsTarget, at most kRoiMaxRows; 0 when one row is over kRoiLdsMax.  *ldsBytes: the call's largest.
int band_rows(int dstH, size_t rowBytes, size_t *ldsBytes)
{
    if (rowBytes > static_cast<size_t>(kRoiLdsMax))
        return 0;
    const int rows = std::max(1, std::min(std::min(dstH, kRoiMaxRows), static_cast<int>(kRoiLdsTarget / rowBytes)));
    *ldsBytes = std::max(*ldsBytes, rows * rowBytes);
    return rows;
}

// more boxes than one grid (or one arena) can address
bool over_caps(uint64_t groups, size_t words) { return groups >= (uint64_t(1) << 31) || words >= (size_t(1) << 30); }

// The destination rectangle of box i: the whole output in a stretch call and where a fit call brings no
// rectangles.  false: it does not lie inside the output, or is less than a pixel wide or high.
bool rect_of(const RoiRect *rects, size_t i, int dstW, int dstH, RoiRect *r)
{
    *r = rects ? rects[i] : RoiRect{0, 0, dstW, dstH};
    return r->w >= 1 && r->h >= 1 && r->x >= 0 && r->y >= 0 && r->x <= dstW - r->w && r->y <= dstH - r->h;
}

// The fit words of a record (roi.hpp RoiFitRec) whose box has g bands; returns all its workgroups: the pad
// workgroups above the rectangle, the bands, the pad workgroups below it.
uint64_t fit_words(uint32_t *ext, const RoiRect &r, int dstH, uint32_t g)
{
    const uint32_t above = static_cast<uint32_t>((r.y + kRoiPadRows - 1) / kRoiPadRows);
    const uint32_t below = static_cast<uint32_t>((dstH - r.y - r.h + kRoiPadRows - 1) / kRoiPadRows);
    ext[kFIW] = static_cast<uint32_t>(r.w);
    ext[kFIH] = static_cast<uint32_t>(r.h);
    ext[kFOX] = static_cast<uint32_t>(r.x);
    ext[kFOY] = static_cast<uint32_t>(r.y);
    ext[kFPadAbove] = above;
    ext[kFPadBelow] = below;
    return static_cast<uint64_t>(above) + g + below;
}

// The header words all four formats share, the records and the tables.
void fill_common(uint32_t magic, const RoiTableCache &cache, const RoiLayout &l, uint32_t *arena)
{
    std::memset(arena, 0, kRoiHdrWords * 4);
    arena[kHMagic] = magic;
    arena[kHRois] = static_cast<uint32_t>(l.nRois);
    arena[kHGroups] = l.groups;
    arena[kHDstW] = static_cast<uint32_t>(cache.dstW());
    arena[kHDstH] = static_cast<uint32_t>(cache.dstH());
    arena[kHLanczos] = cache.method() == kLanczos ? 1u : 0u;
    arena[kHRecOff] = kRoiHdrWords;
    arena[kHWords] = static_cast<uint32_t>(l.words);
    if (!l.rec.empty())
        std::memcpy(arena + kRoiHdrWords, l.rec.data(), l.rec.size() * 4);
    for (const auto &t : l.tables)
        std::memcpy(arena + t.second, t.first->data(), t.first->size() * 4);
}

// roi_layout (fit == false: every box to the whole output, stretch records) and roi_fit_layout
int layout_packed(bool fit, RoiTableCache *cache, int channels, size_t nRois, const RoiBox *rois, const RoiRect *rects,
                  size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t frameSt, RoiLayout *out, int *bad)
{
    const size_t recWords = fit ? kRoiFitRecWords : kRoiRecWords;
    out->reset();
    *bad = -1;
    if (channels != 1 && channels != 3 && channels != 4)
        return kRoiUnsupported;
    const size_t C = static_cast<size_t>(channels);
    if (!frameW || !frameH || frameW > (1u << 24) || frameH > (1u << 24) || srcSt < frameW * C ||
        (nRois && !rois) || cache->dstW() < 1 || cache->dstH() < 1)
        return kRoiInvalid;
    // the kernel keeps byte offsets within a frame's rows in 32 bits
    if (srcSt >= (size_t(1) << 31) / frameH)
        return kRoiUnsupported;
    if (nRois >= (size_t(1) << 24))
        return kRoiUnsupported;
    out->nRois = static_cast<int>(nRois);
    out->channels = channels;
    out->rec.assign(nRois * recWords, 0u);
    size_t words = kRoiHdrWords + nRois * recWords;
    uint64_t groups = 0;
    for (size_t i = 0; i < nRois; ++i) {
        const RoiBox &b = rois[i];
        *bad = static_cast<int>(i);
        RoiRect rc;
        if (!box_in_frame(b, nFrames, frameW, frameH) || !rect_of(fit ? rects : nullptr, i, cache->dstW(), cache->dstH(), &rc))
            return kRoiInvalid;
        const int dstH = rc.h;
        int st = kRoiOk;
        const TableRef x = table_for(cache, out, true, b.w, rc.w, &words, &st);
        const TableRef y = x.t ? table_for(cache, out, false, b.h, rc.h, &words, &st) : x;
        if (!y.t)
            return st;
        // a band row: its tap records and its work rows over the box's width and channels
        const size_t pitchDw = x.t[2], nYp = y.t[0];
        const int rows = band_rows(dstH, C * pitchDw * 4 + nYp * 8, &out->ldsBytes);
        if (!rows)
            return kRoiUnsupported;
        const uint32_t g = static_cast<uint32_t>((dstH + rows - 1) / rows);
        const uint64_t off = static_cast<uint64_t>(b.frame) * frameSt + static_cast<uint64_t>(b.y) * srcSt +
                             static_cast<uint64_t>(b.x) * C;
        uint32_t *r = out->rec.data() + i * recWords;
        r[kRFrame] = static_cast<uint32_t>(b.frame);
        r[kROffLo] = static_cast<uint32_t>(off);
        r[kROffHi] = static_cast<uint32_t>(off >> 32);
        r[kRX] = static_cast<uint32_t>(b.x);
        r[kRY] = static_cast<uint32_t>(b.y);
        r[kRW] = static_cast<uint32_t>(b.w);
        r[kRH] = static_cast<uint32_t>(b.h);
        r[kRFlags] = static_cast<uint32_t>(b.flags);
        r[kRXTab] = x.off;
        r[kRYTab] = y.off;
        r[kRRows] = static_cast<uint32_t>(rows);
        r[kRFirst] = static_cast<uint32_t>(groups);
        r[kRGroups] = g;
        r[kRPitch] = static_cast<uint32_t>(pitchDw);
        groups += fit ? fit_words(r + kRoiFitExt, rc, cache->dstH(), g) : g;
        if (over_caps(groups, words))
            return kRoiUnsupported;
    }
    *bad = -1;
    out->words = words;
    out->groups = static_cast<uint32_t>(groups);
    return kRoiOk;
}

void fill_packed(uint32_t magic, const RoiTableCache &cache, const RoiLayout &l, size_t frameW, uint32_t *arena)
{
    fill_common(magic, cache, l, arena);
    arena[kHChannels] = static_cast<uint32_t>(l.channels);
    arena[kHRowBytes] = static_cast<uint32_t>(frameW * static_cast<size_t>(l.channels));
}

} // namespace

int roi_layout(RoiTableCache *cache, int channels, size_t nRois, const RoiBox *rois, size_t nFrames, size_t frameW,
               size_t frameH, size_t srcSt, size_t frameSt, RoiLayout *out, int *bad)
{
    return layout_packed(false, cache, channels, nRois, rois, nullptr, nFrames, frameW, frameH, srcSt, frameSt, out, bad);
}

int roi_fit_layout(RoiTableCache *cache, int channels, size_t nRois, const RoiBox *rois, const RoiRect *rects,
                   size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t frameSt, RoiLayout *out, int *bad)
{
    return layout_packed(true, cache, channels, nRois, rois, rects, nFrames, frameW, frameH, srcSt, frameSt, out, bad);
}

void roi_fill(const RoiTableCache &cache, const RoiLayout &l, size_t frameW, uint32_t *arena)
{
    fill_packed(kRoiMagic, cache, l, frameW, arena);
}

void roi_fit_fill(const RoiTableCache &cache, const RoiLayout &l, size_t frameW, uint32_t *arena)
{
    fill_packed(kRoiFitMagic, cache, l, frameW, arena);
}

// ---------------------------------------------------------------- CPU twin

namespace {

// round-to-nearest-even float -> fp16 / bf16 bit patterns (overflow to +-inf), as the kernel's conversions
uint16_t f16_bits_host(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    const uint32_t sign = (u >> 16) & 0x8000u;
    u &= 0x7fffffffu;
    if (u >= 0x7f800000u)
        return static_cast<uint16_t>(sign | (u > 0x7f800000u ? 0x7e00u : 0x7c00u));
    if (u >= 0x477ff000u)  // rounds to >= 2^16
        return static_cast<uint16_t>(sign | 0x7c00u);
    if (u < 0x38800000u) {  // subnormal half (or zero): value * 2^24 rounded to an integer
        if (u < 0x33000000u)
            return static_cast<uint16_t>(sign);  // < 2^-25: rounds to zero (2^-25 itself ties to even: zero)
        const int e = static_cast<int>(u >> 23);                // biased exponent, 102 .. 112
        const uint32_t man = (u & 0x7fffffu) | 0x800000u;       // 24-bit significand
        const int shift = 126 - e;                              // 14 .. 24
        const uint32_t q = man >> shift, rem = man & ((1u << shift) - 1u), half = 1u << (shift - 1);
        return static_cast<uint16_t>(sign | (q + ((rem > half || (rem == half && (q & 1u))) ? 1u : 0u)));
    }
    const uint32_t v = u - 0x38000000u;  // rebias 127 -> 15
    const uint32_t q = v >> 13, rem = v & 0x1fffu;
    return static_cast<uint16_t>(sign | (q + ((rem > 0x1000u || (rem == 0x1000u && (q & 1u))) ? 1u : 0u)));
}

uint16_t bf16_bits_host(float f)
{
    uint32_t u;
    std::memcpy(&u, &f, 4);
    if ((u & 0x7fffffffu) > 0x7f800000u)
        return static_cast<uint16_t>((u >> 16) | 0x40u);
    return static_cast<uint16_t>((u + 0x7fffu + ((u >> 16) & 1u)) >> 16);
}

// One component's bytes of output row y of a box, with the kernels' integer formulas: sample q of source row rr
// is box[rr * st + q * step] (step C: one channel of interleaved pixels, one half of a UV row), n samples per row.
void component_row(const uint32_t *xt, const uint32_t *yt, int dstW, int dstH, bool LZ, const uint8_t *box, size_t st,
                       int step, int n, int y, std::vector<uint16_t> *workV, uint8_t *out)
{
    const int NP = static_cast<int>(xt[0]), padL = static_cast<int>(xt[1]), pitch = 2 * static_cast<int>(xt[2]);
    const int32_t *col = reinterpret_cast<const int32_t *>(xt + 4);
    const uint32_t *cx = xt + 4 + 2 * static_cast<size_t>(dstW);
    const int nYp = static_cast<int>(yt[0]);
    const int32_t *row = reinterpret_cast<const int32_t *>(yt + 4);
    const uint32_t *cy = yt + 4 + 4 * static_cast<size_t>(dstH);
    workV->assign(static_cast<size_t>(pitch), 0);
    uint16_t *work = workV->data();
    const int32_t start = row[4 * y], lo = row[4 * y + 1], hi = row[4 * y + 2], deno = row[4 * y + 3];
    // vertical: 16-bit wrapping sums over the row window, rows clamped to the box
    for (int q = 0; q < n; ++q) {
        uint16_t acc = 0;
        for (int k = 0; k < nYp; ++k) {
            const int rr = std::max(lo, std::min(start + k, hi));
            const uint16_t c = static_cast<uint16_t>(cy[static_cast<size_t>(y) * (nYp / 2) + k / 2] >> (16 * (k & 1)));
            acc = static_cast<uint16_t>(acc + box[static_cast<size_t>(rr) * st + static_cast<size_t>(q) * step] * c);
        }
        if (LZ && deno != 0)
            acc = static_cast<uint16_t>(static_cast<int16_t>(static_cast<int>(static_cast<int16_t>(acc)) * 64 / deno));
        work[padL + q] = acc;
    }
    for (int k = 0; k < padL; ++k)  // columns outside the box: the clamped edge column
        work[k] = work[padL];
    for (int k = padL + n; k < pitch; ++k)
        work[k] = work[padL + n - 1];
    // horizontal
    for (int x = 0; x < dstW; ++x) {
        const int32_t a = col[2 * x], D = col[2 * x + 1];
        const uint16_t *wr = work + padL + a;
        if (LZ) {
            int32_t s = 1 << 19;
            for (int p = 0; p < NP; ++p) {
                const uint32_t cf = cx[static_cast<size_t>(p) * dstW + x];
                s += static_cast<int16_t>(wr[2 * p]) * static_cast<int16_t>(cf & 0xffffu) +
                     static_cast<int16_t>(wr[2 * p + 1]) * static_cast<int16_t>(cf >> 16);
            }
            int v = s >> 20;
            if (D != 0)
                v = static_cast<int16_t>(s / D);
            out[x] = static_cast<uint8_t>(std::min(std::max(v, 0), 255));
        } else {
            uint32_t s = 1u << 22;
            for (int p = 0; p < NP; ++p) {
                const uint32_t cf = cx[static_cast<size_t>(p) * dstW + x];
                s += static_cast<uint32_t>(wr[2 * p]) * (cf & 0xffffu) + static_cast<uint32_t>(wr[2 * p + 1]) * (cf >> 16);
            }
            out[x] = static_cast<uint8_t>(std::min((s >> 23) & 0xffffu, 255u));
        }
    }
}

// One output pixel at column xo of row `o` (of its box's first plane): bytes px[order[c]], c < channels
// (n.dtype == 0), or plane p = px[n.order[p]] scaled and biased, planeSt bytes apart.
void store_pixel(const int px[4], int channels, const int order[4], const RoiNorm &n, size_t planeSt, uint8_t *o, int xo)
{
    if (n.dtype == 0) {
        uint8_t *e = o + static_cast<size_t>(xo) * channels;
        for (int c = 0; c < channels; ++c)
            e[c] = static_cast<uint8_t>(px[order[c]]);
        return;
    }
    const size_t elem = n.dtype == 1 ? 4 : 2;
    for (int p = 0; p < n.planes; ++p) {
        volatile float m = static_cast<float>(px[n.order[p]]) * n.scale[p];  // two roundings
        const float f = m + n.bias[p];
        uint8_t *e = o + static_cast<size_t>(p) * planeSt + static_cast<size_t>(xo) * elem;
        if (n.dtype == 1) {
            std::memcpy(e, &f, 4);
        } else {
            const uint16_t h = n.dtype == 2 ? f16_bits_host(f) : bf16_bits_host(f);
            std::memcpy(e, &h, 2);
        }
    }
}

// The rectangle of a record: the whole output (ext == nullptr: a stretch record), or its fit words
RoiRect rect_in(const uint32_t *ext, int dstW, int dstH)
{
    if (!ext)
        return RoiRect{0, 0, dstW, dstH};
    return RoiRect{static_cast<int>(ext[kFOX]), static_cast<int>(ext[kFOY]), static_cast<int>(ext[kFIW]), static_cast<int>(ext[kFIH])};
}

// Every pixel of a dstW x dstH canvas outside rc: px
void pad_canvas(const RoiRect &rc, int dstW, int dstH, const int px[4], int channels, const int order[4], const RoiNorm &n,
                size_t planeSt, size_t dstSt, uint8_t *canvas)
{
    for (int y = 0; y < dstH; ++y)
        for (int x = 0; x < dstW; ++x)
            if (y < rc.y || y >= rc.y + rc.h || x < rc.x || x >= rc.x + rc.w)
                store_pixel(px, channels, order, n, planeSt, canvas + static_cast<size_t>(y) * dstSt, x);
}

// roi_walk (pad == nullptr: stretch records) and roi_fit_walk
void walk_packed(const uint32_t *arena, const uint8_t *src, size_t srcSt, size_t dstSt, size_t planeSt, size_t dstRoiSt,
                 void *dstV, const RoiNorm &n, const uint8_t *pad)
{
    const size_t recWords = pad ? kRoiFitRecWords : kRoiRecWords;
    const int nRois = static_cast<int>(arena[kHRois]);
    const int dstW = static_cast<int>(arena[kHDstW]), dstH = static_cast<int>(arena[kHDstH]);
    const int C = static_cast<int>(arena[kHChannels]);
    const bool LZ = arena[kHLanczos] != 0;
    const int order[4] = {0, 1, 2, 3};
    uint8_t *dst = static_cast<uint8_t *>(dstV);
    std::vector<uint16_t> work;
    std::vector<uint8_t> line(static_cast<size_t>(C) * dstW);
    for (int i = 0; i < nRois; ++i) {
        const uint32_t *r = arena + arena[kHRecOff] + static_cast<size_t>(i) * recWords;
        const uint8_t *box = src + ((static_cast<uint64_t>(r[kROffHi]) << 32) | r[kROffLo]);
        const int w = static_cast<int>(r[kRW]);
        const bool flip = r[kRFlags] & 1u;
        const uint32_t *xt = arena + r[kRXTab], *yt = arena + r[kRYTab];
        const RoiRect rc = rect_in(pad ? r + kRoiFitExt : nullptr, dstW, dstH);
        uint8_t *canvas = dst + static_cast<size_t>(i) * dstRoiSt;
        if (pad) {
            const int px[4] = {pad[0], pad[1], pad[2], pad[3]};
            pad_canvas(rc, dstW, dstH, px, C, order, n, planeSt, dstSt, canvas);
        }
        for (int y = 0; y < rc.h; ++y) {
            for (int c = 0; c < C; ++c)
                component_row(xt, yt, rc.w, rc.h, LZ, box + c, srcSt, C, w, y, &work, line.data() + static_cast<size_t>(c) * rc.w);
            uint8_t *o = canvas + static_cast<size_t>(rc.y + y) * dstSt;
            for (int x = 0; x < rc.w; ++x) {
                int px[4] = {0, 0, 0, 0};
                for (int c = 0; c < C; ++c)
                    px[c] = line[static_cast<size_t>(c) * rc.w + x];
                store_pixel(px, C, order, n, planeSt, o, rc.x + (flip ? rc.w - 1 - x : x));
            }
        }
    }
}

} // namespace

void roi_walk(const uint32_t *arena, const uint8_t *src, size_t srcSt, size_t dstSt, size_t planeSt, size_t dstRoiSt,
              void *dst, const RoiNorm &n)
{
    walk_packed(arena, src, srcSt, dstSt, planeSt, dstRoiSt, dst, n, nullptr);
}

void roi_fit_walk(const uint32_t *arena, const uint8_t *src, size_t srcSt, size_t dstSt, size_t planeSt, size_t dstRoiSt,
                  void *dst, const RoiNorm &n, const uint8_t pad[4])
{
    walk_packed(arena, src, srcSt, dstSt, planeSt, dstRoiSt, dst, n, pad);
}

// ---------------------------------------------------------------- boxes of NV12 / I420 frames to RGB

namespace {

// roi_yuv_layout (fit == false: every box to the whole output, stretch records) and roi_yuv_fit_layout
int layout_yuv(bool fit, RoiTableCache *cache, const RoiYuvSrc &s, size_t nRois, const RoiBox *rois, const RoiRect *rects,
               RoiLayout *out, int *bad)
{
    const size_t recWords = fit ? kRoiYuvFitRecWords : kRoiYuvRecWords;
    out->reset();
    *bad = -1;
    const bool nv12 = s.layout == kRoiNv12;
    if ((!nv12 && s.layout != kRoiI420) || !s.frameW || !s.frameH || (s.frameW & 1) || (s.frameH & 1) ||
        s.frameW > (1u << 24) || s.frameH > (1u << 24) || s.stY < s.frameW || s.stUV < (nv12 ? s.frameW : s.frameW / 2) ||
        (nRois && !rois) || cache->dstW() < 1 || cache->dstH() < 1)
        return kRoiInvalid;
    // the kernel keeps byte offsets within a frame's planes in 32 bits
    if (s.stY >= (size_t(1) << 31) / s.frameH || s.stUV >= (size_t(1) << 31) / (s.frameH / 2))
        return kRoiUnsupported;
    if (nRois >= (size_t(1) << 24))
        return kRoiUnsupported;
    out->nRois = static_cast<int>(nRois);
    out->channels = s.layout;
    out->rec.assign(nRois * recWords, 0u);
    size_t words = kRoiHdrWords + nRois * recWords;
    uint64_t groups = 0;
    const bool linear = cache->method() == kLinear;
    for (size_t i = 0; i < nRois; ++i) {
        const RoiBox &b = rois[i];
        *bad = static_cast<int>(i);
        RoiRect rc;
        if (!box_in_frame(b, s.nFrames, s.frameW, s.frameH) || ((b.x | b.y | b.w | b.h) & 1) ||
            !rect_of(fit ? rects : nullptr, i, cache->dstW(), cache->dstH(), &rc))
            return kRoiInvalid;
        const int dstW = rc.w, dstH = rc.h;
        // Linear chroma above 2x has no pinned answer (the rule of the YUV plans' full-grid chroma)
        if (linear && (dstW > b.w || dstH > b.h))
            return kRoiUnsupported;
        // tables: X of w, Y of h, X of w / 2, Y of h / 2
        TableRef t[4];
        int st = kRoiOk;
        for (int k = 0; k < 4; ++k) {
            t[k] = table_for(cache, out, !(k & 1), ((k & 1) ? b.h : b.w) >> (k >> 1), (k & 1) ? dstH : dstW, &words, &st);
            if (!t[k].t)
                return st;
        }
        // a band row: both sets of tap records, and the Y, U and V work rows
        const size_t pitchY = t[0].t[2], pitchC = t[2].t[2], nYpY = t[1].t[0], nYpC = t[3].t[0];
        const int rows = band_rows(dstH, (pitchY + 2 * pitchC) * 4 + (nYpY + nYpC) * 8, &out->ldsBytes);
        if (!rows)
            return kRoiUnsupported;
        const uint32_t g = static_cast<uint32_t>((dstH + rows - 1) / rows);
        const uint64_t frame = static_cast<uint64_t>(b.frame) * s.frameSt;
        const uint64_t off = frame + static_cast<uint64_t>(b.y) * s.stY + static_cast<uint64_t>(b.x);
        const uint64_t offC = frame + static_cast<uint64_t>(b.y / 2) * s.stUV + static_cast<uint64_t>(nv12 ? b.x : b.x / 2);
        uint32_t *r = out->rec.data() + i * recWords;
        r[kYFrame] = static_cast<uint32_t>(b.frame);
        r[kYOffLo] = static_cast<uint32_t>(off);
        r[kYOffHi] = static_cast<uint32_t>(off >> 32);
        r[kYOffCLo] = static_cast<uint32_t>(offC);
        r[kYOffCHi] = static_cast<uint32_t>(offC >> 32);
        r[kYX] = static_cast<uint32_t>(b.x);
        r[kYY] = static_cast<uint32_t>(b.y);
        r[kYW] = static_cast<uint32_t>(b.w);
        r[kYH] = static_cast<uint32_t>(b.h);
        r[kYFlags] = static_cast<uint32_t>(b.flags);
        r[kYXTab] = t[0].off;
        r[kYYTab] = t[1].off;
        r[kYXTabC] = t[2].off;
        r[kYYTabC] = t[3].off;
        r[kYRows] = static_cast<uint32_t>(rows);
        r[kYFirst] = static_cast<uint32_t>(groups);
        r[kYGroups] = g;
        r[kYPitch] = static_cast<uint32_t>(pitchY);
        r[kYPitchC] = static_cast<uint32_t>(pitchC);
        groups += fit ? fit_words(r + kRoiYuvFitExt, rc, cache->dstH(), g) : g;
        if (over_caps(groups, words))
            return kRoiUnsupported;
    }
    *bad = -1;
    out->words = words;
    out->groups = static_cast<uint32_t>(groups);
    return kRoiOk;
}

void fill_yuv(uint32_t magic, const RoiTableCache &cache, const RoiLayout &l, const RoiYuvSrc &s, uint32_t *arena)
{
    fill_common(magic, cache, l, arena);
    arena[kHYLayout] = static_cast<uint32_t>(s.layout);
    arena[kHYRowBytes] = static_cast<uint32_t>(s.frameW);
    arena[kHYRowBytesC] = static_cast<uint32_t>(s.layout == kRoiNv12 ? s.frameW : s.frameW / 2);
    arena[kHYStY] = static_cast<uint32_t>(s.stY);
    arena[kHYStC] = static_cast<uint32_t>(s.stUV);
}

// roi_yuv_walk (pad == nullptr: stretch records) and roi_yuv_fit_walk
void walk_yuv(const uint32_t *arena, const uint8_t *yP, const uint8_t *uP, const uint8_t *vP, const RoiYuvOut &o,
              size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dstV, const uint8_t *pad)
{
    const size_t recWords = pad ? kRoiYuvFitRecWords : kRoiYuvRecWords;
    const int nRois = static_cast<int>(arena[kHRois]);
    const int dstW = static_cast<int>(arena[kHDstW]), dstH = static_cast<int>(arena[kHDstH]);
    const bool LZ = arena[kHLanczos] != 0, nv12 = arena[kHYLayout] == static_cast<uint32_t>(kRoiNv12);
    const size_t stY = arena[kHYStY], stC = arena[kHYStC];
    const YuvRgbCoef &k = kYuvRgb[o.standard];
    uint8_t *dst = static_cast<uint8_t *>(dstV);
    std::vector<uint16_t> work;
    std::vector<uint8_t> line(3 * static_cast<size_t>(dstW));
    uint8_t *Y = line.data(), *U = Y + dstW, *V = U + dstW;
    for (int i = 0; i < nRois; ++i) {
        const uint32_t *r = arena + arena[kHRecOff] + static_cast<size_t>(i) * recWords;
        const uint64_t off = (static_cast<uint64_t>(r[kYOffHi]) << 32) | r[kYOffLo];
        const uint64_t offC = (static_cast<uint64_t>(r[kYOffCHi]) << 32) | r[kYOffCLo];
        const int w = static_cast<int>(r[kYW]);
        const bool flip = r[kYFlags] & 1u;
        const uint32_t *xt = arena + r[kYXTab], *yt = arena + r[kYYTab];
        const uint32_t *xtC = arena + r[kYXTabC], *ytC = arena + r[kYYTabC];
        const RoiRect rc = rect_in(pad ? r + kRoiYuvFitExt : nullptr, dstW, dstH);
        uint8_t *canvas = dst + static_cast<size_t>(i) * dstRoiSt;
        if (pad) {
            const int px[4] = {pad[0], pad[1], pad[2], 255};
            pad_canvas(rc, dstW, dstH, px, o.channels, o.order, o.n, planeSt, dstSt, canvas);
        }
        for (int y = 0; y < rc.h; ++y) {
            component_row(xt, yt, rc.w, rc.h, LZ, yP + off, stY, 1, w, y, &work, Y);
            component_row(xtC, ytC, rc.w, rc.h, LZ, uP + offC, stC, nv12 ? 2 : 1, w / 2, y, &work, U);
            component_row(xtC, ytC, rc.w, rc.h, LZ, nv12 ? uP + offC + 1 : vP + offC, stC, nv12 ? 2 : 1, w / 2, y, &work, V);
            uint8_t *e = canvas + static_cast<size_t>(rc.y + y) * dstSt;
            for (int x = 0; x < rc.w; ++x) {
                int px[4] = {0, 0, 0, 255};
                yuv_to_rgb(k, Y[x], yuv_chroma_terms(k, U[x], V[x]), px[0], px[1], px[2]);
                store_pixel(px, o.channels, o.order, o.n, planeSt, e, rc.x + (flip ? rc.w - 1 - x : x));
            }
        }
    }
}

} // namespace

int roi_yuv_layout(RoiTableCache *cache, const RoiYuvSrc &s, size_t nRois, const RoiBox *rois, RoiLayout *out, int *bad)
{
    return layout_yuv(false, cache, s, nRois, rois, nullptr, out, bad);
}

int roi_yuv_fit_layout(RoiTableCache *cache, const RoiYuvSrc &s, size_t nRois, const RoiBox *rois, const RoiRect *rects,
                       RoiLayout *out, int *bad)
{
    return layout_yuv(true, cache, s, nRois, rois, rects, out, bad);
}

void roi_yuv_fill(const RoiTableCache &cache, const RoiLayout &l, const RoiYuvSrc &s, uint32_t *arena)
{
    fill_yuv(kRoiYuvMagic, cache, l, s, arena);
}

void roi_yuv_fit_fill(const RoiTableCache &cache, const RoiLayout &l, const RoiYuvSrc &s, uint32_t *arena)
{
    fill_yuv(kRoiYuvFitMagic, cache, l, s, arena);
}

void roi_yuv_walk(const uint32_t *arena, const uint8_t *y, const uint8_t *u, const uint8_t *v, const RoiYuvOut &o,
                  size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dst)
{
    walk_yuv(arena, y, u, v, o, dstSt, planeSt, dstRoiSt, dst, nullptr);
}

void roi_yuv_fit_walk(const uint32_t *arena, const uint8_t *y, const uint8_t *u, const uint8_t *v, const RoiYuvOut &o,
                      size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dst, const uint8_t pad[4])
{
    walk_yuv(arena, y, u, v, o, dstSt, planeSt, dstRoiSt, dst, pad);
}

bool fit_rect(int mode, uint64_t w, uint64_t h, uint64_t dstW, uint64_t dstH, RoiRect *out)
{
    if (mode < kFitStretch || mode > kFitLetterboxTopLeft || !w || !h || !dstW || !dstH || w > (1u << 24) || h > (1u << 24) ||
        dstW > (1u << 20) || dstH > (1u << 20))
        return false;
    uint64_t iw = dstW, ih = dstH;
    if (mode != kFitStretch) {
        if (w * dstH >= h * dstW)
            ih = std::max<uint64_t>(1, (h * dstW + w / 2) / w);
        else
            iw = std::max<uint64_t>(1, (w * dstH + h / 2) / h);
    }
    const bool centred = mode == kFitLetterbox;
    *out = RoiRect{centred ? static_cast<int>((dstW - iw) / 2) : 0, centred ? static_cast<int>((dstH - ih) / 2) : 0,
                   static_cast<int>(iw), static_cast<int>(ih)};
    return true;
}

} // namespace iqo_amd
