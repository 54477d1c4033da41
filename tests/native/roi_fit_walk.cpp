// tests/native/roi_fit_walk.cpp -- both fit arenas of roi.hpp under AddressSanitizer + UBSan, stand-alone
// (TEST INFRASTRUCTURE ONLY; built and run by tests/test_roi_fit_host.py with roi.cpp and plan.cpp).
//
// Lays out, fills and walks the case list of tests/roi_fit_cases.py (boxes into rectangles of a 48 x 40 canvas) and
// a call of 4097 tiny boxes into one-pixel rectangles of an 8 x 6 canvas, for Lanczos-3 and Area: the packed arena
// at 1, 3 and 4 channels, the YUV arena in both layouts, as bytes and as fp16 planes.  Every plane, the arena and
// the destination are heap blocks of their exact sizes, so the sanitizer sees any byte the walk touches outside
// them; every table offset and the fit words of the records are checked against those sizes; and every pad pixel of
// the U8 canvases is compared with the pad colour (pixels inside the rectangles and the fp16 outputs are pinned by
// tests/test_roi_fit_host.py against the oracle, not here).
// Prints "roi_fit_walk ok".
#include "roi.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace iqo_amd;

namespace {

int fails = 0;
#define CHECK(c)                                                        \
    do {                                                                \
        if (!(c)) {                                                     \
            std::printf("%s:%d: %s\n", __FILE__, __LINE__, #c);         \
            ++fails;                                                    \
        }                                                               \
    } while (0)

uint64_t mix(uint64_t &s)
{
    uint64_t z = (s += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

void noise(std::vector<uint8_t> *v, uint64_t seed)
{
    for (uint8_t &b : *v)
        b = static_cast<uint8_t>(mix(seed) >> 56);
}

const uint8_t kPad[4] = {37, 201, 90, 143};

// The float epilogue (fp16, planes in reverse order) or bytes, and the destination's strides
void norm_out(RoiNorm *n, int planes, int dstW, int dstH, size_t bytesPerPixel, size_t *dstSt, size_t *planeSt, size_t *roiSt)
{
    if (planes) {
        n->dtype = 2;
        n->planes = planes;
        for (int p = 0; p < planes; ++p) {
            n->order[p] = planes - 1 - p;
            n->scale[p] = 0.017f;
            n->bias[p] = -2.1f;
        }
    }
    *dstSt = static_cast<size_t>(dstW) * (planes ? 2 : bytesPerPixel);
    *planeSt = *dstSt * dstH;
    *roiSt = *planeSt * (planes ? planes : 1);
}

// The words both fit formats share, of record r (ext: its fit words) of a box going to rc; returns its workgroups
uint64_t check_fit_words(const uint32_t *ext, const RoiRect &rc, int dstH, uint32_t rows, uint32_t bands)
{
    CHECK(ext[kFIW] == static_cast<uint32_t>(rc.w) && ext[kFIH] == static_cast<uint32_t>(rc.h));
    CHECK(ext[kFOX] == static_cast<uint32_t>(rc.x) && ext[kFOY] == static_cast<uint32_t>(rc.y));
    CHECK(bands == (rc.h + rows - 1) / rows);
    CHECK(ext[kFPadAbove] == static_cast<uint32_t>((rc.y + kRoiPadRows - 1) / kRoiPadRows));
    CHECK(ext[kFPadBelow] == static_cast<uint32_t>((dstH - rc.y - rc.h + kRoiPadRows - 1) / kRoiPadRows));
    return static_cast<uint64_t>(ext[kFPadAbove]) + bands + ext[kFPadBelow];
}

// Table words inside the arena, by the rectangle's size
void check_tables(const std::vector<uint32_t> &arena, uint32_t xOff, uint32_t yOff, int iw, int ih, int n, int h)
{
    CHECK(xOff + 4 <= arena.size() && yOff + 4 <= arena.size());
    const uint32_t *xt = arena.data() + xOff, *yt = arena.data() + yOff;
    CHECK(xOff + 4 + static_cast<size_t>(iw) * (2 + xt[0]) <= arena.size());
    CHECK(yOff + 4 + static_cast<size_t>(ih) * (4 + yt[0] / 2) <= arena.size());
    const int32_t *col = reinterpret_cast<const int32_t *>(xt + 4);
    for (int x = 0; x < iw; ++x) {
        CHECK(!(col[2 * x] & 1) && col[2 * x] + static_cast<int>(xt[1]) >= 0);
        CHECK(col[2 * x] + static_cast<int>(xt[1]) + 2 * static_cast<int>(xt[0]) <= 2 * static_cast<int>(xt[2]));
    }
    CHECK(static_cast<int>(xt[1]) + n <= 2 * static_cast<int>(xt[2]));
    const int32_t *row = reinterpret_cast<const int32_t *>(yt + 4);
    for (int y = 0; y < ih; ++y)
        CHECK(row[4 * y + 1] >= 0 && row[4 * y + 2] < h && row[4 * y + 1] <= row[4 * y + 2]);
}

// Every pad byte of the U8 canvases is the pad colour's
void check_pad_u8(const std::vector<uint8_t> &dst, const std::vector<RoiRect> &rects, int dstW, int dstH, int C, const uint8_t *px)
{
    for (size_t i = 0; i < rects.size(); ++i)
        for (int y = 0; y < dstH; ++y)
            for (int x = 0; x < dstW; ++x) {
                const RoiRect &rc = rects[i];
                if (y >= rc.y && y < rc.y + rc.h && x >= rc.x && x < rc.x + rc.w)
                    continue;
                for (int c = 0; c < C; ++c)
                    CHECK(dst[((i * dstH + y) * dstW + x) * C + c] == px[c]);
            }
}

void run_packed(Method m, unsigned degree, int C, int dstW, int dstH, const std::vector<RoiBox> &boxes,
                const std::vector<RoiRect> &rects, int nFrames, int fw, int fh, bool norm)
{
    const size_t srcSt = static_cast<size_t>(fw) * C, frameSt = srcSt * fh;
    std::vector<uint8_t> src(nFrames * frameSt);
    noise(&src, 23);
    RoiTableCache cache(m, degree, dstW, dstH);
    RoiLayout l;
    int bad = -2;
    const int st = roi_fit_layout(&cache, C, boxes.size(), boxes.data(), rects.data(), nFrames, fw, fh, srcSt, frameSt, &l, &bad);
    CHECK(st == kRoiOk && bad == -1);
    if (st != kRoiOk)
        return;
    std::vector<uint32_t> arena(l.words);
    roi_fit_fill(cache, l, fw, arena.data());
    CHECK(arena[kHMagic] == kRoiFitMagic && arena[kHWords] == l.words && arena[kHRois] == boxes.size());
    CHECK(arena[kHRecOff] + boxes.size() * kRoiFitRecWords <= l.words && arena[kHRowBytes] == srcSt);
    CHECK(arena[kHDstW] == static_cast<uint32_t>(dstW) && arena[kHDstH] == static_cast<uint32_t>(dstH));
    uint64_t groups = 0;
    for (size_t i = 0; i < boxes.size(); ++i) {
        const uint32_t *r = arena.data() + arena[kHRecOff] + i * kRoiFitRecWords;
        check_tables(arena, r[kRXTab], r[kRYTab], rects[i].w, rects[i].h, boxes[i].w, boxes[i].h);
        const uint32_t *xt = arena.data() + r[kRXTab], *yt = arena.data() + r[kRYTab];
        CHECK(xt[2] == r[kRPitch] && r[kRRows] >= 1 && r[kRRows] <= static_cast<uint32_t>(kRoiMaxRows));
        CHECK(r[kRRows] * (static_cast<size_t>(C) * xt[2] + 2 * yt[0]) * 4 <= l.ldsBytes &&
              l.ldsBytes <= static_cast<size_t>(kRoiLdsMax));
        CHECK(r[kRFirst] == groups);
        groups += check_fit_words(r + kRoiFitExt, rects[i], dstH, r[kRRows], r[kRGroups]);
    }
    CHECK(groups == l.groups);
    RoiNorm n;
    size_t dstSt, planeSt, roiSt;
    norm_out(&n, norm ? C : 0, dstW, dstH, C, &dstSt, &planeSt, &roiSt);
    std::vector<uint8_t> dst(roiSt * boxes.size(), 0xA5);
    roi_fit_walk(arena.data(), src.data(), srcSt, dstSt, planeSt, roiSt, dst.data(), n, kPad);
    if (!norm)
        check_pad_u8(dst, rects, dstW, dstH, C, kPad);
}

void run_yuv(Method m, unsigned degree, int layout, int dstW, int dstH, const std::vector<RoiBox> &boxes,
             const std::vector<RoiRect> &rects, int nFrames, int fw, int fh, bool norm)
{
    const bool nv12 = layout == kRoiNv12;
    // one heap block per plane, frames frameSt apart in each (the chroma blocks: as long as the Y block needs)
    RoiYuvSrc s;
    s.layout = layout;
    s.nFrames = nFrames;
    s.frameW = fw;
    s.frameH = fh;
    s.stY = fw;
    s.stUV = nv12 ? fw : fw / 2;
    s.frameSt = static_cast<size_t>(fw) * fh;
    std::vector<uint8_t> Y(nFrames * s.frameSt), U((nFrames - 1) * s.frameSt + s.stUV * (fh / 2)), V(nv12 ? 0 : U.size());
    noise(&Y, 5);
    noise(&U, 6);
    noise(&V, 7);
    RoiTableCache cache(m, degree, dstW, dstH);
    RoiLayout l;
    int bad = -2;
    const int st = roi_yuv_fit_layout(&cache, s, boxes.size(), boxes.data(), rects.data(), &l, &bad);
    CHECK(st == kRoiOk && bad == -1);
    if (st != kRoiOk)
        return;
    std::vector<uint32_t> arena(l.words);
    roi_yuv_fit_fill(cache, l, s, arena.data());
    CHECK(arena[kHMagic] == kRoiYuvFitMagic && arena[kHWords] == l.words && arena[kHRois] == boxes.size());
    CHECK(arena[kHRecOff] + boxes.size() * kRoiYuvFitRecWords <= l.words);
    uint64_t groups = 0;
    for (size_t i = 0; i < boxes.size(); ++i) {
        const uint32_t *r = arena.data() + arena[kHRecOff] + i * kRoiYuvFitRecWords;
        check_tables(arena, r[kYXTab], r[kYYTab], rects[i].w, rects[i].h, boxes[i].w, boxes[i].h);
        check_tables(arena, r[kYXTabC], r[kYYTabC], rects[i].w, rects[i].h, boxes[i].w / 2, boxes[i].h / 2);
        CHECK(r[kYRows] >= 1 && r[kYRows] <= static_cast<uint32_t>(kRoiMaxRows) && l.ldsBytes <= static_cast<size_t>(kRoiLdsMax));
        CHECK(r[kYFirst] == groups);
        groups += check_fit_words(r + kRoiYuvFitExt, rects[i], dstH, r[kYRows], r[kYGroups]);
    }
    CHECK(groups == l.groups);
    RoiYuvOut o;
    o.standard = 1;
    o.channels = norm ? 3 : 4;
    o.order[0] = 2, o.order[1] = 1, o.order[2] = 0, o.order[3] = 3;
    size_t dstSt, planeSt, roiSt;
    norm_out(&o.n, norm ? 3 : 0, dstW, dstH, 4, &dstSt, &planeSt, &roiSt);
    std::vector<uint8_t> dst(roiSt * boxes.size(), 0xA5);
    roi_yuv_fit_walk(arena.data(), Y.data(), U.data(), nv12 ? nullptr : V.data(), o, dstSt, planeSt, roiSt, dst.data(), kPad);
    if (!norm) {
        const uint8_t px[4] = {kPad[2], kPad[1], kPad[0], 255};
        check_pad_u8(dst, rects, dstW, dstH, 4, px);
    }
}

} // namespace

int main()
{
    // tests/roi_fit_cases.py CASES and YUV_CASES (every method takes these of them)
    const std::vector<RoiBox> boxes = {{0, 1, 3, 64, 48, 0},  {0, 2, 5, 64, 36, 0},  {1, 3, 7, 33, 60, 0},  {1, 2, 5, 45, 31, 0},
                                       {1, 2, 5, 45, 31, 1},  {2, 5, 11, 32, 24, 0}, {1, 3, 7, 20, 13, 0},  {2, 29, 20, 12, 1, 0},
                                       {2, 29, 20, 12, 20, 0}, {2, 29, 20, 30, 1, 0}, {0, 40, 2, 45, 50, 0}, {0, 9, 60, 45, 40, 0}};
    const std::vector<RoiBox> even = {{0, 0, 2, 64, 48, 0},  {0, 2, 6, 64, 36, 0},  {1, 4, 8, 34, 60, 0},  {1, 2, 6, 46, 32, 0},
                                      {1, 2, 6, 46, 32, 1},  {2, 6, 12, 32, 24, 0}, {1, 4, 8, 20, 14, 0},  {2, 30, 20, 12, 20, 0},
                                      {2, 30, 20, 12, 20, 0}, {2, 30, 20, 30, 20, 0}, {0, 40, 2, 46, 50, 0}, {0, 10, 60, 46, 40, 0}};
    const std::vector<RoiRect> rects = {{0, 0, 48, 40}, {0, 6, 48, 27}, {13, 0, 22, 40}, {5, 7, 31, 19}, {5, 7, 31, 19}, {8, 8, 32, 24},
                                        {4, 7, 40, 26}, {47, 39, 1, 1}, {0, 0, 1, 40},   {0, 0, 48, 1},  {2, 3, 20, 30}, {10, 0, 31, 33}};
    std::vector<RoiBox> evenLz;
    std::vector<RoiRect> rectsLz;
    for (size_t i = 0; i < even.size(); ++i)
        if (rects[i].h > 1) {
            evenLz.push_back(even[i]);
            rectsLz.push_back(rects[i]);
        }
    // 4097 tiny boxes into one-pixel rectangles that walk an 8 x 6 canvas
    std::vector<RoiBox> dots, dotsEven;
    std::vector<RoiRect> dotRects;
    for (int i = 0; i < 4097; ++i) {
        dots.push_back(RoiBox{i % 3, i % 150, (i / 7) % 110, 1 + i % 5, 1, i & 1});  // (one row: Lanczos takes no other to one)
        dotsEven.push_back(RoiBox{i % 3, 2 * (i % 75), 2 * ((i / 7) % 55), 2 + 2 * (i % 3), 2 + 2 * (i % 2), i & 1});
        dotRects.push_back(RoiRect{i % 8, (i / 8) % 6, 1, 1});
    }
    for (Method m : {kLanczos, kArea})
        for (int norm = 0; norm < 2; ++norm) {
            for (int C : {1, 3, 4}) {
                run_packed(m, 3, C, 48, 40, boxes, rects, 3, 160, 120, norm != 0);
                run_packed(m, 3, C, 8, 6, dots, dotRects, 3, 160, 120, norm != 0);
            }
            for (int layout : {kRoiNv12, kRoiI420}) {
                // (Lanczos has no defined single row from an even height: without those rectangles, and Area alone
                // takes the one-pixel rectangles)
                run_yuv(m, 3, layout, 48, 40, m == kLanczos ? evenLz : even, m == kLanczos ? rectsLz : rects, 3, 160, 120, norm != 0);
                if (m == kArea)
                    run_yuv(m, 3, layout, 8, 6, dotsEven, dotRects, 3, 160, 120, norm != 0);
            }
        }
    // a rectangle outside the canvas names its box
    {
        RoiTableCache cache(kArea, 0, 48, 40);
        RoiLayout l;
        int bad = -2;
        std::vector<RoiRect> r2(rects.begin(), rects.begin() + 3);
        r2[2] = RoiRect{40, 0, 9, 40};
        CHECK(roi_fit_layout(&cache, 1, 3, boxes.data(), r2.data(), 3, 160, 120, 160, 160 * 120, &l, &bad) == kRoiInvalid && bad == 2);
    }
    if (fails) {
        std::printf("roi_fit_walk: %d checks failed\n", fails);
        return 1;
    }
    std::printf("roi_fit_walk ok\n");
    return 0;
}
