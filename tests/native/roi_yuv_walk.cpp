// tests/native/roi_yuv_walk.cpp -- both box arenas of roi.hpp under AddressSanitizer + UBSan, stand-alone
// (TEST INFRASTRUCTURE ONLY; built and run by tests/test_roi_yuv_host.py with roi.cpp and plan.cpp).
//
// Lays out, fills and walks the 13-box call of tests/roi_yuv_cases.py and a call of 4097 tiny boxes, for
// Lanczos-3 and Area and both layouts; and, for the packed arena, the boxes of tests/roi_cases.py and a call of
// 4097 one-pixel boxes, for Lanczos-3 and Area and 1, 3 and 4 channels.  Every plane and the arena are heap
// blocks of their exact sizes, so the sanitizer sees any byte the walk reads outside them; and every table and
// plane offset of the records is checked here against those sizes, with the extents the kernel reads.
// Prints one line per case with the 64-bit FNV-1a of the arena's words and of the output's bytes (for comparing
// two builds of roi.cpp), then "roi_yuv_walk ok".
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

uint64_t fnv(const void *p, size_t n)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (size_t i = 0; i < n; ++i)
        h = (h ^ static_cast<const uint8_t *>(p)[i]) * 0x100000001b3ull;
    return h;
}

void sums(const char *what, Method m, int variant, size_t nBoxes, bool norm, const std::vector<uint32_t> &arena,
          const std::vector<uint8_t> &dst)
{
    std::printf("%s method %d variant %d boxes %zu norm %d: arena %016llx out %016llx\n", what, static_cast<int>(m), variant,
                nBoxes, static_cast<int>(norm), static_cast<unsigned long long>(fnv(arena.data(), arena.size() * 4)),
                static_cast<unsigned long long>(fnv(dst.data(), dst.size())));
}

// The float epilogue both runs use (fp16, planes in reverse order), and the destination's strides
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

// The packed arena: C interleaved bytes per pixel, frames fw x fh in one block
void run_packed(Method m, unsigned degree, int C, int dstW, int dstH, const std::vector<RoiBox> &boxes, int nFrames, int fw,
                int fh, bool norm)
{
    const size_t srcSt = static_cast<size_t>(fw) * C, frameSt = srcSt * fh;
    std::vector<uint8_t> src(nFrames * frameSt);
    uint64_t seed = 23;
    for (uint8_t &b : src)
        b = static_cast<uint8_t>(mix(seed) >> 56);
    RoiTableCache cache(m, degree, dstW, dstH);
    RoiLayout l;
    int bad = -2;
    const int st = roi_layout(&cache, C, boxes.size(), boxes.data(), nFrames, fw, fh, srcSt, frameSt, &l, &bad);
    CHECK(st == kRoiOk && bad == -1);
    if (st != kRoiOk)
        return;
    std::vector<uint32_t> arena(l.words);
    roi_fill(cache, l, fw, arena.data());
    CHECK(arena[kHMagic] == kRoiMagic && arena[kHWords] == l.words && arena[kHRois] == boxes.size());
    CHECK(arena[kHRecOff] + boxes.size() * kRoiRecWords <= l.words && arena[kHRowBytes] == srcSt);
    uint64_t groups = 0;
    for (size_t i = 0; i < boxes.size(); ++i) {
        const uint32_t *r = arena.data() + arena[kHRecOff] + i * kRoiRecWords;
        const RoiBox &b = boxes[i];
        // tables inside the arena, whole
        CHECK(r[kRXTab] + 4 <= l.words && r[kRYTab] + 4 <= l.words);
        const uint32_t *xt = arena.data() + r[kRXTab], *yt = arena.data() + r[kRYTab];
        CHECK(r[kRXTab] + 4 + static_cast<size_t>(dstW) * (2 + xt[0]) <= l.words);
        CHECK(r[kRYTab] + 4 + static_cast<size_t>(dstH) * (4 + yt[0] / 2) <= l.words);
        CHECK((xt[2] & 1) && !(xt[1] & 1) && !(yt[0] & 1) && xt[2] == r[kRPitch]);
        const int32_t *col = reinterpret_cast<const int32_t *>(xt + 4);
        for (int x = 0; x < dstW; ++x) {  // every window inside the work row
            CHECK(!(col[2 * x] & 1) && col[2 * x] + static_cast<int>(xt[1]) >= 0);
            CHECK(col[2 * x] + static_cast<int>(xt[1]) + 2 * static_cast<int>(xt[0]) <= 2 * static_cast<int>(xt[2]));
        }
        CHECK(static_cast<int>(xt[1]) + b.w <= 2 * static_cast<int>(xt[2]));
        const int32_t *row = reinterpret_cast<const int32_t *>(yt + 4);
        for (int y = 0; y < dstH; ++y)  // every clamped row inside the box
            CHECK(row[4 * y + 1] >= 0 && row[4 * y + 2] < b.h && row[4 * y + 1] <= row[4 * y + 2]);
        CHECK(r[kRRows] >= 1 && r[kRRows] <= static_cast<uint32_t>(kRoiMaxRows));
        CHECK(r[kRRows] * (static_cast<size_t>(C) * xt[2] + 2 * yt[0]) * 4 <= l.ldsBytes &&
              l.ldsBytes <= static_cast<size_t>(kRoiLdsMax));
        CHECK(r[kRFirst] == groups && r[kRGroups] == (dstH + r[kRRows] - 1) / r[kRRows]);
        groups += r[kRGroups];
        // the box's last byte inside the source block
        const uint64_t off = (static_cast<uint64_t>(r[kROffHi]) << 32) | r[kROffLo];
        CHECK(off + static_cast<uint64_t>(b.h - 1) * srcSt + static_cast<uint64_t>(b.w) * C <= src.size());
    }
    CHECK(groups == l.groups);
    RoiNorm n;
    size_t dstSt, planeSt, roiSt;
    norm_out(&n, norm ? C : 0, dstW, dstH, C, &dstSt, &planeSt, &roiSt);
    std::vector<uint8_t> dst(roiSt * boxes.size());
    roi_walk(arena.data(), src.data(), srcSt, dstSt, planeSt, roiSt, dst.data(), n);
    sums("packed", m, C, boxes.size(), norm, arena, dst);
}

void run(Method m, unsigned degree, int layout, int dstW, int dstH, const std::vector<RoiBox> &boxes, int nFrames, int fw,
         int fh, bool norm)
{
    const bool nv12 = layout == kRoiNv12;
    const size_t stY = static_cast<size_t>(fw), stC = nv12 ? fw : fw / 2;
    const size_t nY = stY * fh, nC = stC * (fh / 2);
    // one block per plane of ALL frames: frame stride nY for every plane pointer needs nC <= nY spacing, so the
    // chroma blocks are laid out with the Y frame stride too
    const size_t frameSt = nY;
    std::vector<uint8_t> Y(nFrames * frameSt), U((nFrames - 1) * frameSt + nC), V(nv12 ? 0 : (nFrames - 1) * frameSt + nC);
    uint64_t seed = 11;
    for (auto *p : {&Y, &U, &V})
        for (uint8_t &b : *p)
            b = static_cast<uint8_t>(mix(seed) >> 56);
    RoiYuvSrc src;
    src.layout = layout;
    src.nFrames = nFrames;
    src.frameW = fw;
    src.frameH = fh;
    src.stY = stY;
    src.stUV = stC;
    src.frameSt = frameSt;
    RoiTableCache cache(m, degree, dstW, dstH);
    RoiLayout l;
    int bad = -2;
    const int st = roi_yuv_layout(&cache, src, boxes.size(), boxes.data(), &l, &bad);
    CHECK(st == kRoiOk && bad == -1);
    if (st != kRoiOk)
        return;
    std::vector<uint32_t> arena(l.words);
    roi_yuv_fill(cache, l, src, arena.data());
    CHECK(arena[kHMagic] == kRoiYuvMagic && arena[kHWords] == l.words && arena[kHRois] == boxes.size());
    CHECK(arena[kHRecOff] + boxes.size() * kRoiYuvRecWords <= l.words);
    uint64_t groups = 0;
    for (size_t i = 0; i < boxes.size(); ++i) {
        const uint32_t *r = arena.data() + arena[kHRecOff] + i * kRoiYuvRecWords;
        const RoiBox &b = boxes[i];
        // tables inside the arena, whole
        const uint32_t xo[2] = {r[kYXTab], r[kYXTabC]}, yo[2] = {r[kYYTab], r[kYYTabC]};
        size_t rowWords = 0, tapWords = 0;
        for (int c = 0; c < 2; ++c) {
            CHECK(xo[c] + 4 <= l.words && yo[c] + 4 <= l.words);
            const uint32_t *xt = arena.data() + xo[c], *yt = arena.data() + yo[c];
            CHECK(xo[c] + 4 + static_cast<size_t>(dstW) * (2 + xt[0]) <= l.words);
            CHECK(yo[c] + 4 + static_cast<size_t>(dstH) * (4 + yt[0] / 2) <= l.words);
            CHECK((xt[2] & 1) && !(xt[1] & 1) && !(yt[0] & 1));
            CHECK(xt[2] == r[c ? kYPitchC : kYPitch]);
            const int n = c ? b.w / 2 : b.w, hgt = c ? b.h / 2 : b.h;
            const int32_t *col = reinterpret_cast<const int32_t *>(xt + 4);
            for (int x = 0; x < dstW; ++x) {  // every window inside the work row
                CHECK(!(col[2 * x] & 1) && col[2 * x] + static_cast<int>(xt[1]) >= 0);
                CHECK(col[2 * x] + static_cast<int>(xt[1]) + 2 * static_cast<int>(xt[0]) <= 2 * static_cast<int>(xt[2]));
            }
            CHECK(static_cast<int>(xt[1]) + n <= 2 * static_cast<int>(xt[2]));
            const int32_t *row = reinterpret_cast<const int32_t *>(yt + 4);
            for (int y = 0; y < dstH; ++y)  // every clamped row inside the box
                CHECK(row[4 * y + 1] >= 0 && row[4 * y + 2] < hgt && row[4 * y + 1] <= row[4 * y + 2]);
            rowWords += (c ? 2 : 1) * xt[2];
            tapWords += 2 * yt[0];
        }
        CHECK(r[kYRows] >= 1 && r[kYRows] <= static_cast<uint32_t>(kRoiMaxRows));
        CHECK(r[kYRows] * (rowWords + tapWords) * 4 <= l.ldsBytes && l.ldsBytes <= static_cast<size_t>(kRoiLdsMax));
        CHECK(r[kYFirst] == groups && r[kYGroups] == (dstH + r[kYRows] - 1) / r[kYRows]);
        groups += r[kYGroups];
        // the box's last byte inside each plane's block
        const uint64_t off = (static_cast<uint64_t>(r[kYOffHi]) << 32) | r[kYOffLo];
        const uint64_t offC = (static_cast<uint64_t>(r[kYOffCHi]) << 32) | r[kYOffCLo];
        CHECK(off + static_cast<uint64_t>(b.h - 1) * stY + b.w <= Y.size());
        CHECK(offC + static_cast<uint64_t>(b.h / 2 - 1) * stC + (nv12 ? b.w : b.w / 2) <= U.size());
    }
    CHECK(groups == l.groups);
    RoiYuvOut o;
    o.standard = 2;
    o.channels = 4;
    size_t dstSt, planeSt, roiSt;
    norm_out(&o.n, norm ? 3 : 0, dstW, dstH, 4, &dstSt, &planeSt, &roiSt);
    std::vector<uint8_t> dst(roiSt * boxes.size());
    roi_yuv_walk(arena.data(), Y.data(), U.data(), nv12 ? nullptr : V.data(), o, dstSt, planeSt, roiSt, dst.data());
    sums("yuv", m, layout, boxes.size(), norm, arena, dst);
}

} // namespace

int main()
{
    const std::vector<RoiBox> cases = {
        {0, 0, 0, 64, 48, 0},   {0, 2, 6, 32, 24, 0},    {1, 4, 10, 90, 62, 0},  {1, 6, 14, 40, 26, 0}, {2, 30, 20, 130, 100, 0},
        {2, 10, 40, 96, 48, 0}, {0, 40, 2, 90, 100, 0},  {0, 8, 58, 100, 62, 0}, {1, 4, 10, 90, 62, 1}, {2, 16, 12, 128, 96, 0},
        {0, 156, 116, 4, 4, 0}, {1, 100, 50, 14, 10, 0}, {1, 148, 60, 2, 20, 0}};
    std::vector<RoiBox> tiny;
    uint64_t s = 5;
    for (int i = 0; i < 4097; ++i) {
        RoiBox b;
        b.w = 4 + 2 * static_cast<int>(mix(s) % 7);   // 4 .. 16
        b.h = 4 + 2 * static_cast<int>(mix(s) % 5);   // 4 .. 12
        b.frame = static_cast<int>(mix(s) % 3);
        b.x = 2 * static_cast<int>(mix(s) % ((160 - b.w) / 2 + 1));
        b.y = 2 * static_cast<int>(mix(s) % ((120 - b.h) / 2 + 1));
        b.flags = static_cast<int>(mix(s) & 1);
        tiny.push_back(b);
    }
    for (int layout : {kRoiNv12, kRoiI420}) {
        run(kLanczos, 3, layout, 32, 24, cases, 3, 160, 120, false);
        run(kArea, 0, layout, 32, 24, cases, 3, 160, 120, true);
        run(kArea, 0, layout, 8, 6, tiny, 3, 160, 120, false);
    }
    // the packed arena: the boxes of tests/roi_cases.py (x through 0 .. 3 mod 4: every misalignment of the first byte)
    const std::vector<RoiBox> packed = {
        {0, 0, 0, 32, 24, 0},   {0, 1, 3, 64, 48, 0},      {1, 2, 5, 45, 31, 0},    {1, 3, 7, 20, 13, 0}, {2, 5, 11, 32, 61, 0},
        {2, 6, 40, 97, 24, 0},  {0, 7, 9, 7, 5, 0},        {2, 29, 20, 131, 100, 0}, {1, 100, 50, 33, 25, 0}, {1, 150, 60, 1, 10, 0},
        {0, 40, 2, 45, 50, 0},  {0, 9, 60, 50, 31, 0},     {1, 2, 5, 45, 31, 1},    {0, 158, 118, 2, 2, 0}};
    std::vector<RoiBox> dots;
    for (int i = 0; i < 4097; ++i) {
        RoiBox b;
        b.w = b.h = 1;
        b.frame = static_cast<int>(mix(s) % 3);
        b.x = static_cast<int>(mix(s) % 160);
        b.y = static_cast<int>(mix(s) % 120);
        b.flags = static_cast<int>(mix(s) & 1);
        dots.push_back(b);
    }
    for (int C : {1, 3, 4}) {
        for (bool norm : {false, true}) {
            run_packed(kLanczos, 3, C, 32, 24, packed, 3, 160, 120, norm);
            run_packed(kArea, 0, C, 32, 24, packed, 3, 160, 120, norm);
        }
        run_packed(kArea, 0, C, 8, 6, dots, 3, 160, 120, false);
    }
    if (fails) {
        std::printf("roi_yuv_walk: %d checks failed\n", fails);
        return 1;
    }
    std::printf("roi_yuv_walk ok\n");
    return 0;
}
