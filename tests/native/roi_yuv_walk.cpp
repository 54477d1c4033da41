// tests/native/roi_yuv_walk.cpp -- the YUV box arena of roi.hpp under AddressSanitizer + UBSan, stand-alone
// (TEST INFRASTRUCTURE ONLY; built and run by tests/test_roi_yuv_host.py with roi.cpp and plan.cpp).
//
// Lays out, fills and walks the 13-box call of tests/roi_yuv_cases.py and a call of 4097 tiny boxes, for
// Lanczos-3 and Area and both layouts.  Every plane and the arena are heap blocks of their exact sizes, so the
// sanitizer sees any byte the walk reads outside them; and every table and plane offset of the records is
// checked here against those sizes, with the extents the kernel reads.
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
    size_t elem = 1, planes = 1;
    if (norm) {
        o.n.dtype = 2;
        o.n.planes = 3;
        for (int p = 0; p < 3; ++p) {
            o.n.order[p] = 2 - p;
            o.n.scale[p] = 0.017f;
            o.n.bias[p] = -2.1f;
        }
        elem = 2;
        planes = 3;
    }
    const size_t dstSt = static_cast<size_t>(dstW) * (norm ? elem : 4), planeSt = dstSt * dstH;
    const size_t roiSt = planeSt * planes;
    std::vector<uint8_t> dst(roiSt * boxes.size());
    roi_yuv_walk(arena.data(), Y.data(), U.data(), nv12 ? nullptr : V.data(), o, dstSt, planeSt, roiSt, dst.data());
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
    if (fails) {
        std::printf("roi_yuv_walk: %d checks failed\n", fails);
        return 1;
    }
    std::printf("roi_yuv_walk ok\n");
    return 0;
}
