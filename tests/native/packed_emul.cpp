// Test-only scalar emulation of kernels_packed.hip packed_tile_kernel over the product's own host
// tables (libiqo_amd/csrc/plan.cpp build_tile_tables + build_packed_tables), so the packed index
// arithmetic -- staging of packed byte rows with PIXEL-wise edge replication, the vertical pass on
// byte rows with the per-channel byte selectors, the de-interleaved work-row layout, the
// per-channel horizontal windows and the store offsets -- is checked against the oracle on a
// machine without a GPU.  Tile by tile, as the kernel walks them.  Never part of the product.
#include "plan.hpp"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

using namespace iqo_amd;

namespace {

int exact_div(int n, int d)
{
    if (d == 0)
        return 0;
    return static_cast<int>(static_cast<int64_t>(n) / d);  // C truncation, as the kernel's result
}

}  // namespace

extern "C" {

// src / dst: packed rows of srcSt / dstSt bytes.  Returns 0 on success, 1 if the shape has no packed
// tile tables (packed_general_kernel), -1 on bad arguments.  geom (may be null): {CT, TH, NP, tiles in x,
// first column tile is a border tile, last column tile is a border tile}.
int packed_emul(int method, unsigned degree, int C, int srcW, int srcH, int dstW, int dstH, int pxScale,
                const uint8_t *src, int srcSt, uint8_t *dst, int dstSt, int *geom)
{
    Plan p;
    std::string err;
    if (C < 2 || C > 4 || !build_plan(static_cast<Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &p, &err))
        return -1;
    TileTables t;
    build_tile_tables(p, &t);
    PackedTables k;
    build_packed_tables(p, t, C, &k);
    if (!k.ok)
        return 1;
    const bool lz = method == kLanczos;
    const int nTx = (dstW + k.CT - 1) / k.CT, nTy = (dstH + k.TH - 1) / k.TH;
    if (geom) {
        geom[0] = k.CT;
        geom[1] = k.TH;
        geom[2] = t.NP;
        geom[3] = nTx;
        geom[4] = k.spans.front().border;
        geom[5] = k.spans.back().border;
    }
    if (packed_lds_bytes(p, t, k, k.TH) > 64 * 1024)
        return -1;
    std::vector<uint8_t> srcL(static_cast<size_t>(k.srcRows) * k.spitch);
    std::vector<uint16_t> work(static_cast<size_t>(k.TH) * C * k.pitchDw * 2);
    for (int ty = 0; ty < nTy; ++ty)
        for (int tx = 0; tx < nTx; ++tx) {
            const int y0 = ty * k.TH, nRows = std::min(k.TH, dstH - y0);
            const PackedSpan &sp = k.spans[static_cast<size_t>(tx)];
            const int rmin = t.rows[static_cast<size_t>(y0)].lo;
            const int nR = t.rows[static_cast<size_t>(y0 + nRows - 1)].hi - rmin + 1;
            if (nR > k.srcRows || sp.groups * 8 * C > k.spitch || sp.groups * 4 > k.pitchDw)
                return -1;
            // 0. stage: staged byte sb of a row is packed byte lo8 * C + sb inside the row, else
            //    channel sb % C of the clamped pixel
            std::fill(srcL.begin(), srcL.end(), 0xEE);
            for (int rr = 0; rr < nR; ++rr)
                for (int sb = 0; sb < sp.groups * 8 * C; ++sb) {
                    const int gb = sp.lo8 * C + sb;
                    int o;
                    if (gb >= 0 && gb < srcW * C)
                        o = gb;
                    else
                        o = std::min(std::max(sp.lo8 + sb / C, 0), srcW - 1) * C + sb % C;
                    srcL[static_cast<size_t>(rr) * k.spitch + sb] = src[static_cast<size_t>(rmin + rr) * srcSt + o];
                }
            // 1. vertical: task (row j, group g): pixel pair m of channel c = staged bytes
            //    2 m C + c and 2 m C + c + C of the group's 8 C bytes -> segment c of work row j
            for (int j = 0; j < nRows; ++j) {
                const TileRec &r = t.rows[static_cast<size_t>(y0 + j)];
                for (int g = 0; g < sp.groups; ++g)
                    for (int c = 0; c < C; ++c)
                        for (int m = 0; m < 4; ++m)
                            for (int h = 0; h < 2; ++h) {
                                const int b = 2 * m * C + c + h * C;
                                uint16_t acc = 0;
                                for (int i = 0; i < t.nYp; ++i) {
                                    const int row = std::min(std::max(r.start + i, r.lo), r.hi);
                                    const uint32_t cc = t.rowCoef[static_cast<size_t>(y0 + j) * t.nYp + i] & 0xffffu;
                                    const uint8_t px = srcL[static_cast<size_t>(row - rmin) * k.spitch + g * 8 * C + b];
                                    acc = static_cast<uint16_t>(acc + px * cc);
                                }
                                if (lz && r.deno != 0)
                                    acc = static_cast<uint16_t>(exact_div(static_cast<int16_t>(acc) * 64, r.deno));
                                work[(static_cast<size_t>(j * C + c) * k.pitchDw + 4 * g + m) * 2 + h] = acc;
                            }
            }
            // 2. horizontal: per channel on its segment; output byte x * C + c
            for (int j = 0; j < nRows; ++j)
                for (int x = tx * k.CT; x < std::min(dstW, (tx + 1) * k.CT); ++x) {
                    const TileCol &cl = t.cols[static_cast<size_t>(x)];
                    const int woff = (cl.a - sp.lo8) >> 1;  // dwords into the segment
                    if (woff < 0 || woff + t.NP > k.pitchDw)
                        return -1;
                    for (int c = 0; c < C; ++c) {
                        const uint16_t *w = &work[static_cast<size_t>(j * C + c) * k.pitchDw * 2];
                        int s = lz ? (1 << 19) : (1 << 22);
                        for (int pp = 0; pp < t.NP; ++pp) {
                            const uint32_t cf = t.colCoef[static_cast<size_t>(x) * t.NP + pp];
                            const uint16_t w0 = w[2 * (woff + pp)], w1 = w[2 * (woff + pp) + 1];
                            if (lz)
                                s += static_cast<int16_t>(w0) * static_cast<int16_t>(cf & 0xffffu) +
                                     static_cast<int16_t>(w1) * static_cast<int16_t>(cf >> 16);
                            else
                                s = static_cast<int>(static_cast<uint32_t>(s) + static_cast<uint32_t>(w0) * (cf & 0xffffu) +
                                                     static_cast<uint32_t>(w1) * (cf >> 16));
                        }
                        int v;
                        if (lz) {
                            v = cl.D != 0 ? static_cast<int16_t>(exact_div(s, cl.D)) : (s >> 20);
                            v = std::min(std::max(v, 0), 255);
                        } else {
                            v = static_cast<int>(std::min((static_cast<uint32_t>(s) >> 23) & 0xffffu, 255u));
                        }
                        dst[static_cast<size_t>(y0 + j) * dstSt + x * C + c] = static_cast<uint8_t>(v);
                    }
                }
        }
    return 0;
}

}  // extern "C"
