// TEST INFRASTRUCTURE ONLY (tests/native/asan.mk, tests/test_host_sanitizers.py): drives every
// host-side table builder of the product (libiqo_amd/csrc/plan.cpp) under AddressSanitizer and
// UBSan, over shapes read from stdin, one per line:
//   method degree srcW srcH dstW dstH pxScale
// For each shape: build_plan, the tile / walker tables, every exact-ratio builder (up2, d32, d31,
// a32, u23, l23), ryx and ryg, band_src_rows over random band cuts (full frame, single rows, the
// last row, random [r0, r1)), and the scalar emulations of the kernels that index those tables
// (tests/native/ratio_emul.cpp, tile_emul.cpp) on a random frame -- an emulated kernel reads
// the tables the way the kernel does (row records past the last row included), so a short table
// is an ASan report here instead of a stray device read.  For channels 2 .. 4 the packed tiling
// (build_packed_tables) and, on small shapes, its emulated kernel (packed_emul.cpp) run too.
// Before the shapes from stdin, a loop over degenerate Lanczos shapes (degree 1 .. 9, srcH 4 .. 40,
// dstH 1 .. 8, both pxScales): build_plan must fail exactly where the top border rows exceed dstH
// (the reference writes rows that do not exist there; restated below from the reference's
// formulas, not from plan.cpp) and build every table cleanly otherwise.  Prints one line per
// builder: the number of shapes it accepted.  Exit status != 0 on any sanitizer report
// (-fno-sanitize-recover) or on a wrong accept / reject.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <string>
#include <vector>

#include "plan.hpp"

extern "C" int ratio_emul(int kind, int method, unsigned degree, int srcW, int srcH, int dstW, int dstH, int pxScale,
                          const uint8_t *src, uint8_t *dst);
extern "C" int tile_emul(int method, unsigned degree, int srcW, int srcH, int dstW, int dstH, int pxScale,
                         const uint8_t *src, uint8_t *dst, int *np_out);

extern "C" int packed_emul(int method, unsigned degree, int C, int srcW, int srcH, int dstW, int dstH, int pxScale,
                           const uint8_t *src, int srcSt, uint8_t *dst, int dstSt, int *geom);

using namespace iqo_amd;

namespace {

// calcNumCoefsForLanczos (IQOLanczosResizerImpl_Generic.cpp:32-96) and the first row loop's bound
// (:392): false where that loop runs past dstH
bool lanczos_rows_defined(int degree, int srcH, int dstH, int pxScale)
{
    if (srcH == dstH)
        return true;
    int a = srcH, b = dstH;
    while (b) {
        const int r = a % b;
        a = b;
        b = r;
    }
    const int rs = srcH / a, rd = dstH / a;
    int taps = 2 * degree;
    if (rs > rd) {
        const int d2 = std::max(1, degree / pxScale);
        taps = 2 * ((d2 * rs + rd - 1) / rd);
    }
    const int64_t m = taps / 2;
    return ((m - 1) * dstH + srcH - 1) / srcH <= dstH;
}

// 0 on success; prints and returns != 0 on a wrong accept / reject
int degenerate_lanczos(std::map<std::string, int> &ok)
{
    for (int px = 1; px <= 2; ++px)
        for (int deg = 1; deg <= 9; ++deg)
            for (int sh = 4; sh <= 40; ++sh)
                for (int dh = 1; dh <= 8; ++dh) {
                    const int sw = 16 + (sh & 7), dw = 8 + (dh & 3);
                    Plan p;
                    std::string err;
                    const bool built = build_plan(kLanczos, static_cast<unsigned>(deg), sw, sh, dw, dh, px, &p, &err);
                    if (built != lanczos_rows_defined(deg, sh, dh, px)) {
                        std::fprintf(stderr, "lanczos-%d %dx%d -> %dx%d px %d: build_plan %d, rows defined %d\n", deg, sw, sh,
                                     dw, dh, px, built, !built);
                        return 6;
                    }
                    if (!built) {
                        if (err.empty())
                            return 7;
                        ++ok["degenerate_rejected"];
                        continue;
                    }
                    ++ok["degenerate_built"];
                    if (static_cast<int>(p.y.coord.size()) != dh || p.y.mainBegin > dh)
                        return 8;
                    TileTables t;
                    build_tile_tables(p, &t);
                    for (int C = 2; C <= 4; ++C) {
                        PackedTables k;
                        build_packed_tables(p, t, C, &k);
                    }
                    int s0 = -1, s1 = -1;
                    band_src_rows(p, 0, dh, &s0, &s1);
                    if (s0 < 0 || s1 > sh || s0 >= s1)
                        return 9;
                    std::vector<uint8_t> src(static_cast<size_t>(sw) * sh, 0x5a), dst(static_cast<size_t>(dw) * dh);
                    int np = 0;
                    tile_emul(kLanczos, static_cast<unsigned>(deg), sw, sh, dw, dh, px, src.data(), dst.data(), &np);
                }
    return 0;
}

}  // namespace

int main()
{
    std::map<std::string, int> ok;
    std::mt19937 rng(12345);
    if (const int rc = degenerate_lanczos(ok))
        return rc;
    int m, deg, sw, sh, dw, dh, px, n = 0;
    while (std::scanf("%d %d %d %d %d %d %d", &m, &deg, &sw, &sh, &dw, &dh, &px) == 7) {
        ++n;
        Plan p;
        std::string err;
        if (!build_plan(static_cast<Method>(m), static_cast<unsigned>(deg), sw, sh, dw, dh, px, &p, &err)) {
            ++ok["build_plan_rejected"];
            continue;
        }
        ++ok["build_plan"];
        TileTables t;
        build_tile_tables(p, &t);
        WalkTables w;
        if (t.ok) {
            ++ok["build_tile_tables"];
            tile_src_rows(p, t, t.TH);
            tile_lds_bytes(p, t, t.TH);
            build_walk_tables(p, t, &w);
            ok["build_walk_tables"] += w.ok;
        }
        Up2Tables u;
        build_up2(p, w, &u);
        ok["build_up2"] += u.ok;
        D32Tables d32;
        build_d32(p, w, &d32);
        ok["build_d32"] += d32.ok;
        D31Tables d31;
        build_d31(p, &d31);
        ok["build_d31"] += d31.ok;
        RyxTables ryx, ryg;
        build_ryx(p, &ryx);
        ok["build_ryx"] += ryx.ok;
        build_ryg(p, &ryg);
        ok["build_ryg"] += ryg.ok;
        U23Tables u23;
        build_u23(p, &u23);
        ok["build_u23"] += u23.ok;
        L23Tables l23;
        build_l23(p, &l23);
        ok["build_l23"] += l23.ok;
        A32Tables a32;
        build_a32(p, &a32);
        ok["build_a32"] += a32.ok;
        // band windows: whole frame, first / last row, one-row bands and random cuts
        std::vector<std::pair<int, int>> cuts = {{0, dh}, {0, 1}, {dh - 1, dh}, {dh / 2, dh / 2 + 1}};
        for (int k = 0; k < 24; ++k) {
            const int a = static_cast<int>(rng() % static_cast<unsigned>(dh)), b = static_cast<int>(rng() % static_cast<unsigned>(dh));
            cuts.push_back({std::min(a, b), std::max(a, b) + 1});
        }
        for (const auto &c : cuts) {
            int s0 = -1, s1 = -1;
            band_src_rows(p, c.first, c.second, &s0, &s1);
            if (s0 < 0 || s1 > sh || s0 >= s1) {
                std::fprintf(stderr, "band_src_rows(%d, %d) -> [%d, %d) outside [0, %d)\n", c.first, c.second, s0, s1, sh);
                return 4;
            }
        }
        ok["band_src_rows"] += 1;
        // the kernels' table reads, emulated (sizes kept to a few megapixels)
        if (static_cast<int64_t>(sw) * sh <= 9000000 && static_cast<int64_t>(dw) * dh <= 9000000) {
            std::vector<uint8_t> src(static_cast<size_t>(sw) * sh), dst(static_cast<size_t>(dw) * dh);
            for (auto &v : src)
                v = static_cast<uint8_t>(rng());
            static const char *names[] = {"emul_lanczos_d32", "emul_lanczos_up2", "emul_area_d32", "emul_lanczos_u23",
                                          "emul_linear_u23", "emul_lanczos_d31", "emul_ryx", "emul_linear_d2",
                                          "emul_linear_up2", "emul_ryg"};
            for (int kind = 0; kind <= 9; ++kind) {
                const int rc = ratio_emul(kind, m, static_cast<unsigned>(deg), sw, sh, dw, dh, px, src.data(), dst.data());
                if (rc < 0) {
                    std::fprintf(stderr, "ratio_emul kind %d rc %d on %d %d %d %d %d %d %d\n", kind, rc, m, deg, sw, sh, dw,
                                 dh, px);
                    return 5;
                }
                ok[names[kind]] += rc == 0;
            }
            int np = 0;
            ok["emul_tile"] += tile_emul(m, static_cast<unsigned>(deg), sw, sh, dw, dh, px, src.data(), dst.data(), &np) == 0;
        }
        // the packed tiling of channels 2 .. 4, and its emulated kernel on shapes of up to 1 megabyte
        for (int C = 2; C <= 4; ++C) {
            PackedTables k;
            build_packed_tables(p, t, C, &k);
            if (!k.ok)
                continue;
            ++ok["build_packed_tables"];
            if (static_cast<size_t>((dw + k.CT - 1) / k.CT) != k.spans.size() || k.TH < 2 ||
                packed_lds_bytes(p, t, k, k.TH) > 64 * 1024) {
                std::fprintf(stderr, "packed tables of %d %d %d %d %d %d %d C %d are inconsistent\n", m, deg, sw, sh, dw, dh,
                             px, C);
                return 10;
            }
            if (static_cast<int64_t>(sw) * sh * C > (1 << 20) || static_cast<int64_t>(dw) * dh * C > (1 << 20))
                continue;
            std::vector<uint8_t> src(static_cast<size_t>(sw) * sh * C), dst(static_cast<size_t>(dw) * dh * C);
            for (auto &v : src)
                v = static_cast<uint8_t>(rng());
            const int rc = packed_emul(m, static_cast<unsigned>(deg), C, sw, sh, dw, dh, px, src.data(), sw * C, dst.data(),
                                       dw * C, nullptr);
            if (rc != 0) {
                std::fprintf(stderr, "packed_emul rc %d on %d %d %d %d %d %d %d C %d\n", rc, m, deg, sw, sh, dw, dh, px, C);
                return 11;
            }
            ++ok["emul_packed"];
        }
    }
    std::printf("shapes %d\n", n);
    for (const auto &kv : ok)
        std::printf("%s %d\n", kv.first.c_str(), kv.second);
    return 0;
}
