// abi.hip -- implementation of include/iqo_hip.h (the extern "C" boundary).
//
// A plan owns: the host Plan (tables + index maps, plan.cpp), their device copies, the chunk
// table of the general kernel, and (lazily) a stream
// plus device staging buffers for the host-pointer entry point.  There is no CPU fallback:
// any HIP failure is returned as a negative status.
#include "iqo_hip.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <condition_variable>
#include <mutex>
#include <new>
#include <thread>
#include <string>
#include <vector>

#include "kernels.hpp"
#include "plan.hpp"
#include "roi.hpp"

using iqo_amd::AxisPlan;
using iqo_amd::CoordInfo;
using iqo_amd::Plan;

struct iqo_hip_plan;
namespace {
void reset_options(iqo_hip_plan *h);
}

struct iqo_hip_plan {
    iqo_hip_plan() { reset_options(this); }  // the option members below: defaults from kOptions
    Plan p;
    int device = 0;
    // plan-cache key (make_plan): identical requests reuse a destroyed plan's tables
    int keyMethod = 0;
    unsigned keyDegree = 0;
    size_t keyDims[5] = {0, 0, 0, 0, 0};
    // bytes per pixel: 1 = planar (every kernel family), 2 .. 4 = packed interleaved channels
    // (iqo_hip_plan_packed: packed_tile_kernel / packed_general_kernel only).  Part of the cache key.
    int channels = 1;
    iqo_amd::PackedTables pk;
    int4 *dPSpans = nullptr;
    // Device tables (general / tile / walker / ratio-Y kernels) are staged into one host blob at
    // plan creation and uploaded by ONE allocation and copy the first time a launch needs them:
    // the specialised kernels take their coefficients as kernel arguments, so a plan that only
    // ever runs them costs no device allocation (the reference benchmark constructs its resizers
    // inside the timed loop, benchmark/benchmark.cpp:206-229).
    std::vector<uint8_t> blob;
    std::vector<std::pair<void **, size_t>> blobPtrs;  // member pointer, byte offset in the blob
    uint8_t *dBlob = nullptr;
    bool tablesUp = false;
    std::mutex tablesMu;
    int4 *dX = nullptr, *dY = nullptr, *dChunks = nullptr;
    int *dTabX = nullptr, *dTabY = nullptr;
    int nChunks = 0, ldsInts = 0;
    // Options (iqo_hip_plan_set_option): what each one does, its accepted values and its default are
    // its row of kOptions below; reset_options sets every one of them.
    int forceGeneral, bands, hostStage, tail, rounds, ryxSplit, ryxAdj, ryxCpt, ryxUc, rygCpt, stack, prefetch,
        streamVariant, lanes, ratioPrefetch, chunkFrames;
    int useTile, useWalk, useUp2, useD32, useD31, useA32, useU23, useL23, useRyx, useRyg, useRyu, useRyuRun;
    int debugFlags;  // variant builds only (timing experiments); 0 otherwise
#ifdef IQO_VARIANT_DEBUG
    uint64_t traceAddr;  // variant builds: workgroup timeline buffer of the block-shared streamer
#endif
    // separable tile kernel (shapes without a specialised kernel; plan option "tile" = 0 turns
    // it off, leaving general_kernel)
    iqo_amd::TileTables tt;
    int tileTH0 = 0, tileSrcRows0 = 0;  // the auto tile height (option "tile_rows" changes it; reset_options restores it)
    int4 *dTRows = nullptr, *dTSpans = nullptr;
    int2 *dTCols = nullptr;
    uint2 *dTRowTap = nullptr;
    uint32_t *dTColCoef = nullptr;
    int32_t *dTColA = nullptr;
    int tileNQp = 0;
    // general-ratio wave walker (plan.hpp WalkTables; option "walk" = 0 keeps tile_kernel)
    iqo_amd::WalkTables wt;
    // exact 2x Lanczos upscale kernel, every row and column in-kernel (option "up2" = 0: walker only)
    iqo_amd::Up2Tables ut;
    // exact 3:2 Lanczos-3 downscale kernel on the main rows (option "d32" = 0: walker only)
    iqo_amd::D32Tables dt;
    iqo_amd::D31Tables t31;
    iqo_amd::RyxTables ryx;
    uint32_t *dRyxRowCoef = nullptr, *dRyxColCoef = nullptr;
    int4 *dRyxCols = nullptr;
    int4 *dRyxRowRec = nullptr;  // general-row tables (ryx.general: the ryg kernel, kernels.hpp RygDev)
    // general upscale rows by window position (kernels.hip ryu_kernel): records, first window start
    int4 *dRyuPos = nullptr;
    int ryuBase = 0;
    bool hasRyu = false;  // the table exists (every window position holds 1 or 2 rows)
    uint32_t *dRyuRun = nullptr;  // run-mode column table (plan.hpp colRun), when it exists
    // exact 2:3 Linear upscale kernel (option "l23" = 0: walker only)
    iqo_amd::L23Tables lt;
    // exact 2:3 Lanczos-3 upscale kernel (option "u23" = 0: walker only)
    iqo_amd::U23Tables vt;
    // exact 3:2 Area downscale kernel (option "a32" = 0: walker only)
    iqo_amd::A32Tables at;
    int4 *dWSpans = nullptr;
    int4 *dWSegs = nullptr;
    uint32_t *dWRowTap = nullptr;
    int4 *dWRows = nullptr;
};

namespace {

constexpr int kChunkOut = 256;     // outputs per general-kernel chunk (= workgroup size)
constexpr int kChunkLds = 8192;    // max work-row ints per chunk (32 KiB LDS)

class DeviceGuard {  // restore the caller's current device
public:
    explicit DeviceGuard(int dev)
    {
        ok_ = hipGetDevice(&prev_) == hipSuccess && hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceGuard()
    {
        if (ok_)
            (void)hipSetDevice(prev_);
    }
    bool ok() const { return ok_; }

private:
    int prev_ = 0;
    bool ok_ = false;
};

// ---- host-pointer path (iqo_hip_resize): staging pool
//
// Device staging frames, pinned host staging, three streams (H2D, kernels, D2H) and per-band
// events, pooled per device for the whole process: constructing a resizer stays cheap (the
// reference benchmark constructs one per call, benchmark.cpp:215-226), and one staging set is
// borrowed per call, so distinct plans can run concurrently from different threads.  The pool
// is never torn down (the HIP runtime may already be gone at static destruction).
constexpr int kHostBands = 8;      // output-row bands of one plane in the host-pointer pipeline
constexpr int kHostBandRows = 64;  // ... each at least this tall
constexpr int kHostChunks = 16;    // (plane, band) chunks of one call: events per staging set
constexpr size_t kHostPipeMinBytes = size_t(4) << 20;  // smaller frames: one band (API latency dominates)

struct HostStage {
    int device = 0;
    hipStream_t sIn = nullptr, sK = nullptr, sOut = nullptr, sIn2 = nullptr;
    hipEvent_t evIn[kHostChunks] = {}, evK[kHostChunks] = {}, evOut[kHostChunks] = {};
    uint8_t *dSrc = nullptr, *dDst = nullptr, *hSrc = nullptr, *hDst = nullptr;
    size_t dSrcCap = 0, dDstCap = 0, hSrcCap = 0, hDstCap = 0;
};

std::mutex g_stageMu;
std::vector<HostStage *> g_stagePool;

void destroy_stage(HostStage *st)
{
    for (int b = 0; b < kHostChunks; ++b) {
        if (st->evIn[b])
            (void)hipEventDestroy(st->evIn[b]);
        if (st->evK[b])
            (void)hipEventDestroy(st->evK[b]);
        if (st->evOut[b])
            (void)hipEventDestroy(st->evOut[b]);
    }
    if (st->sIn)
        (void)hipStreamDestroy(st->sIn);
    if (st->sK)
        (void)hipStreamDestroy(st->sK);
    if (st->sOut)
        (void)hipStreamDestroy(st->sOut);
    if (st->sIn2)
        (void)hipStreamDestroy(st->sIn2);
    (void)hipFree(st->dSrc);
    (void)hipFree(st->dDst);
    (void)hipHostFree(st->hSrc);
    (void)hipHostFree(st->hDst);
    delete st;
}

HostStage *acquire_stage(int device)
{
    {
        std::lock_guard<std::mutex> g(g_stageMu);
        for (size_t i = 0; i < g_stagePool.size(); ++i)
            if (g_stagePool[i]->device == device) {
                HostStage *st = g_stagePool[i];
                g_stagePool.erase(g_stagePool.begin() + static_cast<std::ptrdiff_t>(i));
                return st;
            }
    }
    HostStage *st = new (std::nothrow) HostStage();
    if (!st)
        return nullptr;
    st->device = device;
    bool ok = hipStreamCreateWithFlags(&st->sIn, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&st->sK, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&st->sOut, hipStreamNonBlocking) == hipSuccess &&
              hipStreamCreateWithFlags(&st->sIn2, hipStreamNonBlocking) == hipSuccess;
    for (int b = 0; ok && b < kHostChunks; ++b)
        ok = hipEventCreateWithFlags(&st->evIn[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&st->evK[b], hipEventDisableTiming) == hipSuccess &&
             hipEventCreateWithFlags(&st->evOut[b], hipEventDisableTiming) == hipSuccess;
    if (!ok) {
        // a partly built set is destroyed, never pooled: the next call builds a fresh one
        destroy_stage(st);
        return nullptr;
    }
    return st;
}

void release_stage(HostStage *st)
{
    std::lock_guard<std::mutex> g(g_stageMu);
    g_stagePool.push_back(st);
}

int grow_device(uint8_t **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap)
        return IQO_HIP_OK;
    (void)hipFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipMalloc(reinterpret_cast<void **>(p), bytes) != hipSuccess)
        return IQO_HIP_ENOMEM;
    *cap = bytes;
    return IQO_HIP_OK;
}

int grow_pinned(uint8_t **p, size_t *cap, size_t bytes)
{
    if (bytes <= *cap)
        return IQO_HIP_OK;
    (void)hipHostFree(*p);
    *p = nullptr;
    *cap = 0;
    if (hipHostMalloc(reinterpret_cast<void **>(p), bytes, hipHostMallocDefault) != hipSuccess)
        return IQO_HIP_ENOMEM;
    *cap = bytes;
    return IQO_HIP_OK;
}

// Host memory the DMA engines reach directly: hipHostMalloc'd or hipHostRegister'ed.
bool is_pinned_host(const void *p)
{
    hipPointerAttribute_t a{};
    if (hipPointerGetAttributes(&a, p) != hipSuccess) {
        (void)hipGetLastError();  // pageable memory reports an error here; clear it
        return false;
    }
    return a.type == hipMemoryTypeHost;
}

void copy_rows(uint8_t *dst, size_t dstSt, const uint8_t *src, size_t srcSt, size_t w, size_t rows)
{
    if (dstSt == w && srcSt == w) {
        std::memcpy(dst, src, w * rows);
        return;
    }
    for (size_t r = 0; r < rows; ++r)
        std::memcpy(dst + r * dstSt, src + r * srcSt, w);
}

// Row copies between pageable user memory and the pinned staging of the host-pointer path, split
// over a small process-wide thread pool: one thread's memcpy (~10 GB/s) is slower than the PCIe
// link the staged rows then cross.  Created on first use and never torn down (as the staging
// pool); one parallel copy at a time -- a caller that finds the pool busy copies alone.
struct RowCopy {
    uint8_t *dst;
    size_t dstSt;
    const uint8_t *src;
    size_t srcSt, w, rows;
};

class CopyPool {
public:
    static CopyPool &instance()
    {
        static CopyPool *p = new CopyPool();
        return *p;
    }
    // up to kMaxJobs row copies (e.g. the three I420 planes) as ONE parallel job: the rows of all
    // of them are split evenly over the workers, so a call pays one wake-up, not one per plane
    static constexpr int kMaxJobs = 3;
    void copy(const RowCopy *jobs, int n)
    {
        size_t bytes = 0, rows = 0;
        for (int j = 0; j < n; ++j) {
            bytes += jobs[j].w * jobs[j].rows;
            rows += jobs[j].rows;
        }
        std::unique_lock<std::mutex> use(useMu_, std::try_to_lock);
        // below ~256 KiB one thread's memcpy beats the wake-up of the pool
        if (!use.owns_lock() || workers_.empty() || n > kMaxJobs || bytes < (size_t(256) << 10) || rows < 32) {
            for (int j = 0; j < n; ++j)
                copy_rows(jobs[j].dst, jobs[j].dstSt, jobs[j].src, jobs[j].srcSt, jobs[j].w, jobs[j].rows);
            return;
        }
        std::unique_lock<std::mutex> g(mu_);
        nJobs_ = n;
        totalRows_ = rows;
        for (int j = 0; j < n; ++j)
            jobs_[j] = jobs[j];
        parts_ = static_cast<int>(workers_.size()) + 1;
        next_ = 0;
        remaining_ = parts_;
        ++gen_;
        cv_.notify_all();
        while (next_ < parts_) {  // the caller takes parts too
            const int part = next_++;
            g.unlock();
            run_part(part);
            g.lock();
            --remaining_;
        }
        done_.wait(g, [&] { return remaining_ == 0; });
    }

private:
    CopyPool()
    {
        const unsigned hw = std::thread::hardware_concurrency();
        const unsigned n = hw >= 4 ? std::min(7u, hw / 2) : 0u;
        for (unsigned i = 0; i < n; ++i)
            workers_.emplace_back([this] { work(); });
        for (auto &t : workers_)
            t.detach();
    }
    // part k copies global rows [R k / parts, R (k+1) / parts) of the jobs' rows laid end to end
    void run_part(int part) const
    {
        size_t r0 = totalRows_ * static_cast<size_t>(part) / static_cast<size_t>(parts_);
        const size_t r1 = totalRows_ * static_cast<size_t>(part + 1) / static_cast<size_t>(parts_);
        size_t base = 0;
        for (int j = 0; j < nJobs_ && r0 < r1; ++j) {
            const RowCopy &c = jobs_[j];
            const size_t a = std::max(r0, base), b = std::min(r1, base + c.rows);
            if (a < b) {
                copy_rows(c.dst + (a - base) * c.dstSt, c.dstSt, c.src + (a - base) * c.srcSt, c.srcSt, c.w, b - a);
                r0 = b;
            }
            base += c.rows;
        }
    }
    void work()
    {
        unsigned long seen = 0;
        std::unique_lock<std::mutex> g(mu_);
        for (;;) {
            cv_.wait(g, [&] { return gen_ != seen; });
            seen = gen_;
            while (next_ < parts_) {
                const int part = next_++;
                g.unlock();
                run_part(part);
                g.lock();
                if (--remaining_ == 0)
                    done_.notify_all();
            }
        }
    }
    std::mutex useMu_, mu_;
    std::condition_variable cv_, done_;
    std::vector<std::thread> workers_;
    RowCopy jobs_[kMaxJobs]{};
    int nJobs_ = 0;
    size_t totalRows_ = 0;
    int parts_ = 0, next_ = 0, remaining_ = 0;
    unsigned long gen_ = 0;
};

void copy_rows_par(uint8_t *dst, size_t dstSt, const uint8_t *src, size_t srcSt, size_t w, size_t rows)
{
    const RowCopy c{dst, dstSt, src, srcSt, w, rows};
    CopyPool::instance().copy(&c, 1);
}

void copy_planes_par(const RowCopy *jobs, int n) { CopyPool::instance().copy(jobs, n); }

bool is_gfx950(int dev)
{
    // the device's architecture cannot change in a process: queried once per device (the
    // property query costs more than building a small plan's tables)
    static std::mutex mu;
    static std::vector<signed char> known;  // -1 unknown, 0 / 1
    std::lock_guard<std::mutex> g(mu);
    if (dev < 0)
        return false;
    if (static_cast<size_t>(dev) >= known.size())
        known.resize(static_cast<size_t>(dev) + 1, -1);
    if (known[static_cast<size_t>(dev)] < 0) {
        hipDeviceProp_t prop;
        if (hipGetDeviceProperties(&prop, dev) != hipSuccess)
            return false;
        known[static_cast<size_t>(dev)] = std::strncmp(prop.gcnArchName, "gfx950", 6) == 0 ? 1 : 0;
    }
    return known[static_cast<size_t>(dev)] == 1;
}

template <typename T>
void upload(iqo_hip_plan *h, T **dptr, const T *src, size_t n)
{
    // stage into the plan's blob (256-B aligned sections); ensure_tables uploads it on first use
    const size_t off = (h->blob.size() + 255) & ~static_cast<size_t>(255);
    const size_t bytes = std::max<size_t>(n, 1) * sizeof(T);
    h->blob.resize(off + bytes, 0);
    if (src && n)
        std::memcpy(h->blob.data() + off, src, n * sizeof(T));
    h->blobPtrs.emplace_back(reinterpret_cast<void **>(dptr), off);
    *dptr = nullptr;
}

// One allocation + one copy of every staged table, then the table pointers point into it.
int ensure_tables(iqo_hip_plan *h)
{
    std::lock_guard<std::mutex> lock(h->tablesMu);
    if (h->tablesUp)
        return IQO_HIP_OK;
    if (!h->blob.empty()) {
        if (hipMalloc(reinterpret_cast<void **>(&h->dBlob), h->blob.size()) != hipSuccess)
            return IQO_HIP_ENOMEM;
        if (hipMemcpy(h->dBlob, h->blob.data(), h->blob.size(), hipMemcpyHostToDevice) != hipSuccess)
            return IQO_HIP_EHIP;
    }
    for (const auto &pr : h->blobPtrs)
        *pr.first = h->dBlob + pr.second;
    h->tablesUp = true;
    return IQO_HIP_OK;
}

// Source-column interval [a, b) that output column x reads (general kernel).
void column_span(const Plan &p, int x, int *a, int *b)
{
    const CoordInfo &c = p.x.coord[static_cast<size_t>(x)];
    const int W = p.srcW;
    if (c.kind == iqo_amd::kIdentity) {
        *a = c.srcO;
        *b = c.srcO + 1;
    } else if (p.method == iqo_amd::kLinear && c.kind != iqo_amd::kMain) {
        *a = c.kind == iqo_amd::kBorderLo ? 0 : W - 1;
        *b = *a + 1;
    } else if (p.method == iqo_amd::kLinear) {
        *a = std::max(0, std::min(c.srcO, W - 1));
        *b = std::max(0, std::min(c.srcO + 1, W - 1)) + 1;
    } else {
        *a = std::max(0, std::min(c.srcO, W - 1));
        *b = std::max(*a + 1, std::min(c.srcO + p.x.taps, W));
    }
}

int build_chunks(const Plan &p, std::vector<int4> *chunks, int *ldsInts)
{
    chunks->clear();
    *ldsInts = 1;
    int x = 0;
    while (x < p.dstW) {
        int lo, hi;
        column_span(p, x, &lo, &hi);
        if (hi - lo > kChunkLds)
            return IQO_HIP_EUNSUP;
        int xe = x + 1;
        while (xe < p.dstW && xe - x < kChunkOut) {
            int a, b;
            column_span(p, xe, &a, &b);
            int nlo = std::min(lo, a), nhi = std::max(hi, b);
            if (nhi - nlo > kChunkLds)
                break;
            lo = nlo;
            hi = nhi;
            ++xe;
        }
        chunks->push_back(make_int4(x, xe, lo, hi));
        *ldsInts = std::max(*ldsInts, hi - lo);
        x = xe;
    }
    return IQO_HIP_OK;
}

void free_plan(iqo_hip_plan *h)
{
    (void)hipFree(h->dBlob);
    delete h;
}

std::vector<int4> coord_records(const AxisPlan &a)
{
    std::vector<int4> v(a.coord.size());
    for (size_t i = 0; i < v.size(); ++i)
        v[i] = make_int4(a.coord[i].srcO, a.coord[i].tabOff, a.coord[i].kind, a.coord[i].aux);
    return v;
}

iqo_amd::RyxDev ryx_dev(const iqo_hip_plan *h);

// Every host table of a plan, in dependency order.  Host memory only: make_plan stages the result
// for upload (stage_*), the iqo_host_* queries stop here.
void build_host_tables(iqo_hip_plan *h)
{
    iqo_amd::build_tile_tables(h->p, &h->tt);
    h->tileTH0 = h->tt.TH;
    h->tileSrcRows0 = h->tt.srcRows;
    if (h->tt.ok)
        iqo_amd::build_walk_tables(h->p, h->tt, &h->wt);
    // Tables of the exact-ratio kernels (most take their coefficients as kernel arguments; ryx has
    // device tables).  Built whether or not the tile tables exist: ryx also serves shapes whose taps
    // exceed the tile kernel's (Lanczos-8/9 2:1).
    iqo_amd::build_up2(h->p, h->wt, &h->ut);
    iqo_amd::build_d32(h->p, h->wt, &h->dt);
    iqo_amd::build_d31(h->p, &h->t31);
    iqo_amd::build_ryx(h->p, &h->ryx);
#ifdef IQO_RYU_EXACT  // variant builds (A/B): exact-ratio upscale rows on the general-row kernels instead
    if (h->ryx.ok && h->ryx.Q > h->ryx.P)
        h->ryx = iqo_amd::RyxTables();
#endif
    if (!h->ryx.ok)
        iqo_amd::build_ryg(h->p, &h->ryx);  // general rows (no exact P:Q)
    if (h->ryx.ok && ryx_dev(h).parts == 0)
        h->ryx = iqo_amd::RyxTables();  // no column split fits the workgroup limits
    // Window-position records of a general upscale (plan.cpp build_ryu_positions, kernels.hip
    // ryu_kernel); none when a position holds more than 2 rows: ryg_kernel's NL = 1 mode runs the
    // plan.  With them the run-mode column table (runPairs > 0), where one exists.
    if (h->ryx.ok && h->ryx.general && h->ryx.rowLoads == 1)
        h->hasRyu = iqo_amd::build_ryu_positions(h->p.dstH, &h->ryx);
    if (h->hasRyu) {
        h->ryuBase = h->ryx.posBase;
        iqo_amd::build_ryu_runs(h->p.dstW, &h->ryx);
    }
    iqo_amd::build_a32(h->p, &h->at);
    iqo_amd::build_u23(h->p, &h->vt);
    iqo_amd::build_l23(h->p, &h->lt);
    // packed plans: the packed tiling over the tile tables
    if (h->channels > 1)
        iqo_amd::build_packed_tables(h->p, h->tt, h->channels, &h->pk);
}

void stage_walk(iqo_hip_plan *h)
{
    std::vector<int4> ws(h->wt.spans.size());
    for (size_t i = 0; i < ws.size(); ++i)
        ws[i] = make_int4(h->wt.spans[i].lo8, h->wt.spans[i].units, h->wt.spans[i].interior, 0);
    std::vector<int4> sg(2 * h->wt.segs.size());
    for (size_t i = 0; i < h->wt.segs.size(); ++i) {
        const iqo_amd::WalkSeg &g = h->wt.segs[i];
        sg[2 * i] = make_int4(g.first, g.slotOff, g.border, g.firstD);
        sg[2 * i + 1] = make_int4(static_cast<int>(g.yM), g.yS, g.yNeg, 0);
    }
    std::vector<int4> wr(h->wt.rows.size());
    for (size_t i = 0; i < wr.size(); ++i)
        wr[i] = make_int4(h->wt.rows[i].lo, h->wt.rows[i].hi, h->wt.rows[i].hiSlot, h->wt.rows[i].deno);
    upload(h, &h->dWSpans, ws.data(), ws.size());
    upload(h, &h->dWRows, wr.data(), wr.size());
    upload(h, &h->dWRowTap, h->wt.rowTap.data(), h->wt.rowTap.size());
    upload(h, &h->dWSegs, sg.data(), sg.size());
}

// The ratio-Y / general-row kernels' tables (the other exact-ratio kernels have no device tables:
// their coefficients are kernel arguments).
void stage_ryx(iqo_hip_plan *h)
{
    if (h->ryx.general) {
        // ryg_kernel reads the records of rows up to y1 - 1 + kRygPD + 1 unclamped (its FIFO look-ahead
        // and the next row's record): build_ryg's padding must cover them
        static_assert(iqo_amd::kRygRecPad >= iqo_amd::kRygPD + 2, "ryg row records: padding below the look-ahead");
        std::vector<int4> rr(h->ryx.rowRec.size() / 2);
        for (size_t i = 0; i < rr.size(); ++i) {
            const size_t ia = std::min(rr.size() - 1, i + iqo_amd::kRygPD - 1);  // (rows past the end repeat)
            rr[i] = make_int4(h->ryx.rowRec[2 * i], h->ryx.rowRec[2 * i + 1], h->ryx.rowRec[2 * ia], 0);
        }
        upload(h, &h->dRyxRowRec, rr.data(), rr.size());
    }
    if (h->hasRyu) {
        static_assert(iqo_amd::kRyuPosPad >= 3, "ryu_kernel reads the records up to a band's last position + 2");
        static_assert(iqo_amd::kRyuRec == 8, "ryu_kernel reads 8-int position records");
        upload(h, &h->dRyuPos, reinterpret_cast<const int4 *>(h->ryx.posRec.data()), h->ryx.posRec.size() / 4);
        if (h->ryx.runPairs > 0)
            upload(h, &h->dRyuRun, h->ryx.colRun.data(), h->ryx.colRun.size());
    }
    std::vector<int4> rc(h->ryx.cols.size() / 4);
    for (size_t i = 0; i < rc.size(); ++i)
        rc[i] = make_int4(h->ryx.cols[4 * i], h->ryx.cols[4 * i + 1], h->ryx.cols[4 * i + 2], 0);
    upload(h, &h->dRyxRowCoef, h->ryx.rowCoef.data(), h->ryx.rowCoef.size());
    upload(h, &h->dRyxColCoef, h->ryx.colCoef.data(), h->ryx.colCoef.size());
    upload(h, &h->dRyxCols, rc.data(), rc.size());
}

// The separable tile kernel's tables (TileRec / TileCol have the int4 / int2 layout).
void stage_tile(iqo_hip_plan *h)
{
    const iqo_amd::TileTables &t = h->tt;
    std::vector<int4> rows(t.rows.size()), spans(t.spans.size());
    std::vector<int2> cols(t.cols.size());
    for (size_t i = 0; i < rows.size(); ++i)
        rows[i] = make_int4(t.rows[i].start, t.rows[i].lo, t.rows[i].hi, t.rows[i].deno);
    for (size_t i = 0; i < cols.size(); ++i)
        cols[i] = make_int2(t.cols[i].a, t.cols[i].D);
    for (size_t i = 0; i < spans.size(); ++i) {
        int border = 0;  // any column of the tile with a Lanczos border division
        for (size_t x = i * t.CT; x < std::min(t.cols.size(), (i + 1) * t.CT); ++x)
            border |= t.cols[x].D != 0;
        spans[i] = make_int4(t.spans[i].lo8, t.spans[i].groups, border, 0);
    }
    // column coefficients transposed to [pair p][column-in-quad k][quad Q] (and window starts to
    // [k][Q]) over the padded tile width, so that a wave's load of one (p, k) is 64 consecutive
    // dwords; padding quads get zero coefficients and their tile's start (woff 0)
    const int nQp = static_cast<int>(spans.size()) * t.CT / 4;
    std::vector<uint32_t> coefT(static_cast<size_t>(t.NP) * 4 * nQp, 0u);
    std::vector<int32_t> colA(static_cast<size_t>(4) * nQp, 0);
    for (int Q = 0; Q < nQp; ++Q)
        for (int k = 0; k < 4; ++k) {
            const int x = 4 * Q + k;
            const bool in = x < static_cast<int>(t.cols.size());
            colA[static_cast<size_t>(k) * nQp + Q] = in ? t.cols[static_cast<size_t>(x)].a : t.spans[static_cast<size_t>(4 * Q / t.CT)].lo8;
            for (int p = 0; p < t.NP; ++p)
                coefT[(static_cast<size_t>(p) * 4 + k) * nQp + Q] = in ? t.colCoef[static_cast<size_t>(x) * t.NP + p] : 0u;
        }
    h->tileNQp = nQp;
    // per (row, tap): coefficient splat and the clamped source row it reads
    std::vector<uint2> rowTap(t.rowCoef.size());
    for (size_t y = 0; y < t.rows.size(); ++y)
        for (int i = 0; i < t.nYp; ++i) {
            const iqo_amd::TileRec &r = t.rows[y];
            const int row = std::min(std::max(r.start + i, r.lo), r.hi);
            rowTap[y * t.nYp + i] = make_uint2(t.rowCoef[y * t.nYp + i], static_cast<uint32_t>(row));
        }
    upload(h, &h->dTRows, rows.data(), rows.size());
    upload(h, &h->dTCols, cols.data(), cols.size());
    upload(h, &h->dTSpans, spans.data(), spans.size());
    upload(h, &h->dTRowTap, rowTap.data(), rowTap.size());
    upload(h, &h->dTColCoef, coefT.data(), coefT.size());
    upload(h, &h->dTColA, colA.data(), colA.size());
}

// Packed plans: the packed tiling over the tile tables stage_tile staged (its column coefficients
// are laid out over the planar tiles' padded width, which covers the narrower packed tiles').
void stage_packed(iqo_hip_plan *h)
{
    std::vector<int4> spans(h->pk.spans.size());
    for (size_t i = 0; i < spans.size(); ++i)
        spans[i] = make_int4(h->pk.spans[i].lo8, h->pk.spans[i].groups, h->pk.spans[i].border, 0);
    upload(h, &h->dPSpans, spans.data(), spans.size());
}

// The options of iqo_hip_plan_set_option, one row each: name, member, accepted values lo .. hi,
// default, and whether a caller of the public ABI may set it (the others are the A/B keys: kernel
// family switches and band / lane / prefetch / column-split schedules, every one speed-only,
// accepted only with IQO_HIP_TUNING=1, include/iqo_hip.h).  The tile height and the variant builds'
// two debug keys are no plain integers: they have handlers of their own in iqo_hip_plan_set_option.
struct Option {
    const char *name;
    int iqo_hip_plan::*member;
    long lo, hi;  // lo > hi (onoff): any value, stored as value != 0
    int def;
    bool pub;
};
using PlanT = iqo_hip_plan;
constexpr long kMax = std::numeric_limits<long>::max();
constexpr Option onoff(const char *name, int PlanT::*member, int def, bool pub) { return {name, member, 1, 0, def, pub}; }
constexpr Option kOptions[] = {
    onoff("force_general", &PlanT::forceGeneral, 0, true),  // general_kernel whatever the shape
    {"bands", &PlanT::bands, 0, kMax, 0, true},                    // bands per frame of the banded kernels (0 = auto)
    // host-pointer path of large frames (>= 4 MiB; speed only): 0 the runtime's pageable copies, 1 the
    // pinned staging pipeline (host_pipeline), for A/B
    {"host_stage", &PlanT::hostStage, 0, 1, 0, true},
    // block-shared Lanczos streamer: short bands for each XCD's last frame (0 auto, -1 off, n bands; speed only)
    {"tail", &PlanT::tail, -1, 4096, 0, false},
    // block-shared Lanczos streamer: target rounds for the auto band count (0 = 6, -1 = makespan model; speed only)
    {"rounds", &PlanT::rounds, -1, 64, 0, false},
    // ratio-Y kernel column parts (speed only): 0 one 8-wave workgroup per row where it fits, 1 default,
    // 2 / 3 parts of 2 / 1 waves, 4 the general rows' round-6 rule before one-wave parts
    {"ryx_split", &PlanT::ryxSplit, 0, 4, 1, false},
    // ratio-Y kernel adjacent column pairs per thread (speed only): 0 off, 1 where they fit
    {"ryx_adj", &PlanT::ryxAdj, 0, 1, 1, false},
    // ratio-Y upscales: 0 two output columns per thread, 1 four at the Lanczos 4:9 upscales (speed only)
    {"ryx_cpt", &PlanT::ryxCpt, 0, 1, 1, false},
    // ratio-Y kernel: uniform column coefficients as scalars where every column has the same; 0 per-lane
    // column coefficients everywhere (speed only)
    onoff("ryx_uc", &PlanT::ryxUc, 1, false),
    // general-row kernel, rows of > 1024 outputs: output columns per thread (0 auto, 2, 3, 4 -- not 1,
    // iqo_hip_plan_set_option; speed only)
    {"ryg_cpt", &PlanT::rygCpt, 0, 4, 0, false},
    // block-shared streamer, narrow frames side by side in one workgroup (speed only): 0 off, 1 where a
    // frame fills <= 1/2 wave, 2 from 2 frames
    {"stack", &PlanT::stack, 0, 2, 1, false},
    // Lanczos streamer prefetch depth (rows): ring streamer depth 1..3 / symmetric LDS ring K = 3..5
    {"prefetch", &PlanT::prefetch, 1, 4, 3, false},
    // A/B: 0 block-shared symmetric streamer where eligible, 1 accumulator-ring streamer, 2 per-wave
    // symmetric streamer (all bit-identical)
    {"stream_variant", &PlanT::streamVariant, 0, 2, 0, false},
    {"lanes", &PlanT::lanes, 0, 62, 0, false},  // Lanczos / Linear streamers: producing lanes per wave (0 = auto)
    // exact-ratio kernels: row groups loaded ahead (0 = kernel default; speed only); a depth the plan's
    // kernel does not instantiate fails the resize call with IQO_HIP_EINVAL
    {"ratio_prefetch", &PlanT::ratioPrefetch, 0, 8, 0, false},
    {"chunk_frames", &PlanT::chunkFrames, 0, kMax, 0, false},  // frames per launch (0 = up to 65535)
    onoff("tile", &PlanT::useTile, 1, false),  // 0: shapes without a specialised kernel use general_kernel
    onoff("walk", &PlanT::useWalk, 1, false),  // 0: general ratios use tile_kernel instead of the wave walker
    onoff("up2", &PlanT::useUp2, 1, false),    // 0: exact 2x Lanczos upscales use the wave walker alone
    onoff("d32", &PlanT::useD32, 1, false),    // 0: exact 3:2 Lanczos-3 downscales use the wave walker alone
    onoff("d31", &PlanT::useD31, 1, false),    // 0: exact 3:1 Lanczos downscales use the general kernels
    onoff("a32", &PlanT::useA32, 1, false),    // 0: exact 3:2 Area downscales use the wave walker alone
    onoff("u23", &PlanT::useU23, 1, false),    // 0: exact 2:3 Lanczos-3 upscales use the wave walker alone
    onoff("l23", &PlanT::useL23, 1, false),    // 0: exact 2:3 Linear upscales use the wave walker alone
    onoff("ryx", &PlanT::useRyx, 1, false),    // 0: exact-vertical-ratio downscales use the general kernels
    // 0: general-row downscales (1 .. 2 : 1) use the wave walker / tile kernel
    onoff("ryg", &PlanT::useRyg, 1, false),
    // 0: general upscale rows walk output rows (ryg_kernel's NL = 1 mode), not window positions (A/B)
    onoff("ryu", &PlanT::useRyu, 1, false),
    // 0: general upscale rows read each column's window separately (per-column mode, A/B)
    onoff("ryu_run", &PlanT::useRyuRun, 1, false),
};

// Every option iqo_hip_plan_set_option can change, back to its default.
void reset_options(iqo_hip_plan *h)
{
    for (const Option &o : kOptions)
        h->*o.member = o.def;
    h->debugFlags = 0;
#ifdef IQO_VARIANT_DEBUG
    h->traceAddr = 0;
#endif
    if (h->tt.ok) {  // option "tile_rows"
        h->tt.TH = h->tileTH0;
        h->tt.srcRows = h->tileSrcRows0;
    }
}

// Destroyed plans are kept (options reset) and handed out again for an identical request: the
// reference benchmark constructs and destroys its three resizers in every timed cycle
// (benchmark/benchmark.cpp:206-229), and a plan's host tables cost more to build than a small
// frame takes to resize.  Bounded; the oldest entry is freed first.
constexpr size_t kPlanCache = 16;
std::mutex g_planCacheMu;
std::vector<iqo_hip_plan *> g_planCache;

iqo_hip_plan *plan_cache_take(int m, unsigned degree, int channels, const size_t (&dims)[5], int device)
{
    std::lock_guard<std::mutex> g(g_planCacheMu);
    for (size_t i = g_planCache.size(); i-- > 0;) {
        iqo_hip_plan *h = g_planCache[i];
        if (h->keyMethod == m && h->keyDegree == degree && h->channels == channels && h->device == device &&
            std::equal(dims, dims + 5, h->keyDims)) {
            g_planCache.erase(g_planCache.begin() + static_cast<std::ptrdiff_t>(i));
            return h;
        }
    }
    return nullptr;
}

void plan_cache_put(iqo_hip_plan *h)
{
    reset_options(h);
    iqo_hip_plan *evict = nullptr;
    {
        std::lock_guard<std::mutex> g(g_planCacheMu);
        g_planCache.push_back(h);
        if (g_planCache.size() > kPlanCache) {
            evict = g_planCache.front();
            g_planCache.erase(g_planCache.begin());
        }
    }
    if (evict) {
        DeviceGuard guard(evict->device);
        free_plan(evict);
    }
}

int make_plan(iqo_amd::Method m, unsigned degree, size_t sw, size_t sh, size_t dw, size_t dh, size_t px,
              int device, iqo_hip_plan **out, int channels = 1)
{
    if (!out)
        return IQO_HIP_EINVAL;
    *out = nullptr;
    if (channels < 1 || channels > 4)
        return IQO_HIP_EINVAL;
    const size_t dims[5] = {sw, sh, dw, dh, px};
    if (iqo_hip_plan *c = plan_cache_take(static_cast<int>(m), degree, channels, dims, device)) {
        *out = c;
        return IQO_HIP_OK;
    }
    iqo_hip_plan *h = new (std::nothrow) iqo_hip_plan();
    if (!h)
        return IQO_HIP_ENOMEM;
    std::string err;
    if (!iqo_amd::build_plan(m, degree, sw, sh, dw, dh, px, &h->p, &err)) {
        delete h;
        return IQO_HIP_EINVAL;
    }
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count || !is_gfx950(device)) {
        delete h;
        return IQO_HIP_ENODEV;
    }
    h->device = device;
    h->keyMethod = static_cast<int>(m);
    h->keyDegree = degree;
    h->channels = channels;
    std::copy(dims, dims + 5, h->keyDims);
    DeviceGuard guard(device);
    if (!guard.ok()) {
        delete h;
        return IQO_HIP_ENODEV;
    }
    std::vector<int4> chunks;
    int rc = build_chunks(h->p, &chunks, &h->ldsInts);
    if (rc) {
        delete h;
        return rc;
    }
    h->nChunks = static_cast<int>(chunks.size());
    build_host_tables(h);
    // stage what has device tables, in the blob's section order
    std::vector<int4> xr = coord_records(h->p.x), yr = coord_records(h->p.y);
    upload(h, &h->dX, xr.data(), xr.size());
    upload(h, &h->dY, yr.data(), yr.size());
    upload(h, &h->dTabX, h->p.x.table.data(), h->p.x.table.size());
    upload(h, &h->dTabY, h->p.y.table.data(), h->p.y.table.size());
    upload(h, &h->dChunks, chunks.data(), chunks.size());
    if (h->wt.ok)
        stage_walk(h);
    if (h->ryx.ok)
        stage_ryx(h);
    if (h->tt.ok)
        stage_tile(h);
    if (h->pk.ok)
        stage_packed(h);
    *out = h;
    return IQO_HIP_OK;
}

uint32_t pair16(int lo, int hi) { return (static_cast<uint32_t>(lo) & 0xffffu) | (static_cast<uint32_t>(hi) << 16); }

// Device-side views of a plan for each kernel family (kernel arguments, no device memory).
iqo_amd::LanczosDev lanczos_dev(const iqo_hip_plan *h)
{
    const Plan &p = h->p;
    iqo_amd::LanczosDev l{};
    const iqo_amd::FastLanczos &f = p.flz;
    l.KY = f.KY;
    l.KX = f.KX;
    l.NY = f.NY;
    l.NXP = f.NXP;
    l.offX = f.offX;
    l.srcW = p.srcW;
    l.srcH = p.srcH;
    l.dstW = p.dstW;
    l.dstH = p.dstH;
    l.offY = f.offY;
    for (int i = 0; i < f.NY; ++i)
        l.cy[i] = pair16(f.cy[i], f.cy[i]);
    for (int i = 0; i < f.NXP / 2; ++i)
        l.cx[i] = pair16(f.cx[2 * i], f.cx[2 * i + 1]);
    l.mainBeginY = f.mainBeginY;
    l.mainEndY = f.mainEndY;
    l.mainBeginX = f.mainBeginX;
    l.mainEndX = f.mainEndX;
    for (int i = 0; i < 16; ++i) {
        l.yTopM[i] = f.yTopM[i];
        l.yTopS[i] = f.yTopS[i];
        l.yBotM[i] = f.yBotM[i];
        l.yBotS[i] = f.yBotS[i];
    }
    for (int k = 0; k < 8; ++k) {
        l.xM[k] = f.xM[k];
        l.xT[k] = f.xT[k];
    }
    if (f.NX == 20 && f.NY == 16) {  // Lanczos-5 2:1: kernels.hpp LanczosDev (reused fields)
        for (int k = 0; k < 16; ++k) {
            l.cx[k] = f.xM8[k];
            (k < 8 ? l.xM[k] : reinterpret_cast<uint32_t &>(l.xT[k - 8])) = static_cast<uint32_t>(f.xT8[k]);
        }
    }
    l.yTopNeg = f.yTopNeg;
    l.yBotNeg = f.yBotNeg;
    l.xNeg = f.xNeg;
    l.dbg = h->debugFlags;
#ifdef IQO_VARIANT_DEBUG
    l.trace = h->traceAddr;
#endif
    l.prefetch = h->prefetch;
    l.rounds = h->rounds;
    l.tail = h->tail;
    l.stack = h->stack;
    l.sym = !f.sym || h->streamVariant == 1 ? 0 : (h->streamVariant >= 2 ? h->streamVariant : 1);
    if (f.NY == 12 || f.NY == 16)
        l.sym = 1;  // Lanczos-4 / -5 2:1: the block-shared symmetric streamer is their only instantiation
    l.NX = f.NX;
    l.offXO = f.offXO;
    for (int i = 0; i < f.NX / 2 && i < 10; ++i)
        (i < 8 ? l.cxo[i] : l.cy[i]) = pair16(f.cxo[2 * i], f.cxo[2 * i + 1]);  // (pairs 8, 9: Lanczos-5)
    l.np = h->lanes;
    return l;
}

iqo_amd::AreaDev area_dev(const iqo_hip_plan *h)
{
    const Plan &p = h->p;
    iqo_amd::AreaDev a{};
    a.KY = p.far.KY;
    a.KX = p.far.KX;
    a.srcW = p.srcW;
    a.dstW = p.dstW;
    for (int i = 0; i < a.KY; ++i)
        a.cy[i] = pair16(p.far.cy[i], p.far.cy[i]);
    for (int i = 0; i < (a.KX + 1) / 2; ++i)  // odd KX: the last pair is (c_{KX-1}, 0)
        a.cx[i] = pair16(p.far.cx[2 * i], 2 * i + 1 < a.KX ? p.far.cx[2 * i + 1] : 0);
    a.dstH = p.dstH;
    a.lin = p.far.lin ? 1 : 0;
    a.srcH = p.srcH;
    return a;
}

iqo_amd::LinearDev linear_dev(const iqo_hip_plan *h)
{
    const Plan &p = h->p;
    iqo_amd::LinearDev l{};
    l.srcW = p.srcW;
    l.srcH = p.srcH;
    l.dstW = p.dstW;
    l.dstH = p.dstH;
    l.F = p.fln.F;
    for (int q = 0; q < 3; ++q) {
        l.cx[q] = pair16(p.fln.cx[q][0], p.fln.cx[q][1]);
        l.cy[q] = pair16(p.fln.cy[q][0], p.fln.cy[q][1]);
    }
    l.dbg = h->debugFlags;
    l.np = h->lanes;
    return l;
}

iqo_amd::TileDev tile_dev(const iqo_hip_plan *h)
{
    const iqo_amd::TileTables &t = h->tt;
    iqo_amd::TileDev d;
    d.lanczos = h->p.method == iqo_amd::kLanczos;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.NP = t.NP;
    d.nYp = t.nYp;
    d.CT = t.CT;
    d.TH = t.TH;
    d.pitchDw = t.pitchDw;
    d.log2nQ = t.log2nQ;
    d.srcRows = t.srcRows;
    d.spitch = t.spitch;
    d.rows = h->dTRows;
    d.rowTap = h->dTRowTap;
    d.cols = h->dTCols;
    d.colCoef = h->dTColCoef;
    d.colA = h->dTColA;
    d.nQp = h->tileNQp;
    d.spans = h->dTSpans;
    return d;
}

// packed_tile_kernel: the tile tables with the packed tiling (plan.hpp PackedTables)
iqo_amd::TileDev packed_tile_dev(const iqo_hip_plan *h)
{
    iqo_amd::TileDev d = tile_dev(h);
    const iqo_amd::PackedTables &k = h->pk;
    d.CT = k.CT;
    d.TH = k.TH;
    d.pitchDw = k.pitchDw;
    d.log2nQ = k.log2nQ;
    d.srcRows = k.srcRows;
    d.spitch = k.spitch;
    d.spans = h->dPSpans;
    return d;
}

iqo_amd::WalkDev walk_dev(const iqo_hip_plan *h)
{
    const iqo_amd::WalkTables &w = h->wt;
    iqo_amd::WalkDev d;
    d.t = tile_dev(h);
    d.nS = w.nS;
    d.spans = h->dWSpans;
    d.NV = w.NV;
    d.R = w.R;
    d.pitch = w.pitch;
    d.waveBytes = static_cast<int>(w.waveBytes);
    d.rowTap = h->dWRowTap;
    d.rows = h->dWRows;
    d.segs = h->dWSegs;
    return d;
}

iqo_amd::Up2Dev up2_dev(const iqo_hip_plan *h)
{
    const iqo_amd::Up2Tables &u = h->ut;
    iqo_amd::Up2Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.F = u.F;
    d.NT = u.NT;
    d.np = h->lanes;
    d.cy0 = u.cy0;
    d.cx0 = u.cx0;
    std::memcpy(d.cy1, u.cy1, sizeof d.cy1);
    std::memcpy(d.cx1, u.cx1, sizeof d.cx1);
    std::memcpy(d.xM, u.xM, sizeof d.xM);
    std::memcpy(d.xT, u.xT, sizeof d.xT);
    d.m0 = u.m0;
    d.m1 = u.m1;
    std::memcpy(d.yM, u.yM, sizeof d.yM);
    std::memcpy(d.yS, u.yS, sizeof d.yS);
    return d;
}

iqo_amd::D32Dev d32_dev(const iqo_hip_plan *h)
{
    const iqo_amd::D32Tables &t = h->dt;
    iqo_amd::D32Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.np = h->lanes;
    d.pd = h->ratioPrefetch;
    d.variant = t.variant;
    std::memcpy(d.cy, t.cy, sizeof d.cy);
    std::memcpy(d.cx, t.cx, sizeof d.cx);
    std::memcpy(d.xM, t.xM, sizeof d.xM);
    std::memcpy(d.xT, t.xT, sizeof d.xT);
    d.m0 = t.m0;
    d.m1 = t.m1;
    std::memcpy(d.yM, t.yM, sizeof d.yM);
    std::memcpy(d.yS, t.yS, sizeof d.yS);
    return d;
}

iqo_amd::D31Dev d31_dev(const iqo_hip_plan *h)
{
    const iqo_amd::D31Tables &t = h->t31;
    iqo_amd::D31Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.np = h->lanes;
    d.pd = h->ratioPrefetch;
    d.variant = t.variant;
    d.cc = t.cc;
    std::memcpy(d.cp, t.cp, sizeof d.cp);
    std::memcpy(d.cxe, t.cxe, sizeof d.cxe);
    std::memcpy(d.cxo, t.cxo, sizeof d.cxo);
    std::memcpy(d.xM, t.xM, sizeof d.xM);
    std::memcpy(d.xT, t.xT, sizeof d.xT);
    d.m0 = t.m0;
    d.m1 = t.m1;
    std::memcpy(d.yM, t.yM, sizeof d.yM);
    std::memcpy(d.yS, t.yS, sizeof d.yS);
    return d;
}

iqo_amd::RyxDev ryx_dev(const iqo_hip_plan *h)
{
    const iqo_amd::RyxTables &t = h->ryx;
    iqo_amd::RyxDev d;
    d.lanczos = h->p.method == iqo_amd::kLanczos;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.P = t.P;
    d.Q = t.Q;
    d.taps = t.taps;
    d.NP = t.NP;
    d.off = t.off;
    d.m0 = t.m0;
    d.m1 = t.m1;
    std::memcpy(d.yM, t.yM, sizeof d.yM);
    std::memcpy(d.yS, t.yS, sizeof d.yS);
    d.rowCoef = h->dRyxRowCoef;
    d.cols = h->dRyxCols;
    d.colCoef = h->dRyxColCoef;
    // column split into `n` workgroups of `threads` threads: output columns [xs[k], xs[k+1]) (even,
    // 2 per thread) from source columns [cs[k], ce[k]) (multiples of 4, 4 per thread)
    auto split = [&](int n, int threads) -> bool {
        int xs[17], cs[16], ce[16];
        for (int k = 0; k <= n; ++k)
            xs[k] = k == 0 ? 0 : k == n ? d.dstW : (k * d.dstW / n + 1) & ~1;
        for (int k = 0; k < n; ++k) {
            int lo = 1 << 30, hi = -(1 << 30);
            for (int x = xs[k]; x < xs[k + 1]; ++x) {
                const int a = t.cols[static_cast<size_t>(x) * 4] / 2 - iqo_amd::kRyxPad;  // even window start
                lo = std::min(lo, a);
                hi = std::max(hi, a + 2 * t.NP);
            }
            cs[k] = k == 0 ? 0 : std::max(0, lo) & ~3;
            ce[k] = k == n - 1 ? d.srcW : std::min(d.srcW, (hi + 3) & ~3);
            if (ce[k] - cs[k] > 4 * threads || xs[k + 1] - xs[k] > d.cpt * threads || (k > 0 && lo < 0) ||
                (k < n - 1 && hi > d.srcW) || xs[k + 1] <= xs[k])
                return false;
        }
        d.parts = n;
        d.threads = threads;
        for (int k = 0; k < 17; ++k)
            d.xs[k] = k <= n ? xs[k] : d.dstW;
        for (int k = 0; k < 16; ++k) {
            d.cs[k] = k < n ? cs[k] : 0;
            d.ce[k] = k < n ? ce[k] : d.srcW;
        }
        return true;
    };
    // the fewest parts of `threads` threads that hold the row (up to 16)
    auto split_min = [&](int threads) {
        for (int n = 1; n <= 16; ++n)
            if (split(n, threads))
                return true;
        return false;
    };
    // Lanczos: workgroups of 4 waves (half or a quarter of the row each) when their source spans
    // fit 256 threads x 4 columns: barriers over 4 waves instead of 8 (1080p -> 480p: Lanczos-2
    // 0.171 vs 0.182 ms, Lanczos-3 0.232 vs 0.239, profiles/r03/ryx_split.txt; 4K -> 960x540
    // Lanczos-3 0.441 vs 0.404 ms with four parts instead of two of 8 waves; Area 5 % slower,
    // so not for Area).  Option "ryx_split": 0 one 8-wave workgroup per row where it fits, 2 / 3
    // parts of 2 waves / 1 wave.  parts = 0: no split fits (build_plan then drops the kernel).
    d.parts = 0;
    d.threads = 512;
    // Lanczos-3 upscales (4:9 rows, 4 pairs): 4 output columns per thread in one workgroup per row
    // (640 -> 1920 in 480 threads instead of four 256-thread parts of 2 columns per thread: 0.333
    // vs 0.359 ms; Lanczos-2 with 6 columns per thread was slower, 0.379 vs 0.308 ms,
    // profiles/r04/ryx_up49.txt)
    d.cpt = 2;
    if (d.Q > d.P && d.NP >= 4 && h->ryxCpt) {
        d.cpt = 4;
        const int need = std::max((d.srcW + 3) / 4, (d.dstW + d.cpt - 1) / d.cpt);
        if (need <= 512 && split(1, (need + 63) / 64 * 64))
            return d;
        if (split_min(512))
            return d;
        d.cpt = 2;
        d.parts = 0;
    }
    // general rows (ryg): output columns per thread ~ 4 x dstW / srcW, so that the threads of the
    // horizontal pass (CPT columns each) match those of the vertical pass (4 source columns each):
    // 1080p -> 1366x768 with 3 columns per thread (two parts of 256 threads) 0.256 ms vs 4 columns
    // 0.308 (a third of the threads idle in the horizontal pass), 2 columns needed four parts
    // (profiles/r05/steady_ryg_cpt.txt); option "ryg_cpt" forces 2, 3 or 4
    if (t.general) {
        // (12-row windows or 6 column pairs with 4 columns per thread spill: 3 at most there; 16-row
        // windows spill at 3: 2 there, Lanczos-6 1080p -> 1366x768 0.490 -> 0.381 ms,
        // profiles/r06/ryg_l45.txt)
        const int cap = t.taps >= 16 ? 2 : t.taps >= 12 || t.NP >= 6 ? 3 : 4;
        d.cpt = h->rygCpt ? h->rygCpt : std::min(cap, std::max(2, (4 * d.dstW + d.srcW / 2) / d.srcW));
        if (t.rowLoads >= 3)
            d.cpt = 2;  // (downscales past 2:1: 2 columns per thread is the only instantiation)
        // (round 6, late) parts of ONE wave where the row fits 16 of them: a barrier over one wave
        // instead of 4 or 8, and no 512-thread part half idle (2560 columns took two parts of 512
        // threads for 640 columns' work).  Lanczos downscale rows: 2560x1440 -> 1024x576 0.554 ->
        // 0.339 ms, -> 1920x1080 0.393 -> 0.255, 4K -> 1600x900 0.429 -> 0.363, 1080p -> 1366x768
        // -2.6 %; rows that need more than 16 parts of one wave take parts of two waves below 4 rows
        // per output row (4K -> 1366x768 0.399 -> 0.332; at 4 rows the 22-tap kernel, which spills,
        // was 11 % slower in them).  Upscale rows keep one or two workgroups where those hold the
        // row (1024x576 -> 1080p was 6 % slower in one-wave parts) and take one-wave parts where
        // not (1366x768 -> 2560x1440 0.263 -> 0.225).  Area rows keep the 8-wave parts (4K ->
        // 1366x768 12 % slower in one-wave parts).  profiles/r06/ryg_split.txt; option ryx_split = 4
        // restores the previous rule.
        if (h->ryxSplit == 1 && d.lanczos) {
            if (t.rowLoads >= 2 && (split_min(64) || (t.rowLoads < 4 && split_min(128))))
                return d;
            if (t.rowLoads == 1 && !split(2, 256) && !split(1, 512) && split_min(64))
                return d;
        }
        const int split_opt = h->ryxSplit == 4 ? 1 : h->ryxSplit;
        const int tw = split_opt == 2 ? 128 : 64;
        if ((split_opt >= 2 && split_min(tw)) || (split_opt == 1 && split(2, 256)) || split(1, 512))
            return d;  // (ryx_split 0: one 8-wave part where it fits)
        // (round 5, late) one more column per thread when that keeps the row in one workgroup, else
        // the fewest parts, each of the fewest 64-thread multiples that hold it: 1080p -> 1600x900
        // had two 512-thread parts with half their threads idle
        if (!h->rygCpt && t.rowLoads < 3 && d.cpt < cap) {
            ++d.cpt;
            if (split(1, 512))
                return d;
            --d.cpt;
        }
        for (int n = 2; n <= 16; ++n)
            for (int th = 128; th <= 512; th += 64)
                if (split(n, th))
                    return d;
        d.cpt = 2;
        d.parts = 0;
    }
    const int sopt = h->ryxSplit == 4 ? 1 : h->ryxSplit;  // (4: the previous rules, above and here)
    const int tw = sopt == 2 ? 128 : sopt == 3 ? 64 : 256;
    if (!(sopt >= 2 && split_min(tw)) && !(sopt == 1 && d.lanczos && d.dstW >= 64 && split(2, 256)) && !split(1, 512) &&
        !(sopt == 1 && split(4, 256)))
        split_min(512);
    // (round 6, late) Lanczos rows whose parts are less than 3/4 busy take the fewest parts of one
    // wave instead: 2560 columns in four 256-thread parts left 96 threads of each idle (2560x1440 ->
    // 640x360 0.299 -> 0.240 ms, Lanczos-2 -> 1138x640 0.319 -> 0.263, Lanczos-6 -> 720p 0.235 ->
    // 0.191); the 1080p / 4K rows of the bench list fill their parts to 94-97 % and keep them (there
    // one-wave parts were 5-10 % slower), profiles/r06/ryg_split.txt
    if (h->ryxSplit == 1 && d.lanczos && d.parts > 0) {
        int busy = 0;
        for (int k = 0; k < d.parts; ++k)
            busy += std::max((d.ce[k] - d.cs[k] + 3) / 4, (d.xs[k + 1] - d.xs[k] + d.cpt - 1) / d.cpt);
        if (4 * busy < 3 * d.parts * d.threads)
            split_min(64);  // (leaves the split as it is when no one-wave split holds the row)
    }
    // adjacent column pairs per thread (9:4 only, where every pair's windows start 1 or 2 pairs
    // apart, i.e. columns at 2:1 or more): one LDS run of NP + 2 dwords for both columns
    d.adj = 0;
    if (d.parts > 0 && h->ryxAdj && d.P == 2 && d.Q == 1 && d.lanczos && d.cpt == 2) {
        // 2:1 rows with 2:1 columns (uniform coefficients, below): every pair's windows one pair apart
        bool ok = true;
        for (int k = 0; k < d.parts && ok; ++k)
            for (int x = d.xs[k]; x + 1 < d.xs[k + 1] && ok; x += 2)
                ok = t.cols[static_cast<size_t>(x + 1) * 4] - t.cols[static_cast<size_t>(x) * 4] == 4;
        d.adj = ok ? 1 : 0;
    }
    if (d.parts > 0 && h->ryxAdj && d.P == 9 && d.Q == 4) {
        bool ok = true;
        for (int k = 0; k < d.parts && ok; ++k)
            for (int x = d.xs[k]; x + 1 < d.xs[k + 1] && ok; x += 2) {
                const int dl = t.cols[static_cast<size_t>(x + 1) * 4] - t.cols[static_cast<size_t>(x) * 4];
                ok = dl == 4 || dl == 8;
            }
        d.adj = ok ? 1 : 0;
    }
    // uniform column coefficients (Lanczos 2:1 columns): the kernel keeps them in scalar registers,
    // not NP x CPT per-lane registers (Lanczos-9: 38 VGPRs, the difference between 2 and 4 waves
    // per SIMD); option "ryx_uc" = 0 keeps the per-lane tables
    d.uc = 0;
    if (d.parts > 0 && h->ryxUc && d.lanczos && d.P == 2 && d.Q == 1 && d.cpt == 2) {
        bool same = true;
        const size_t np = static_cast<size_t>(t.NP);
        for (size_t x = 1; x < static_cast<size_t>(d.dstW) && same; ++x)
            same = std::equal(t.colCoef.begin() + static_cast<ptrdiff_t>(x * np), t.colCoef.begin() + static_cast<ptrdiff_t>((x + 1) * np),
                              t.colCoef.begin());
        d.uc = same ? 1 : 0;
    }
    if (d.adj && d.P == 2 && !d.uc)
        d.adj = 0;  // (2:1 adjacent pairs: uniform-column instantiations only)
    return d;
}

// The general-row kernel's view: ryx_dev's column split and tables plus the row records.
iqo_amd::RygDev ryg_dev(const iqo_hip_plan *h)
{
    const iqo_amd::RyxDev x = ryx_dev(h);
    iqo_amd::RygDev d;
    d.lanczos = x.lanczos;
    d.srcW = x.srcW;
    d.srcH = x.srcH;
    d.dstW = x.dstW;
    d.dstH = x.dstH;
    d.taps = x.taps;
    d.NP = x.NP;
    d.m0 = x.m0;
    d.m1 = x.m1;
    std::memcpy(d.yM, x.yM, sizeof d.yM);
    std::memcpy(d.yS, x.yS, sizeof d.yS);
    d.rowRec = h->dRyxRowRec;
    d.rowCoef = x.rowCoef;
    d.cols = x.cols;
    d.colCoef = x.colCoef;
    d.parts = x.parts;
    d.threads = x.threads;
    std::memcpy(d.xs, x.xs, sizeof d.xs);
    std::memcpy(d.cs, x.cs, sizeof d.cs);
    std::memcpy(d.ce, x.ce, sizeof d.ce);
    d.cpt = x.cpt;
    d.nl = h->ryx.rowLoads;
    if (d.nl == 1 && h->hasRyu && h->useRyu) {
        d.posRec = h->dRyuPos;
        d.posBase = h->ryuBase;
        d.posRows = h->ryx.posRows;
        // run mode: 4 adjacent columns per thread, every part starting on a multiple of 4 columns
        bool aligned = d.cpt == 4 && h->ryx.runPairs > 0 && h->useRyuRun;
        for (int k = 0; k < d.parts && aligned; ++k)
            aligned = d.xs[k] % 4 == 0;
        if (aligned) {
            d.colRun = h->dRyuRun;
            d.run = h->ryx.runPairs;
        }
    }
    return d;
}

iqo_amd::L23Dev l23_dev(const iqo_hip_plan *h)
{
    iqo_amd::L23Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.np = h->lanes;
    d.pd = h->ratioPrefetch;
    std::memcpy(d.cy, h->lt.cy, sizeof d.cy);
    std::memcpy(d.cx, h->lt.cx, sizeof d.cx);
    return d;
}

iqo_amd::U23Dev u23_dev(const iqo_hip_plan *h)
{
    const iqo_amd::U23Tables &t = h->vt;
    iqo_amd::U23Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.np = h->lanes;
    d.pd = h->ratioPrefetch;
    d.cy0 = t.cy0;
    d.cx0 = t.cx0;
    std::memcpy(d.cy, t.cy, sizeof d.cy);
    std::memcpy(d.cx, t.cx, sizeof d.cx);
    std::memcpy(d.xM, t.xM, sizeof d.xM);
    std::memcpy(d.xT, t.xT, sizeof d.xT);
    d.m0 = t.m0;
    d.m1 = t.m1;
    std::memcpy(d.yM, t.yM, sizeof d.yM);
    std::memcpy(d.yS, t.yS, sizeof d.yS);
    return d;
}

iqo_amd::A32Dev a32_dev(const iqo_hip_plan *h)
{
    iqo_amd::A32Dev d;
    d.srcW = h->p.srcW;
    d.srcH = h->p.srcH;
    d.dstW = h->p.dstW;
    d.dstH = h->p.dstH;
    d.np = h->lanes;
    d.pd = h->ratioPrefetch;
    std::memcpy(d.cy, h->at.cy, sizeof d.cy);
    std::memcpy(d.cx, h->at.cx, sizeof d.cx);
    return d;
}

iqo_amd::GeneralDev general_dev(const iqo_hip_plan *h)
{
    const Plan &p = h->p;
    iqo_amd::GeneralDev g{};
    g.method = p.method;
    g.srcW = p.srcW;
    g.srcH = p.srcH;
    g.dstW = p.dstW;
    g.nX = p.x.taps;
    g.nY = p.y.taps;
    g.xInfo = h->dX;
    g.yInfo = h->dY;
    g.tabX = h->dTabX;
    g.tabY = h->dTabY;
    g.chunks = h->dChunks;
    g.nChunks = h->nChunks;
    g.ldsInts = h->ldsInts;
    return g;
}

// The ratio-Y kernel is usable when its tables exist and a column split fits for the plan's
// CURRENT options (ryx_split / ryx_cpt are speed options; upload_exact checked the defaults only).
// The defaults end in split_min(512), the widest split, so when they fit every option does.
bool ryx_usable(const iqo_hip_plan *h)
{
    return h->ryx.ok && !h->ryx.general && h->useRyx && ryx_dev(h).parts > 0;
}

// ... and its general-row variant (build_ryg)
bool ryg_usable(const iqo_hip_plan *h)
{
    return h->ryx.ok && h->ryx.general && h->useRyg && ryx_dev(h).parts > 0;
}

// Area and Linear rows shrinking by less than 1.4, or with two row phases (exact 3:2), keep the wave
// walker when it can run: ryg loads NL = 2 rows per output row and is slower there (steady clock,
// x256: Area 1080p -> 1600x900 0.368 vs 0.267 ms, 1440p -> 1080p 0.415 vs 0.356, Linear 3:2 0.181
// vs 0.163; at 45:32 ryg is ahead, Area 0.198 vs 0.271; profiles/r05/ratio_sweep_ryg_ab.txt)
bool walk_beats_ryg(const iqo_hip_plan *h)
{
    const Plan &p = h->p;
    return p.method != iqo_amd::kLanczos && (5 * p.srcH < 7 * p.dstH || p.y.phases <= 2);
}

// What a call's pointers and strides offer the kernels' vector accesses: base, row stride and frame
// stride OR-ed into one word per side.  All three are multiples of a power of two a exactly when the
// word's low bits a - 1 are zero.
struct Layout {
    uintptr_t src, dst;
};
constexpr Layout kAlignedLayout{0, 0};
// an alignment the iqo_host_* / instance queries take for a layout: a power of two, 1 .. 16
bool valid_align(size_t a) { return a >= 1 && a <= 16 && !(a & (a - 1)); }

Layout layout_of(const void *src, size_t srcSt, size_t srcFrameSt, const void *dst, size_t dstSt, size_t dstFrameSt)
{
    return Layout{reinterpret_cast<uintptr_t>(src) | srcSt | srcFrameSt, reinterpret_cast<uintptr_t>(dst) | dstSt | dstFrameSt};
}

// The alignment in bytes that each kernel family's vector accesses need of the source and of the
// destination (base, row stride and frame stride alike).
struct Align {
    unsigned src, dst;
};

Align kernel_align(const iqo_hip_plan *h, int kernel)
{
    switch (kernel) {
    case IQO_KERNEL_LANCZOS_STREAM:  // 16-B loads, 16 / KX output bytes per thread
        return {16, 16u / static_cast<unsigned>(h->p.flz.KX)};
    case IQO_KERNEL_AREA_INT: {
        // 16-B loads / 16 / KX output bytes per thread; 12-B loads / 12 / KX bytes when KX is 3 or 6
        const unsigned KX = static_cast<unsigned>(h->p.far.KX), cols = 16 % KX == 0 ? 16 : 12;
        return {cols == 16 ? 16u : 4u, cols / KX};
    }
    case IQO_KERNEL_LINEAR_UP2:
        return {8, 16};
    case IQO_KERNEL_WALK:  // the wave walker loads aligned dwords: 4-byte aligned source frames and rows
        return {4, 1};
    case IQO_KERNEL_LANCZOS_UP2:  // the 2x Lanczos kernel loads 8 B per lane and stores 16 B per lane
        return {8, 16};
    case IQO_KERNEL_LANCZOS_D32:  // the 3:2 Lanczos kernel loads 12 B per lane (4-byte aligned) and stores 8 B per lane
        return {4, 8};
    case IQO_KERNEL_LANCZOS_D31:  // the 3:1 Lanczos kernel loads 12 B per lane (4-byte aligned) and stores 4 B per lane
        return {4, 4};
    case IQO_KERNEL_AREA_D32:
        return {4, 8};
    case IQO_KERNEL_LANCZOS_U23:  // the 2:3 Lanczos kernel loads 8 B per lane and stores 12 B per lane
    case IQO_KERNEL_LINEAR_U23:
        return {8, 4};
    default:
        // general_kernel; tile_kernel: any alignment (the kernel adapts per frame); ryx (exact vertical
        // ratio, tabled columns): dword loads (round 5: unaligned dword loads verified on gfx950,
        // profiles/r05/unaligned_src.txt), 2-byte stores (1-byte stores when the destination is not
        // 2-byte aligned, launch_ryx); ryg (general rows): dword loads, byte stores
        return {1, 1};
    }
}

bool layout_fits(const iqo_hip_plan *h, int kernel, Layout l)
{
    const Align a = kernel_align(h, kernel);
    assert(a.src && !(a.src & (a.src - 1)) && a.dst && !(a.dst & (a.dst - 1)));  // powers of two (Layout)
    return !(l.src & (a.src - 1)) && !(l.dst & (a.dst - 1));
}

// The kernel family a call with this layout runs: the first family of the cascade below that has
// the plan's shape, is switched on, and finds the alignment its vector accesses need
// (kernel_align).  A family refused for alignment leaves the plan with the walker / tile kernel for
// the later steps, and in the end with the general kernel.
int select_kernel(const iqo_hip_plan *h, Layout l)
{
    if (h->channels > 1)  // packed plans: none of the planar kernels; both packed kernels take any alignment
        return h->pk.ok && !h->forceGeneral ? IQO_KERNEL_PACKED_TILE : IQO_KERNEL_PACKED_GENERAL;
    // the plan's streamer family (build_plan: LANCZOS_STREAM, AREA_INT, LINEAR_UP2), else the general kernel
    int k = h->forceGeneral ? IQO_KERNEL_GENERAL : h->p.kernel;
    if (!layout_fits(h, k, l))
        k = IQO_KERNEL_GENERAL;
    if (k == IQO_KERNEL_GENERAL && !h->forceGeneral && h->tt.ok && h->useTile)
        k = IQO_KERNEL_TILE;
    if (k == IQO_KERNEL_TILE && h->wt.ok && h->useWalk && layout_fits(h, IQO_KERNEL_WALK, l))
        k = IQO_KERNEL_WALK;
    // an exact-ratio family takes over from the walker / tile kernel
    auto take = [&](int family, bool have) {
        if ((k == IQO_KERNEL_WALK || k == IQO_KERNEL_TILE) && have && layout_fits(h, family, l))
            k = family;
    };
    take(IQO_KERNEL_LANCZOS_UP2, h->ut.ok && h->useUp2);
    take(IQO_KERNEL_LANCZOS_D32, h->dt.ok && h->useD32);
    take(IQO_KERNEL_LANCZOS_D31, h->t31.ok && h->useD31);
    // (ryx also takes shapes whose taps exceed the tile kernel's tables: Lanczos-8/9 2:1)
    if ((k == IQO_KERNEL_WALK || k == IQO_KERNEL_TILE || (k == IQO_KERNEL_GENERAL && !h->forceGeneral)) &&
        ryx_usable(h))
        k = IQO_KERNEL_RYX;
    take(IQO_KERNEL_AREA_D32, h->at.ok && h->useA32);
    take(IQO_KERNEL_LANCZOS_U23, h->vt.ok && h->useU23);
    take(IQO_KERNEL_LINEAR_U23, h->lt.ok && h->useL23);
    // general rows last: only what no exact-ratio kernel takes
    if ((k == IQO_KERNEL_TILE || (k == IQO_KERNEL_WALK && !walk_beats_ryg(h))) && ryg_usable(h))
        k = IQO_KERNEL_RYG;
    return k;
}

// The kernel family a full-frame call with aligned pointers and strides runs.
int plan_kernel(const iqo_hip_plan *h) { return select_kernel(h, kAlignedLayout); }

// The kernel family a call with these pointers and strides runs.
int kernel_for_layout(const iqo_hip_plan *h, const void *src, size_t srcSt, size_t srcFrameSt, const void *dst,
                      size_t dstSt, size_t dstFrameSt)
{
    return select_kernel(h, layout_of(src, srcSt, srcFrameSt, dst, dstSt, dstFrameSt));
}

iqo_hip_instance to_desc(const iqo_amd::Instance &k)
{
    iqo_hip_instance d{};
    d.family = k.family;
    d.sub = k.sub;
    d.LZ = k.LZ;
    d.P = k.P;
    d.Q = k.Q;
    d.T = k.T;
    d.NP = k.NP;
    d.PD = k.PD;
    d.ADJ = k.ADJ;
    d.CPT = k.CPT;
    d.UC = k.UC;
    d.NL = k.NL;
    d.RUN = k.RUN;
    d.KM = k.KM;
    d.VY = k.VY;
    d.NV = k.NV;
    d.NT = k.NT;
    d.F = k.F;
    d.VARIANT = k.VARIANT;
    return d;
}

// The exact-ratio kernels instantiate a few prefetch depths each; any other forced depth is an
// error, not a silent fall-back to the default kernel.
bool ratio_prefetch_ok(const iqo_hip_plan *h, int kernel)
{
    const int pd = h->ratioPrefetch;
    if (pd <= 0)
        return true;
    if (kernel == IQO_KERNEL_LANCZOS_D32)
        return h->dt.variant == 0 ? (pd == 1 || pd == 2 || pd == 4) : (pd == 1 || pd == 3);
    if (kernel == IQO_KERNEL_LANCZOS_D31)
        return h->t31.variant == 0 ? (pd == 1 || pd == 5) : (pd == 1 || pd == 2 || pd == 4);
    if (kernel == IQO_KERNEL_LANCZOS_U23 || kernel == IQO_KERNEL_LINEAR_U23)
        return pd == 1 || pd == 2;
    if (kernel == IQO_KERNEL_AREA_D32)
        return pd == 2 || pd == 4 || pd == 8;
    return true;
}

// The instantiation a full-frame call with this layout runs (iqo_hip.h iqo_hip_instance): the family
// of select_kernel, then the family's own lookup (kernels.hpp) on the *Dev the launch would get.  Host
// data only, so it also serves a plan without device tables (iqo_host_instance_for): there the device
// pointers of the *Dev are null, and the general rows' two decisions that launch_ryg reads off pointers
// come from what ryg_dev itself decided -- rows by window position exactly when it set posRec
// (nl == 1 && hasRyu && useRyu), the run mode exactly when it set d.run.
int plan_instance(const iqo_hip_plan *h, Layout l, iqo_hip_instance *out)
{
    static_assert(iqo_amd::kFamTile == IQO_KERNEL_TILE && iqo_amd::kFamWalk == IQO_KERNEL_WALK &&
                      iqo_amd::kFamUp2 == IQO_KERNEL_LANCZOS_UP2 && iqo_amd::kFamD32 == IQO_KERNEL_LANCZOS_D32 &&
                      iqo_amd::kFamA32 == IQO_KERNEL_AREA_D32 && iqo_amd::kFamU23 == IQO_KERNEL_LANCZOS_U23 &&
                      iqo_amd::kFamL23 == IQO_KERNEL_LINEAR_U23 && iqo_amd::kFamD31 == IQO_KERNEL_LANCZOS_D31 &&
                      iqo_amd::kFamRyx == IQO_KERNEL_RYX && iqo_amd::kFamRyg == IQO_KERNEL_RYG &&
                      iqo_amd::kSubRyu == IQO_INSTANCE_SUB_RYU,
                  "kernels.hpp kFam* are iqo_hip.h IQO_KERNEL_*");
    if (h->channels > 1)
        return IQO_HIP_EUNSUP;
    const int kernel = select_kernel(h, l);
    if (!ratio_prefetch_ok(h, kernel))
        return IQO_HIP_EINVAL;
    const iqo_amd::Instance *k = nullptr;
    switch (kernel) {
    case IQO_KERNEL_TILE: k = iqo_amd::tile_instance(tile_dev(h)); break;
    case IQO_KERNEL_WALK: k = iqo_amd::walk_instance(walk_dev(h)); break;
    case IQO_KERNEL_LANCZOS_UP2: k = iqo_amd::up2_instance(up2_dev(h)); break;
    case IQO_KERNEL_LANCZOS_D32: k = iqo_amd::d32_instance(d32_dev(h)); break;
    case IQO_KERNEL_LANCZOS_D31: k = iqo_amd::d31_instance(d31_dev(h)); break;
    case IQO_KERNEL_LANCZOS_U23: k = iqo_amd::u23_instance(u23_dev(h)); break;
    case IQO_KERNEL_LINEAR_U23: k = iqo_amd::l23_instance(l23_dev(h)); break;
    case IQO_KERNEL_AREA_D32: k = iqo_amd::a32_instance(a32_dev(h)); break;
    case IQO_KERNEL_RYX: k = iqo_amd::ryx_instance(ryx_dev(h)); break;
    case IQO_KERNEL_RYG: {
        const iqo_amd::RygDev d = ryg_dev(h);
        k = iqo_amd::ryg_instance(d, d.nl == 1 && h->hasRyu && h->useRyu, d.run);
        break;
    }
    default: {  // a family with one kernel
        *out = iqo_hip_instance{};
        out->family = kernel;
        return IQO_HIP_OK;
    }
    }
    if (!k)
        return IQO_HIP_EINVAL;  // (the launch function rejects the call the same way)
    *out = to_desc(*k);
    return IQO_HIP_OK;
}

iqo_amd::Io make_io(size_t frames, const uint8_t *src, size_t srcSt, size_t srcFrameSt, size_t srcRow0, int srcRowEnd,
                    uint8_t *dst, size_t dstSt, size_t dstFrameSt, int dstRow0)
{
    iqo_amd::Io io;
    io.frames = static_cast<int>(frames);
    io.src = src;
    io.srcSt = static_cast<int64_t>(srcSt);
    io.srcFrameSt = static_cast<int64_t>(srcFrameSt);
    io.srcRow0 = static_cast<int>(srcRow0);
    io.srcRowEnd = srcRowEnd;
    io.dst = dst;
    io.dstSt = static_cast<int64_t>(dstSt);
    io.dstFrameSt = static_cast<int64_t>(dstFrameSt);
    io.dstRow0 = dstRow0;
    return io;
}

// Whether the launcher of `kernel` takes this layout: kernels.hpp layout_ok on the Io that run_band builds
// for output rows [rb, re) of the plan, with the source window [srcRow0, srcRowEnd).  Host arithmetic
// only, so an entry with several planes can ask for all of them before its first launch.
bool layout_accepted(const iqo_hip_plan *h, int kernel, int rb, int re, size_t srcRow0, int srcRowEnd, size_t srcSt,
                     size_t dstSt)
{
    const iqo_amd::Io io = make_io(1, nullptr, srcSt, 0, srcRow0, srcRowEnd, nullptr, dstSt, 0, rb);
    const int64_t C = h->channels;
    int64_t sb, db;
    return iqo_amd::layout_ok(kernel, io, re, h->p.srcW * C, h->p.dstW * C, &sb, &db);
}

// ... of a whole frame of one plane of an I420 / NV12 call.  wholeSource: the window is every source row (the
// fused I420 launch), which contains the rows run_band names
bool plane_layout_accepted(const iqo_hip_plan *h, int kernel, bool wholeSource, size_t srcSt, size_t dstSt)
{
    int s0, s1;
    iqo_amd::band_src_rows(h->p, 0, h->p.dstH, &s0, &s1);
    return layout_accepted(h, kernel, 0, h->p.dstH, 0, wholeSource ? h->p.srcH : s1, srcSt, dstSt);
}

// The one dispatch from a kernel family to its launcher, for output rows [rb, re) of `io`.  query: the
// launcher fills the grid it would launch and launches nothing (kernels.hpp LaunchGrid).
hipError_t launch_family(const iqo_hip_plan *h, int kernel, const iqo_amd::Io &io, int rb, int re, hipStream_t s,
                         iqo_amd::LaunchGrid *query)
{
    switch (kernel) {
    case IQO_KERNEL_LANCZOS_STREAM: return iqo_amd::launch_lanczos_stream(lanczos_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_AREA_INT: return iqo_amd::launch_area_int(area_dev(h), io, rb, re, s, query);
    case IQO_KERNEL_LINEAR_UP2: return iqo_amd::launch_linear_up2(linear_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_TILE: return iqo_amd::launch_tile(tile_dev(h), io, rb, re, s, query);
    case IQO_KERNEL_WALK: return iqo_amd::launch_walk(walk_dev(h), io, rb, re, h->bands, s, 0, -1, 1, query);
    case IQO_KERNEL_LANCZOS_UP2: return iqo_amd::launch_up2(up2_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_LANCZOS_D32: return iqo_amd::launch_d32(d32_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_LANCZOS_D31: return iqo_amd::launch_d31(d31_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_RYX: return iqo_amd::launch_ryx(ryx_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_RYG: {
        iqo_amd::RygDev d = ryg_dev(h);
        if (query) {
            // a plan without device tables yet (host-only, or before the first call): the tables launch_ryg
            // reads its two decisions off stand in as placeholders, which a query never dereferences
            static const int4 kNoTable{};
            if (!d.rowRec)
                d.rowRec = &kNoTable;
            if (d.nl == 1 && h->hasRyu && h->useRyu && !d.posRec)
                d.posRec = &kNoTable;
            if (d.run && !d.colRun)
                d.colRun = reinterpret_cast<const uint32_t *>(&kNoTable);
        }
        return iqo_amd::launch_ryg(d, io, rb, re, h->bands, s, query);
    }
    case IQO_KERNEL_AREA_D32: return iqo_amd::launch_a32(a32_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_LANCZOS_U23: return iqo_amd::launch_u23(u23_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_LINEAR_U23: return iqo_amd::launch_l23(l23_dev(h), io, rb, re, h->bands, s, query);
    case IQO_KERNEL_PACKED_TILE: return iqo_amd::launch_packed_tile(packed_tile_dev(h), h->channels, io, rb, re, s, query);
    case IQO_KERNEL_PACKED_GENERAL: return iqo_amd::launch_packed_general(general_dev(h), h->channels, io, rb, re, s, query);
    default: return iqo_amd::launch_general(general_dev(h), io, rb, re, s, query);
    }
}

// Frames of run_band's first launch: at most 65535 (grid y), fewer with the option "chunk_frames".
size_t frames_per_launch(const iqo_hip_plan *h, size_t nFrames)
{
    size_t chunk = 65535;
    if (h->chunkFrames > 0) {
        chunk = std::min(chunk, static_cast<size_t>(h->chunkFrames));
        const size_t n = (nFrames + chunk - 1) / chunk;  // equal launches, not one straggler
        chunk = (nFrames + n - 1) / n;
    }
    return chunk;
}

// iqo_hip_plan_launch_grid / iqo_host_launch_grid: the grid of the first launch of an aligned, tightly packed
// run_band call of nFrames frames over output rows [r0, r0 + rows), from the launcher itself.
int plan_launch_grid(const iqo_hip_plan *h, size_t nFrames, size_t r0, size_t rows, iqo_hip_launch_grid *out)
{
    static_assert(IQO_GRID_MAP_NONE == iqo_amd::kMapNone && IQO_GRID_MAP_SPREAD == iqo_amd::kMapSpread &&
                      IQO_GRID_MAP_CHUNKS == iqo_amd::kMapChunks && IQO_GRID_MAP_XCD_TAIL == iqo_amd::kMapXcdTail &&
                      IQO_HIP_GRID_STRIDE_BLOCKS == iqo_amd::kGridStrideBlocks,
                  "kernels.hpp kMap* / kGridStrideBlocks are iqo_hip.h's");
    const Plan &p = h->p;
    const size_t dstH = static_cast<size_t>(p.dstH);
    if (r0 > dstH || rows > dstH - r0 || rows == 0 || nFrames == 0)
        return IQO_HIP_EINVAL;
    const int kernel = plan_kernel(h);
    if (!ratio_prefetch_ok(h, kernel))
        return IQO_HIP_EINVAL;
    const int rb = static_cast<int>(r0), re = static_cast<int>(r0 + rows);
    int s0, s1;
    iqo_amd::band_src_rows(p, rb, re, &s0, &s1);
    const size_t C = static_cast<size_t>(h->channels), frames = std::min(frames_per_launch(h, nFrames), nFrames);
    const size_t srcSt = (static_cast<size_t>(p.srcW) * C + 15) & ~size_t(15), dstSt = (static_cast<size_t>(p.dstW) * C + 15) & ~size_t(15);
    const iqo_amd::Io io = make_io(frames, nullptr, srcSt, srcSt * static_cast<size_t>(p.srcH), 0, s1, nullptr, dstSt,
                                   dstSt * dstH, rb);
    iqo_amd::LaunchGrid g;
    const hipError_t e = launch_family(h, kernel, io, rb, re, nullptr, &g);
    if (e == hipErrorNotSupported)
        return IQO_HIP_EUNSUP;
    if (e != hipSuccess)
        return IQO_HIP_EINVAL;
    *out = iqo_hip_launch_grid{};
    out->family = kernel;
    out->map = g.map;
    out->gridX = g.gridX;
    out->gridY = g.gridY;
    out->gridZ = g.gridZ;
    out->block = g.block;
    out->blocks = g.blocks;
    out->chunk = g.chunk;
    out->unitsPerFrame = g.unitsPerFrame;
    out->unitsPerBlock = g.unitsPerBlock;
    out->units = g.units;
    out->bands = g.bands;
    out->wavesPerRow = g.wavesPerRow;
    out->framesPerBlock = g.framesPerBlock;
    out->tailBands = g.tailBands;
    out->frames = static_cast<unsigned>(frames);
    return IQO_HIP_OK;
}

int run_band(iqo_hip_plan *h, size_t nFrames, size_t r0, size_t rows, size_t srcRow0, size_t srcSt,
             size_t srcFrameSt, const uint8_t *src, size_t dstSt, size_t dstFrameSt, uint8_t *dst, hipStream_t s)
{
    const Plan &p = h->p;
    const size_t C = static_cast<size_t>(h->channels);
    if (!src || !dst || srcSt < static_cast<size_t>(p.srcW) * C || dstSt < static_cast<size_t>(p.dstW) * C)
        return IQO_HIP_EINVAL;
    const size_t dstH = static_cast<size_t>(p.dstH);
    if (r0 > dstH || rows > dstH - r0 || srcRow0 >= static_cast<size_t>(p.srcH))
        return IQO_HIP_EINVAL;
    if (rows == 0 || nFrames == 0)
        return IQO_HIP_OK;
    // the window must start at or above the first source row the band reads (iqo_hip_band_src_rows);
    // the kernels read at most up to the window's end s1, never past it
    int s0, s1;
    iqo_amd::band_src_rows(p, static_cast<int>(r0), static_cast<int>(r0 + rows), &s0, &s1);
    if (srcRow0 > static_cast<size_t>(s0))
        return IQO_HIP_EINVAL;
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;

    const int kernel = kernel_for_layout(h, src, srcSt, srcFrameSt, dst, dstSt, dstFrameSt);
    if (kernel == IQO_KERNEL_TILE || kernel == IQO_KERNEL_WALK || kernel == IQO_KERNEL_RYX ||
        kernel == IQO_KERNEL_RYG || kernel == IQO_KERNEL_GENERAL || kernel == IQO_KERNEL_PACKED_TILE ||
        kernel == IQO_KERNEL_PACKED_GENERAL) {
        const int rc = ensure_tables(h);
        if (rc)
            return rc;
    }

    const int rb = static_cast<int>(r0), re = static_cast<int>(r0 + rows);
    // Frames per launch: at most 65535 (grid y).  The option "chunk_frames" splits further into
    // equal launches (measured: no gain on MI355X for C2 at 256 frames, a loss for C3 at 48 --
    // the per-frame slowdown of C2 past ~130 frames per call is not a per-launch effect).
    const size_t chunk = frames_per_launch(h, nFrames);
    if (!ratio_prefetch_ok(h, kernel))
        return IQO_HIP_EINVAL;
    for (size_t f0 = 0; f0 < nFrames; f0 += chunk) {
        const iqo_amd::Io io = make_io(std::min(chunk, nFrames - f0), src + f0 * srcFrameSt, srcSt, srcFrameSt, srcRow0,
                                       s1, dst + f0 * dstFrameSt, dstSt, dstFrameSt, rb);
        const hipError_t e = launch_family(h, kernel, io, rb, re, s, nullptr);
        // the launchers reject a parameter set they have no instantiation for before launching
        // (hipErrorInvalidValue / hipErrorNotSupported): a plan / kernel mismatch, reported as such
        // (the drop-in classes report those on every call instead of falling back for good)
        if (e == hipErrorInvalidValue)
            return IQO_HIP_EINVAL;
        if (e == hipErrorNotSupported)
            return IQO_HIP_EUNSUP;
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return IQO_HIP_OK;
}

// iqo_hip_resize_device_norm: every check runs on the host before the first launch, so a rejected
// call leaves the destination untouched.
int run_norm(iqo_hip_plan *h, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *src,
             const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt, size_t dstFrameSt, void *dst, hipStream_t s)
{
    if (!src || !dst || !norm)
        return IQO_HIP_EINVAL;
    if (h->channels < 2)  // planar plans: sixteen kernel families without the float epilogue
        return IQO_HIP_EUNSUP;
    const Plan &p = h->p;
    const size_t C = static_cast<size_t>(h->channels);
    if (norm->dtype != IQO_OUT_F32 && norm->dtype != IQO_OUT_F16 && norm->dtype != IQO_OUT_BF16)
        return IQO_HIP_EINVAL;
    if (norm->planes < 1 || norm->planes > 4)
        return IQO_HIP_EINVAL;
    for (int i = 0; i < norm->planes; ++i)
        if (norm->order[i] < 0 || norm->order[i] >= h->channels || !std::isfinite(norm->scale[i]) ||
            !std::isfinite(norm->bias[i]))
            return IQO_HIP_EINVAL;
    const size_t elem = norm->dtype == IQO_OUT_F32 ? 4 : 2;
    const size_t dstW = static_cast<size_t>(p.dstW), dstH = static_cast<size_t>(p.dstH);
    const size_t planes = static_cast<size_t>(norm->planes);
    if (reinterpret_cast<uintptr_t>(dst) % elem || dstRowSt % elem || dstPlaneSt % elem || dstFrameSt % elem)
        return IQO_HIP_EINVAL;
    // (divisions: no product of caller-supplied strides can wrap)
    if (srcSt < static_cast<size_t>(p.srcW) * C || dstRowSt < dstW * elem || dstPlaneSt / dstH < dstRowSt ||
        (nFrames > 1 && dstFrameSt / planes < dstPlaneSt))
        return IQO_HIP_EINVAL;
    // the kernels address one float frame with 32-bit byte offsets (launch_packed_tile's limits)
    const size_t kLim = size_t(1) << 31;
    if (dstRowSt >= kLim || dstPlaneSt >= kLim ||
        (planes - 1) * dstPlaneSt + (dstH - 1) * dstRowSt + dstW * elem >= kLim ||
        static_cast<size_t>(p.srcH - 1) * srcSt + static_cast<size_t>(p.srcW) * C >= kLim || srcSt >= (size_t(1) << 24))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    const int rc = ensure_tables(h);
    if (rc)
        return rc;
    const int kernel = plan_kernel(h);
    iqo_amd::NormDev n;
    n.dtype = norm->dtype;
    n.planes = norm->planes;
    n.planeSt = static_cast<int>(dstPlaneSt);
    for (int i = 0; i < 4; ++i) {
        const bool used = i < norm->planes;
        n.order[i] = used ? norm->order[i] : 0;
        n.scale[i] = used ? norm->scale[i] : 0.f;
        n.bias[i] = used ? norm->bias[i] : 0.f;
    }
    int s0, s1;  // the source rows a full frame reads, as run_band
    iqo_amd::band_src_rows(p, 0, p.dstH, &s0, &s1);
    const size_t chunk = 65535;  // frames per launch (grid y of the general kernel)
    for (size_t f0 = 0; f0 < nFrames; f0 += chunk) {
        const iqo_amd::Io io = make_io(std::min(chunk, nFrames - f0), src + f0 * srcFrameSt, srcSt, srcFrameSt, 0, s1,
                                       static_cast<uint8_t *>(dst) + f0 * dstFrameSt, dstRowSt, dstFrameSt, 0);
        const hipError_t e = kernel == IQO_KERNEL_PACKED_TILE
                                 ? iqo_amd::launch_packed_tile_norm(packed_tile_dev(h), h->channels, io, n, 0, p.dstH, s)
                                 : iqo_amd::launch_packed_general_norm(general_dev(h), h->channels, io, n, 0, p.dstH, s);
        if (e == hipErrorInvalidValue)
            return IQO_HIP_EINVAL;
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return IQO_HIP_OK;
}

} // namespace

extern "C" {

int iqo_hip_available(void)
{
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess)
        return 0;
    int n = 0;
    for (int d = 0; d < count; ++d)
        n += is_gfx950(d) ? 1 : 0;
    return n;
}

int iqo_hip_plan_lanczos(unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale,
                         int device, iqo_hip_plan **out)
{
    return make_plan(iqo_amd::kLanczos, degree, srcW, srcH, dstW, dstH, pxScale, device, out);
}

int iqo_hip_plan_area(size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device, iqo_hip_plan **out)
{
    return make_plan(iqo_amd::kArea, 0, srcW, srcH, dstW, dstH, 1, device, out);
}

int iqo_hip_plan_linear(size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device, iqo_hip_plan **out)
{
    return make_plan(iqo_amd::kLinear, 0, srcW, srcH, dstW, dstH, 1, device, out);
}

int iqo_hip_plan_packed(int method, unsigned degree, int channels, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                        size_t pxScale, int device, iqo_hip_plan **out)
{
    if (method < IQO_METHOD_LANCZOS || method > IQO_METHOD_LINEAR || channels < 1 || channels > 4) {
        if (out)
            *out = nullptr;
        return IQO_HIP_EINVAL;
    }
    const bool lz = method == IQO_METHOD_LANCZOS;  // degree / pxScale: Lanczos only (as the planar constructors)
    return make_plan(static_cast<iqo_amd::Method>(method), lz ? degree : 0, srcW, srcH, dstW, dstH, lz ? pxScale : 1,
                     device, out, channels);
}

int iqo_hip_plan_channels(const iqo_hip_plan *plan) { return plan ? plan->channels : IQO_HIP_EINVAL; }

void iqo_hip_plan_destroy(iqo_hip_plan *plan)
{
    if (!plan)
        return;
    plan_cache_put(plan);  // kept for an identical request (make_plan), or freed when evicted
}

int iqo_hip_plan_query(const iqo_hip_plan *h, iqo_hip_plan_desc *d)
{
    if (!h || !d)
        return IQO_HIP_EINVAL;
    d->method = h->p.method;
    d->device = h->device;
    d->srcW = static_cast<size_t>(h->p.srcW);
    d->srcH = static_cast<size_t>(h->p.srcH);
    d->dstW = static_cast<size_t>(h->p.dstW);
    d->dstH = static_cast<size_t>(h->p.dstH);
    d->tapsX = h->p.x.taps;
    d->tapsY = h->p.y.taps;
    d->phasesX = h->p.x.phases;
    d->phasesY = h->p.y.phases;
    d->kernel = plan_kernel(h);
    d->bandsPerFrame = h->bands;
    d->tileRows = h->channels > 1 ? (h->pk.ok ? h->pk.TH : 0) : h->tt.ok ? h->tt.TH : 0;
    return IQO_HIP_OK;
}

int iqo_hip_plan_instance(const iqo_hip_plan *h, size_t srcAlign, size_t dstAlign, iqo_hip_instance *desc)
{
    if (!h || !desc || !valid_align(srcAlign) || !valid_align(dstAlign))
        return IQO_HIP_EINVAL;
    return plan_instance(h, Layout{srcAlign, dstAlign}, desc);
}

int iqo_hip_plan_launch_grid(const iqo_hip_plan *h, size_t nFrames, size_t dstRow0, size_t dstRows, iqo_hip_launch_grid *desc)
{
    if (!h || !desc)
        return IQO_HIP_EINVAL;
    DeviceGuard guard(h->device);  // (the automatic band counts ask the plan's device for its occupancy)
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    return plan_launch_grid(h, nFrames, dstRow0, dstRows, desc);
}

int iqo_hip_plan_prepare(iqo_hip_plan *h)
{
    if (!h)
        return IQO_HIP_EINVAL;
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    return ensure_tables(h);
}

// The A/B keys (kOptions rows that are not public, and the three keys handled below) are accepted
// only with IQO_HIP_TUNING=1 in the environment -- tests, bench.py --option and the tuning scripts
// set it; a caller of the public ABI sees force_general, bands and host_stage only (include/iqo_hip.h).
bool tuning_enabled()
{
    const char *e = std::getenv("IQO_HIP_TUNING");
    return e && *e && std::strcmp(e, "0") != 0;
}

int iqo_hip_plan_set_option(iqo_hip_plan *h, const char *key, long value)
{
    if (!h || !key)
        return IQO_HIP_EINVAL;
    const Option *o = std::find_if(std::begin(kOptions), std::end(kOptions),
                                   [&](const Option &r) { return !std::strcmp(key, r.name); });
    const bool known = o != std::end(kOptions);
    if (!(known && o->pub) && !tuning_enabled())
        return IQO_HIP_EINVAL;
    if (known) {
        const bool onoff = o->lo > o->hi;
        if (!onoff && (value < o->lo || value > o->hi))
            return IQO_HIP_EINVAL;
        if (o->member == &iqo_hip_plan::rygCpt && value == 1)  // (0 auto, 2, 3, 4)
            return IQO_HIP_EINVAL;
        h->*o->member = onoff ? value != 0 : static_cast<int>(value);
        return IQO_HIP_OK;
    }
#ifdef IQO_VARIANT_DEBUG
    if (!std::strcmp(key, "debug_flags")) {  // variant builds only: timing experiments, wrong results
        h->debugFlags = static_cast<int>(value);
        return IQO_HIP_OK;
    }
    if (!std::strcmp(key, "trace_addr")) {  // variant builds only: device buffer of 16 B per workgroup
        h->traceAddr = static_cast<uint64_t>(value);
        return IQO_HIP_OK;
    }
#endif
    if (!std::strcmp(key, "tile_rows")) {  // output rows per tile of the tile kernel (0 = auto)
        iqo_amd::TileTables t = h->tt;
        if (!t.ok)
            return IQO_HIP_EUNSUP;
        if (value == 0) {
            iqo_amd::build_tile_tables(h->p, &t);
        } else if (!iqo_amd::tile_set_rows(h->p, &t, static_cast<int>(value))) {
            return IQO_HIP_EINVAL;
        }
        h->tt.TH = t.TH;
        h->tt.srcRows = t.srcRows;
        return IQO_HIP_OK;
    }
    return IQO_HIP_EINVAL;
}

int iqo_hip_resize_device(iqo_hip_plan *h, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                          size_t dstSt, size_t dstFrameSt, uint8_t *dDst, void *stream)
{
    if (!h)
        return IQO_HIP_EINVAL;
    return run_band(h, nFrames, 0, static_cast<size_t>(h->p.dstH), 0, srcSt, srcFrameSt, dSrc, dstSt, dstFrameSt,
                    dDst, static_cast<hipStream_t>(stream));
}

int iqo_hip_resize_device_norm(iqo_hip_plan *h, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                               const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt, size_t dstFrameSt,
                               void *dDst, void *stream)
{
    if (!h)
        return IQO_HIP_EINVAL;
    return run_norm(h, nFrames, srcSt, srcFrameSt, dSrc, norm, dstRowSt, dstPlaneSt, dstFrameSt, dDst,
                    static_cast<hipStream_t>(stream));
}

int iqo_hip_band_src_rows(const iqo_hip_plan *h, size_t dstRow0, size_t dstRows, size_t *srcRow0, size_t *srcRows)
{
    if (!h || !srcRow0 || !srcRows || dstRow0 + dstRows > static_cast<size_t>(h->p.dstH))
        return IQO_HIP_EINVAL;
    int s0, s1;
    iqo_amd::band_src_rows(h->p, static_cast<int>(dstRow0), static_cast<int>(dstRow0 + dstRows), &s0, &s1);
    *srcRow0 = static_cast<size_t>(s0);
    *srcRows = static_cast<size_t>(s1 - s0);
    return IQO_HIP_OK;
}

int iqo_hip_resize_band(iqo_hip_plan *h, size_t nFrames, size_t dstRow0, size_t dstRows, size_t srcRow0, size_t srcSt,
                        size_t srcFrameSt, const uint8_t *dSrcWindow, size_t dstSt, size_t dstFrameSt, uint8_t *dDstBand,
                        void *stream)
{
    if (!h)
        return IQO_HIP_EINVAL;
    return run_band(h, nFrames, dstRow0, dstRows, srcRow0, srcSt, srcFrameSt, dSrcWindow, dstSt, dstFrameSt,
                    dDstBand, static_cast<hipStream_t>(stream));
}

// The host-pointer drop-in (reference resize(), LanczosResizer.hpp:47-52 semantics: synchronous,
// host buffers).  Output-row bands are pipelined over three streams: band b's new source rows go
// up on sIn, its kernel runs on sK once they have landed, its output rows come down on sOut, so
// the H2D of band b+1, the kernel of band b and the D2H of band b-1 overlap (PCIe is full
// duplex).  Pinned host buffers are DMA'd in place; pageable ones are staged through pinned
// memory by the calling thread one band ahead of the copy engines.
// One plane of a host-pointer call: the user's buffers and the plane's place in the staging set
// (device and pinned staging at byte offsets sOff / dOff, row pitches sPitch / dPitch; pinSrc /
// pinDst: the user buffer is pinned and DMA'd in place).
struct HostPlane {
    iqo_hip_plan *h;
    size_t srcSt;
    const uint8_t *src;
    size_t dstSt;
    uint8_t *dst;
    size_t sOff, dOff, sPitch, dPitch;
    bool pinSrc, pinDst;
};

// The host-pointer pipeline over one or more planes (the I420 planes of one call share it): each
// plane is cut into output-row bands, and chunk c = (plane, band) goes through
//   stage its new source rows into pinned memory (the copy pool) -> H2D (two upload streams,
//   alternating chunks: two SDMA queues) -> the plane's kernel on its band (sK, after the chunk's
//   uploads) -> D2H of the band (sOut) -> unstage into the user's rows,
// so the host staging of chunk c + 1 overlaps the upload of chunk c, and every plane's transfers
// overlap the other planes' instead of each plane paying a synchronous round trip.
int host_pipeline(HostStage *st, HostPlane *planes, int nPlanes)
{
    struct Chunk {
        int plane, r0, r1;
    };
    Chunk ch[kHostChunks];
    int nc = 0;
    for (int q = 0; q < nPlanes; ++q) {
        const int dstH = planes[q].h->p.dstH;
        const int maxBands = nPlanes == 1 ? kHostBands : q == 0 ? kHostBands / 2 : kHostBands / 4;
        const int bands = std::max(1, std::min(maxBands, dstH / kHostBandRows));
        for (int b = 0; b < bands && nc < kHostChunks; ++b)
            ch[nc++] = Chunk{q, static_cast<int>(static_cast<int64_t>(dstH) * b / bands),
                             static_cast<int>(static_cast<int64_t>(dstH) * (b + 1) / bands)};
    }
    int rowsUp[4] = {0, 0, 0, 0};  // per plane: source rows [0, rowsUp) are queued for upload
    int lastUp[4] = {-1, -1, -1, -1};  // per plane: the chunk that queued the latest upload
    for (int c = 0; c < nc; ++c) {
        HostPlane &P = planes[ch[c].plane];
        const Plan &p = P.h->p;
        const size_t C = static_cast<size_t>(P.h->channels);  // rows of width * channels bytes
        const size_t W = static_cast<size_t>(p.srcW) * C, w = static_cast<size_t>(p.dstW) * C;
        int s0, s1;
        iqo_amd::band_src_rows(p, ch[c].r0, ch[c].r1, &s0, &s1);
        const bool lastOfPlane = c == nc - 1 || ch[c + 1].plane != ch[c].plane;
        if (lastOfPlane)
            s1 = p.srcH;
        int &up = rowsUp[ch[c].plane];
        const int prevUp = lastUp[ch[c].plane];
        hipStream_t sUp = (c & 1) ? st->sIn2 : st->sIn;
        if (s1 > up) {
            const size_t n = static_cast<size_t>(s1 - up);
            const uint8_t *from = P.src + static_cast<size_t>(up) * P.srcSt;
            size_t fromSt = P.srcSt;
            if (!P.pinSrc) {
                uint8_t *pin = st->hSrc + P.sOff + static_cast<size_t>(up) * P.sPitch;
                copy_rows_par(pin, P.sPitch, from, P.srcSt, W, n);
                from = pin;
                fromSt = P.sPitch;
            }
            if (hipMemcpy2DAsync(st->dSrc + P.sOff + static_cast<size_t>(up) * P.sPitch, P.sPitch, from, fromSt, W, n,
                                 hipMemcpyHostToDevice, sUp) != hipSuccess)
                return IQO_HIP_EHIP;
            up = s1;
            lastUp[ch[c].plane] = c;
        }
        // the band's rows: this chunk's upload, and the halo rows the plane's previous upload brought
        if (hipEventRecord(st->evIn[c], sUp) != hipSuccess || hipStreamWaitEvent(st->sK, st->evIn[c], 0) != hipSuccess ||
            (prevUp >= 0 && prevUp != c && hipStreamWaitEvent(st->sK, st->evIn[prevUp], 0) != hipSuccess))
            return IQO_HIP_EHIP;
        const size_t rows = static_cast<size_t>(ch[c].r1 - ch[c].r0);
        const size_t sBytes = P.sPitch * static_cast<size_t>(p.srcH), dBytes = P.dPitch * static_cast<size_t>(p.dstH);
        int rc = run_band(P.h, 1, static_cast<size_t>(ch[c].r0), rows, 0, P.sPitch, sBytes, st->dSrc + P.sOff, P.dPitch,
                          dBytes, st->dDst + P.dOff + static_cast<size_t>(ch[c].r0) * P.dPitch, st->sK);
        if (rc)
            return rc;
        if (hipEventRecord(st->evK[c], st->sK) != hipSuccess || hipStreamWaitEvent(st->sOut, st->evK[c], 0) != hipSuccess)
            return IQO_HIP_EHIP;
        uint8_t *to = P.pinDst ? P.dst + static_cast<size_t>(ch[c].r0) * P.dstSt
                               : st->hDst + P.dOff + static_cast<size_t>(ch[c].r0) * P.dPitch;
        if (hipMemcpy2DAsync(to, P.pinDst ? P.dstSt : P.dPitch, st->dDst + P.dOff + static_cast<size_t>(ch[c].r0) * P.dPitch,
                             P.dPitch, w, rows, hipMemcpyDeviceToHost, st->sOut) != hipSuccess ||
            hipEventRecord(st->evOut[c], st->sOut) != hipSuccess)
            return IQO_HIP_EHIP;
    }
    // output bands leave the pinned staging as they land
    for (int c = 0; c < nc; ++c) {
        if (hipEventSynchronize(st->evOut[c]) != hipSuccess)
            return IQO_HIP_EHIP;
        const HostPlane &P = planes[ch[c].plane];
        if (!P.pinDst)
            copy_rows_par(P.dst + static_cast<size_t>(ch[c].r0) * P.dstSt, P.dstSt,
                          st->hDst + P.dOff + static_cast<size_t>(ch[c].r0) * P.dPitch, P.dPitch,
                          static_cast<size_t>(P.h->p.dstW) * static_cast<size_t>(P.h->channels),
                          static_cast<size_t>(ch[c].r1 - ch[c].r0));
    }
    return IQO_HIP_OK;
}

// Large frames, the default: whole-plane copies straight from the user's buffers (pageable ones
// through the HIP runtime's own staging, which runs at close to the PCIe rate: 44 GB/s H2D for a
// 12 MB plane set against 53 GB/s from pinned memory, profiles/r05/pcie_probe.json), every plane's
// upload first, then the kernels, then the downloads, one stream, one synchronisation.  Our own
// banded staging pipeline (host_pipeline: pool memcpy into pinned memory + DMA per band, option
// host_stage = 1) spent more host time on its per-band copies, events and launches than the
// transfers take: C2 Y 0.43 -> 0.24 ms from pageable memory, I420 0.58 -> 0.42 ms; from pinned
// buffers the pipeline took 0.33 / 0.38 ms (profiles/r05/host_latency.txt).
int host_direct(HostStage *st, HostPlane *planes, int nPlanes)
{
    for (int q = 0; q < nPlanes; ++q) {
        const HostPlane &P = planes[q];
        const Plan &p = P.h->p;
        const size_t W = static_cast<size_t>(p.srcW) * static_cast<size_t>(P.h->channels), H = static_cast<size_t>(p.srcH);
        const hipError_t e = (P.srcSt == W && P.sPitch == W)
                                 ? hipMemcpyAsync(st->dSrc + P.sOff, P.src, W * H, hipMemcpyHostToDevice, st->sK)
                                 : hipMemcpy2DAsync(st->dSrc + P.sOff, P.sPitch, P.src, P.srcSt, W, H,
                                                    hipMemcpyHostToDevice, st->sK);
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    for (int q = 0; q < nPlanes; ++q) {
        const HostPlane &P = planes[q];
        const Plan &p = P.h->p;
        const size_t sBytes = P.sPitch * static_cast<size_t>(p.srcH), dBytes = P.dPitch * static_cast<size_t>(p.dstH);
        const int rc = run_band(P.h, 1, 0, static_cast<size_t>(p.dstH), 0, P.sPitch, sBytes, st->dSrc + P.sOff, P.dPitch,
                                dBytes, st->dDst + P.dOff, st->sK);
        if (rc)
            return rc;
    }
    for (int q = 0; q < nPlanes; ++q) {
        const HostPlane &P = planes[q];
        const Plan &p = P.h->p;
        const size_t w = static_cast<size_t>(p.dstW) * static_cast<size_t>(P.h->channels), hh = static_cast<size_t>(p.dstH);
        const hipError_t e = (P.dstSt == w && P.dPitch == w)
                                 ? hipMemcpyAsync(P.dst, st->dDst + P.dOff, w * hh, hipMemcpyDeviceToHost, st->sK)
                                 : hipMemcpy2DAsync(P.dst, P.dstSt, st->dDst + P.dOff, P.dPitch, w, hh,
                                                    hipMemcpyDeviceToHost, st->sK);
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return hipStreamSynchronize(st->sK) == hipSuccess ? IQO_HIP_OK : IQO_HIP_EHIP;
}

static int host_resize(iqo_hip_plan *h, HostStage *st, size_t srcSt, const uint8_t *src, size_t dstSt, uint8_t *dst)
{
    const Plan &p = h->p;
    const size_t C = static_cast<size_t>(h->channels);  // staged rows: width * channels bytes
    const size_t W = static_cast<size_t>(p.srcW) * C, w = static_cast<size_t>(p.dstW) * C;
    const size_t sPitch = (W + 15) & ~size_t(15);
    const size_t dPitch = (w + 15) & ~size_t(15);
    const size_t sBytes = sPitch * p.srcH, dBytes = dPitch * p.dstH;
    if (grow_device(&st->dSrc, &st->dSrcCap, sBytes) || grow_device(&st->dDst, &st->dDstCap, dBytes))
        return IQO_HIP_ENOMEM;
    // small frames are always staged: the pinned-memory queries cost more than the copy
    const bool small = sBytes < kHostPipeMinBytes;
    const bool pinSrc = !small && is_pinned_host(src), pinDst = !small && is_pinned_host(dst);
    // pinned staging: the small-frame path and the banded pipeline (host_stage = 1) use it; the
    // default large-frame path (host_direct) copies straight from the caller's buffers
    const bool staged = small || h->hostStage;
    if (staged && !pinSrc && grow_pinned(&st->hSrc, &st->hSrcCap, sBytes))
        return IQO_HIP_ENOMEM;
    if (staged && !pinDst && grow_pinned(&st->hDst, &st->hDstCap, dBytes))
        return IQO_HIP_ENOMEM;

    const int dstH = p.dstH;
    if (small) {
        // small frame: upload, kernel and download in order on one stream, one synchronisation
        // (the pipeline's events and cross-stream waits cost more than they overlap here)
        const uint8_t *from = src;
        size_t fromSt = srcSt;
        if (!pinSrc) {
            copy_rows_par(st->hSrc, sPitch, src, srcSt, W, static_cast<size_t>(p.srcH));
            from = st->hSrc;
            fromSt = sPitch;
        }
        if (hipMemcpy2DAsync(st->dSrc, sPitch, from, fromSt, W, static_cast<size_t>(p.srcH), hipMemcpyHostToDevice,
                             st->sK) != hipSuccess)
            return IQO_HIP_EHIP;
        int rc = run_band(h, 1, 0, static_cast<size_t>(dstH), 0, sPitch, sBytes, st->dSrc, dPitch, dBytes, st->dDst,
                          st->sK);
        if (rc)
            return rc;
        uint8_t *to = pinDst ? dst : st->hDst;
        if (hipMemcpy2DAsync(to, pinDst ? dstSt : dPitch, st->dDst, dPitch, w, static_cast<size_t>(dstH),
                             hipMemcpyDeviceToHost, st->sK) != hipSuccess ||
            hipStreamSynchronize(st->sK) != hipSuccess)
            return IQO_HIP_EHIP;
        if (!pinDst)
            copy_rows_par(dst, dstSt, st->hDst, dPitch, w, static_cast<size_t>(dstH));
        return IQO_HIP_OK;
    }
    HostPlane pl{h, srcSt, src, dstSt, dst, 0, 0, sPitch, dPitch, pinSrc, pinDst};
    return h->hostStage ? host_pipeline(st, &pl, 1) : host_direct(st, &pl, 1);
}

int iqo_hip_resize(iqo_hip_plan *h, size_t srcSt, const uint8_t *src, size_t dstSt, uint8_t *dst)
{
    if (!h || !src || !dst)
        return IQO_HIP_EINVAL;
    const Plan &p = h->p;
    const size_t C = static_cast<size_t>(h->channels);
    if (srcSt < static_cast<size_t>(p.srcW) * C || dstSt < static_cast<size_t>(p.dstW) * C)
        return IQO_HIP_EINVAL;
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    HostStage *st = acquire_stage(h->device);
    if (!st)
        return IQO_HIP_EHIP;
    int rc = host_resize(h, st, srcSt, src, dstSt, dst);
    if (rc) {
        // leave nothing in flight on the staging set before it goes back to the pool
        (void)hipStreamSynchronize(st->sIn);
        (void)hipStreamSynchronize(st->sIn2);
        (void)hipStreamSynchronize(st->sK);
        (void)hipStreamSynchronize(st->sOut);
    }
    release_stage(st);
    return rc;
}

// ---- YUV 4:2:0 (I420): the reference benchmark's three-plane workload (benchmark.cpp:131-229)

struct iqo_hip_yuv_plan {
    iqo_hip_plan *y = nullptr, *c = nullptr;  // luma plan, chroma plan (shared by U and V)
    iqo_hip_plan *cf = nullptr;               // full-grid chroma plan (iqo_hip_yuv_plan_set_chroma), shared likewise
    int chroma = IQO_CHROMA_REPLICATE;        // of the RGB / norm entries
};

// The full-grid chroma plan of IQO_CHROMA_FULL under the luma plan hy: srcW/2 x srcH/2 -> dstW x dstH at
// pxScale 1, `channels` 1 (I420) or 2 (NV12).  chroma_full_status: what rules a shape out before any
// plan is built.
static int chroma_full_status(int method, size_t srcW, size_t srcH, size_t dstW, size_t dstH)
{
    // Linear above 2x has no pinned answer (README, "Shapes without a pinned answer")
    if (method == IQO_METHOD_LINEAR && (dstW > 2 * (srcW / 2) || dstH > 2 * (srcH / 2)))
        return IQO_HIP_EUNSUP;
    return IQO_HIP_OK;
}

static int chroma_full_plan(const iqo_hip_plan *hy, int channels, iqo_hip_plan **out)
{
    const Plan &p = hy->p;
    const size_t sw = static_cast<size_t>(p.srcW), sh = static_cast<size_t>(p.srcH);
    const size_t dw = static_cast<size_t>(p.dstW), dh = static_cast<size_t>(p.dstH);
    const int rc = chroma_full_status(static_cast<int>(p.method), sw, sh, dw, dh);
    if (rc)
        return rc;
    return iqo_hip_plan_packed(static_cast<int>(p.method), p.degree, channels, sw / 2, sh / 2, dw, dh, 1, hy->device, out);
}

// iqo_hip_{nv12,yuv}_plan_set_chroma on the plan's three members
static int set_chroma(const iqo_hip_plan *hy, int channels, iqo_hip_plan **cf, int *chroma, int mode)
{
    if (mode != IQO_CHROMA_REPLICATE && mode != IQO_CHROMA_FULL)
        return IQO_HIP_EINVAL;
    if (mode == IQO_CHROMA_FULL && !*cf) {
        const int rc = chroma_full_plan(hy, channels, cf);
        if (rc)
            return rc;
    }
    *chroma = mode;
    return IQO_HIP_OK;
}

int iqo_hip_plan_yuv420(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device,
                        iqo_hip_yuv_plan **out)
{
    if (!out)
        return IQO_HIP_EINVAL;
    *out = nullptr;
    if (srcW < 2 || srcH < 2 || dstW < 2 || dstH < 2)
        return IQO_HIP_EINVAL;
    iqo_hip_yuv_plan *yp = new (std::nothrow) iqo_hip_yuv_plan();
    if (!yp)
        return IQO_HIP_ENOMEM;
    int rc = IQO_HIP_EINVAL;
    if (method == IQO_METHOD_LANCZOS) {
        // chroma: pxScale 2 (benchmark.cpp:222, sample/resize_yuv420p.cpp:159)
        rc = iqo_hip_plan_lanczos(degree, srcW, srcH, dstW, dstH, 1, device, &yp->y);
        if (!rc)
            rc = iqo_hip_plan_lanczos(degree, srcW / 2, srcH / 2, dstW / 2, dstH / 2, 2, device, &yp->c);
    } else if (method == IQO_METHOD_AREA) {
        rc = iqo_hip_plan_area(srcW, srcH, dstW, dstH, device, &yp->y);
        if (!rc)
            rc = iqo_hip_plan_area(srcW / 2, srcH / 2, dstW / 2, dstH / 2, device, &yp->c);
    } else if (method == IQO_METHOD_LINEAR) {
        rc = iqo_hip_plan_linear(srcW, srcH, dstW, dstH, device, &yp->y);
        if (!rc)
            rc = iqo_hip_plan_linear(srcW / 2, srcH / 2, dstW / 2, dstH / 2, device, &yp->c);
    }
    if (rc) {
        iqo_hip_yuv_plan_destroy(yp);
        return rc;
    }
    *out = yp;
    return IQO_HIP_OK;
}

void iqo_hip_yuv_plan_destroy(iqo_hip_yuv_plan *yp)
{
    if (!yp)
        return;
    iqo_hip_plan_destroy(yp->y);
    iqo_hip_plan_destroy(yp->c);
    iqo_hip_plan_destroy(yp->cf);
    delete yp;
}

iqo_hip_plan *iqo_hip_yuv_plane(iqo_hip_yuv_plan *yp, int plane)
{
    if (!yp)
        return nullptr;
    return plane == 0 ? yp->y : plane == 1 ? yp->c : plane == 2 ? yp->cf : nullptr;
}

int iqo_hip_yuv_plan_set_chroma(iqo_hip_yuv_plan *yp, int mode)
{
    if (!yp || !yp->y)
        return IQO_HIP_EINVAL;
    return set_chroma(yp->y, 1, &yp->cf, &yp->chroma, mode);
}

int iqo_hip_yuv_plan_chroma(const iqo_hip_yuv_plan *yp) { return yp ? yp->chroma : IQO_HIP_EINVAL; }

int iqo_hip_resize_yuv420_device(iqo_hip_yuv_plan *yp, size_t nFrames, size_t srcStY, size_t srcStUV,
                                 size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                 size_t dstStY, size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstU,
                                 uint8_t *dstV, void *stream, int *fused)
{
    if (fused)
        *fused = 0;
    if (!yp || !yp->y || !yp->c || !srcY || !srcU || !srcV || !dstY || !dstU || !dstV)
        return IQO_HIP_EINVAL;
    iqo_hip_plan *hy = yp->y, *hc = yp->c;
    const Plan &py = hy->p, &pc = hc->p;
    if (srcStY < static_cast<size_t>(py.srcW) || dstStY < static_cast<size_t>(py.dstW) ||
        srcStUV < static_cast<size_t>(pc.srcW) || dstStUV < static_cast<size_t>(pc.dstW))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;
    DeviceGuard guard(hy->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const int ky = kernel_for_layout(hy, srcY, srcStY, srcFrameSt, dstY, dstStY, dstFrameSt);
    const int ku = kernel_for_layout(hc, srcU, srcStUV, srcFrameSt, dstU, dstStUV, dstFrameSt);
    const int kv = kernel_for_layout(hc, srcV, srcStUV, srcFrameSt, dstV, dstStUV, dstFrameSt);
    const bool fusable = ky == ku && ku == kv &&
                         (ky == IQO_KERNEL_LANCZOS_STREAM || ky == IQO_KERNEL_AREA_INT || ky == IQO_KERNEL_LINEAR_UP2);
    // every plane's layout against its launcher's limits before the first launch: a rejected chroma plane
    // must not leave a written Y plane behind
    if (!plane_layout_accepted(hy, ky, fusable, srcStY, dstStY) || !plane_layout_accepted(hc, ku, fusable, srcStUV, dstStUV) ||
        !plane_layout_accepted(hc, kv, fusable, srcStUV, dstStUV))
        return IQO_HIP_EINVAL;
    if (fusable) {
        // frames per launch: as run_band
        size_t chunk = std::min<size_t>(65535, hy->chunkFrames > 0 ? static_cast<size_t>(hy->chunkFrames) : 65535);
        const size_t n = (nFrames + chunk - 1) / chunk;
        chunk = (nFrames + n - 1) / n;
        hipError_t e = hipSuccess;
        for (size_t f0 = 0; f0 < nFrames && e == hipSuccess; f0 += chunk) {
            const size_t nf = std::min(chunk, nFrames - f0), so = f0 * srcFrameSt, dof = f0 * dstFrameSt;
            const iqo_amd::Io iy = make_io(nf, srcY + so, srcStY, srcFrameSt, 0, py.srcH, dstY + dof, dstStY, dstFrameSt, 0);
            const iqo_amd::Io iu = make_io(nf, srcU + so, srcStUV, srcFrameSt, 0, pc.srcH, dstU + dof, dstStUV, dstFrameSt, 0);
            const iqo_amd::Io iv = make_io(nf, srcV + so, srcStUV, srcFrameSt, 0, pc.srcH, dstV + dof, dstStUV, dstFrameSt, 0);
            if (ky == IQO_KERNEL_LANCZOS_STREAM)
                e = iqo_amd::launch_yuv420_lanczos(lanczos_dev(hy), iy, lanczos_dev(hc), iu, iv, s);
            else if (ky == IQO_KERNEL_AREA_INT)
                e = iqo_amd::launch_yuv420_area(area_dev(hy), iy, area_dev(hc), iu, iv, s);
            else
                e = iqo_amd::launch_yuv420_linear(linear_dev(hy), iy, linear_dev(hc), iu, iv, s);
        }
        if (e == hipSuccess) {
            if (fused)
                *fused = 1;
            return IQO_HIP_OK;
        }
        if (e == hipErrorInvalidValue)  // a launcher's own rejection, made before it launches: as run_band
            return IQO_HIP_EINVAL;
        if (e != hipErrorNotSupported)
            return IQO_HIP_EHIP;
        (void)hipGetLastError();
    }
    // plane by plane
    int rc = run_band(hy, nFrames, 0, static_cast<size_t>(py.dstH), 0, srcStY, srcFrameSt, srcY, dstStY, dstFrameSt,
                      dstY, s);
    if (!rc)
        rc = run_band(hc, nFrames, 0, static_cast<size_t>(pc.dstH), 0, srcStUV, srcFrameSt, srcU, dstStUV, dstFrameSt,
                      dstU, s);
    if (!rc)
        rc = run_band(hc, nFrames, 0, static_cast<size_t>(pc.dstH), 0, srcStUV, srcFrameSt, srcV, dstStUV, dstFrameSt,
                      dstV, s);
    return rc;
}

// ---- NV12: a planar Y plane and one interleaved UV plane at half size.  Y keeps the planar plan and
// all its kernels; UV is a 2-channel packed plan (Lanczos chroma: pxScale 2, as iqo_hip_plan_yuv420).

struct iqo_hip_nv12_plan {
    iqo_hip_plan *y = nullptr, *uv = nullptr;
    iqo_hip_plan *uvf = nullptr;         // full-grid UV plan (iqo_hip_nv12_plan_set_chroma)
    int chroma = IQO_CHROMA_REPLICATE;   // of the RGB / norm entries
};

int iqo_hip_plan_nv12(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, int device,
                      iqo_hip_nv12_plan **out)
{
    if (!out)
        return IQO_HIP_EINVAL;
    *out = nullptr;
    if (srcW < 2 || srcH < 2 || dstW < 2 || dstH < 2)
        return IQO_HIP_EINVAL;
    iqo_hip_nv12_plan *np = new (std::nothrow) iqo_hip_nv12_plan();
    if (!np)
        return IQO_HIP_ENOMEM;
    int rc = iqo_hip_plan_packed(method, degree, 1, srcW, srcH, dstW, dstH, 1, device, &np->y);
    if (!rc)
        rc = iqo_hip_plan_packed(method, degree, 2, srcW / 2, srcH / 2, dstW / 2, dstH / 2, 2, device, &np->uv);
    if (rc) {
        iqo_hip_nv12_plan_destroy(np);
        return rc;
    }
    *out = np;
    return IQO_HIP_OK;
}

void iqo_hip_nv12_plan_destroy(iqo_hip_nv12_plan *np)
{
    if (!np)
        return;
    iqo_hip_plan_destroy(np->y);
    iqo_hip_plan_destroy(np->uv);
    iqo_hip_plan_destroy(np->uvf);
    delete np;
}

iqo_hip_plan *iqo_hip_nv12_plane(iqo_hip_nv12_plan *np, int plane)
{
    if (!np)
        return nullptr;
    return plane == 0 ? np->y : plane == 1 ? np->uv : plane == 2 ? np->uvf : nullptr;
}

int iqo_hip_nv12_plan_set_chroma(iqo_hip_nv12_plan *np, int mode)
{
    if (!np || !np->y)
        return IQO_HIP_EINVAL;
    return set_chroma(np->y, 2, &np->uvf, &np->chroma, mode);
}

int iqo_hip_nv12_plan_chroma(const iqo_hip_nv12_plan *np) { return np ? np->chroma : IQO_HIP_EINVAL; }

int iqo_hip_resize_nv12_device(iqo_hip_nv12_plan *np, size_t nFrames, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                               const uint8_t *srcY, const uint8_t *srcUV, size_t dstStY, size_t dstStUV,
                               size_t dstFrameSt, uint8_t *dstY, uint8_t *dstUV, void *stream)
{
    if (!np || !np->y || !np->uv)
        return IQO_HIP_EINVAL;
    // both planes' pointers, strides and layouts before the first launch: a rejected UV plane must not
    // leave a written Y plane behind
    iqo_hip_plan *hy = np->y, *huv = np->uv;
    if (!srcY || !srcUV || !dstY || !dstUV || srcStY < static_cast<size_t>(hy->p.srcW) ||
        dstStY < static_cast<size_t>(hy->p.dstW) || srcStUV < 2 * static_cast<size_t>(huv->p.srcW) ||
        dstStUV < 2 * static_cast<size_t>(huv->p.dstW))
        return IQO_HIP_EINVAL;
    if (!plane_layout_accepted(hy, kernel_for_layout(hy, srcY, srcStY, srcFrameSt, dstY, dstStY, dstFrameSt), false, srcStY,
                               dstStY) ||
        !plane_layout_accepted(huv, kernel_for_layout(huv, srcUV, srcStUV, srcFrameSt, dstUV, dstStUV, dstFrameSt), false,
                               srcStUV, dstStUV))
        return IQO_HIP_EINVAL;
    // two launches on the same stream
    hipStream_t s = static_cast<hipStream_t>(stream);
    int rc = run_band(np->y, nFrames, 0, static_cast<size_t>(np->y->p.dstH), 0, srcStY, srcFrameSt, srcY, dstStY,
                      dstFrameSt, dstY, s);
    if (!rc)
        rc = run_band(np->uv, nFrames, 0, static_cast<size_t>(np->uv->p.dstH), 0, srcStUV, srcFrameSt, srcUV, dstStUV,
                      dstFrameSt, dstUV, s);
    return rc;
}

// ---- NV12 / I420 straight to RGB bytes or normalised RGB tensors.  Two passes on the stream: the
// resize entries above, unchanged, into the caller's workspace, then yuv_rgb_kernel
// (kernels_color.hip) from the workspace to the destination.  Every check runs on the host before the
// first launch, so a rejected call launches nothing and leaves the destination untouched.
// In IQO_CHROMA_FULL the first pass is Y by its plan and chroma by the plan's full-grid chroma plan
// (srcW/2 x srcH/2 -> dstW x dstH), plane by plane, and the second pass is the kernel's 4:4:4 form.

// Workspace of one frame: the Y plane, then U and V (I420) or the interleaved UV plane (NV12, rows of
// 2 * cSt bytes) in the same bytes.  Rows are padded to what a thread of yuv_rgb_kernel loads (8 Y
// bytes, 4 chroma pairs) and to 16 bytes, so that every plane kernel finds its widest stores aligned
// and the fused I420 instantiations stay one launch.
// IQO_CHROMA_FULL: U and V (or the UV plane) hold dstH rows of dstW samples, padded as Y's rows, so a
// thread's 8 chroma pairs (16 bytes of UV, 8 each of U and V) are one aligned load.
struct YuvRgbWs {
    size_t ySt, cSt, cRows, frame;
};

static YuvRgbWs yuv_rgb_ws(size_t dstW, size_t dstH, int chroma)
{
    const size_t w8 = (dstW + 7) / 8 * 8;
    const bool full = chroma == IQO_CHROMA_FULL;
    YuvRgbWs w;
    w.ySt = (w8 + 15) & ~static_cast<size_t>(15);
    w.cSt = full ? w.ySt : (w8 / 2 + 15) & ~static_cast<size_t>(15);
    w.cRows = full ? dstH : dstH / 2;
    w.frame = w.ySt * dstH + 2 * w.cSt * w.cRows;
    return w;
}

size_t iqo_hip_yuv_rgb_workspace_bytes_chroma(size_t dstW, size_t dstH, size_t nFrames, int mode)
{
    const size_t kMaxSize = std::numeric_limits<size_t>::max(), kLim = size_t(1) << 31;
    if (dstW >= kLim || dstH >= kLim || (mode != IQO_CHROMA_REPLICATE && mode != IQO_CHROMA_FULL))
        return kMaxSize;  // (no plan has such a frame)
    const size_t frame = yuv_rgb_ws(dstW, dstH, mode).frame;
    if (frame && nFrames > (kMaxSize - 15) / frame)
        return kMaxSize;
    return nFrames * frame + 15;  // + 15: the calls round the base up to 16 bytes
}

size_t iqo_hip_yuv_rgb_workspace_bytes(size_t dstW, size_t dstH, size_t nFrames)
{
    return iqo_hip_yuv_rgb_workspace_bytes_chroma(dstW, dstH, nFrames, IQO_CHROMA_REPLICATE);
}

int iqo_host_yuv_to_rgb(int standard, size_t n, const uint8_t *y, const uint8_t *u, const uint8_t *v, uint8_t *rgb)
{
    if (standard < 0 || standard >= iqo_amd::kYuvRgbStandards || !y || !u || !v || !rgb)
        return IQO_HIP_EINVAL;
    const iqo_amd::YuvRgbCoef &k = iqo_amd::kYuvRgb[standard];
    for (size_t i = 0; i < n; ++i) {
        int R, G, B;
        iqo_amd::yuv_to_rgb(k, y[i], iqo_amd::yuv_chroma_terms(k, u[i], v[i]), R, G, B);
        rgb[3 * i] = static_cast<uint8_t>(R);
        rgb[3 * i + 1] = static_cast<uint8_t>(G);
        rgb[3 * i + 2] = static_cast<uint8_t>(B);
    }
    return IQO_HIP_OK;
}

// Where the second pass writes: packed bytes (norm == nullptr; rowSt = the row stride) or planar floats.
struct YuvRgbOut {
    int channels;
    const int *order;
    const iqo_hip_norm *norm;
    size_t rowSt, planeSt, frameSt;
    void *dst;
};

// One source plane as the first pass reads it: `bpp` bytes per pixel
static bool yuv_src_ok(const Plan &p, size_t bpp, size_t srcSt)
{
    const size_t rowB = static_cast<size_t>(p.srcW) * bpp;
    return srcSt >= rowB && srcSt < (size_t(1) << 24) && static_cast<size_t>(p.srcH - 1) * srcSt + rowB < (size_t(1) << 31);
}

// Everything the second pass needs checked (as run_norm for the float form); fills *nd for it.
static int yuv_rgb_check(const Plan &py, int chroma, size_t nFrames, int standard, const YuvRgbOut &o,
                         const void *workspace, size_t workspaceBytes, iqo_amd::NormDev *nd)
{
    if (!o.dst || !workspace || (!o.norm && !o.order))
        return IQO_HIP_EINVAL;
    if (standard < 0 || standard >= iqo_amd::kYuvRgbStandards)
        return IQO_HIP_EINVAL;
    const size_t dstW = static_cast<size_t>(py.dstW), dstH = static_cast<size_t>(py.dstH), kLim = size_t(1) << 31;
    size_t elem = 1, planes = 1, rowB;
    if (o.norm) {
        const iqo_hip_norm &n = *o.norm;
        if (n.dtype != IQO_OUT_F32 && n.dtype != IQO_OUT_F16 && n.dtype != IQO_OUT_BF16)
            return IQO_HIP_EINVAL;
        if (n.planes < 1 || n.planes > 4)
            return IQO_HIP_EINVAL;
        for (int i = 0; i < n.planes; ++i)
            if (n.order[i] < 0 || n.order[i] > 2 || !std::isfinite(n.scale[i]) || !std::isfinite(n.bias[i]))
                return IQO_HIP_EINVAL;
        elem = n.dtype == IQO_OUT_F32 ? 4 : 2;
        planes = static_cast<size_t>(n.planes);
        rowB = dstW * elem;
        if (reinterpret_cast<uintptr_t>(o.dst) % elem || o.rowSt % elem || o.planeSt % elem || o.frameSt % elem)
            return IQO_HIP_EINVAL;
        if (o.planeSt / dstH < o.rowSt || o.planeSt >= kLim)
            return IQO_HIP_EINVAL;
        nd->dtype = n.dtype;
        nd->planes = n.planes;
        nd->planeSt = static_cast<int>(o.planeSt);
        for (int i = 0; i < 4; ++i) {
            const bool used = i < n.planes;
            nd->order[i] = used ? n.order[i] : 0;
            nd->scale[i] = used ? n.scale[i] : 0.f;
            nd->bias[i] = used ? n.bias[i] : 0.f;
        }
    } else {
        if (o.channels < 3 || o.channels > 4)
            return IQO_HIP_EINVAL;
        for (int c = 0; c < o.channels; ++c)
            if (o.order[c] < 0 || o.order[c] > 3)
                return IQO_HIP_EINVAL;
        rowB = dstW * static_cast<size_t>(o.channels);
    }
    // (divisions: no product of caller-supplied strides can wrap)
    const size_t frameRows = o.norm ? o.planeSt : o.rowSt;  // a frame holds `planes` planes / dstH rows of these
    if (o.rowSt < rowB || o.rowSt >= kLim || (nFrames > 1 && o.frameSt / (o.norm ? planes : dstH) < frameRows))
        return IQO_HIP_EINVAL;
    // the kernel addresses one destination frame and one workspace frame with 32-bit offsets
    if ((planes - 1) * (o.norm ? o.planeSt : 0) + (dstH - 1) * o.rowSt + rowB >= kLim ||
        yuv_rgb_ws(dstW, dstH, chroma).frame >= kLim)
        return IQO_HIP_EINVAL;
    if (workspaceBytes < iqo_hip_yuv_rgb_workspace_bytes_chroma(dstW, dstH, nFrames, chroma))
        return IQO_HIP_EINVAL;
    return IQO_HIP_OK;
}

static uint8_t *yuv_rgb_ws_base(void *workspace)
{
    return reinterpret_cast<uint8_t *>((reinterpret_cast<uintptr_t>(workspace) + 15) & ~static_cast<uintptr_t>(15));
}

// The second pass: yuv_rgb_kernel over the workspace planes the first pass wrote.
static int yuv_rgb_convert(const iqo_hip_plan *hy, int chroma, size_t nFrames, const uint8_t *ws, bool interleavedUV,
                           int standard, const YuvRgbOut &o, const iqo_amd::NormDev &nd, hipStream_t s)
{
    const Plan &py = hy->p;
    const bool full = chroma == IQO_CHROMA_FULL;
    const YuvRgbWs w = yuv_rgb_ws(static_cast<size_t>(py.dstW), static_cast<size_t>(py.dstH), chroma);
    DeviceGuard guard(hy->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    iqo_amd::YuvRgbDev d{};
    d.dstW = py.dstW;
    d.dstH = py.dstH;
    d.cw = full ? py.dstW : py.dstW / 2;
    d.ch = full ? py.dstH : py.dstH / 2;
    d.k = iqo_amd::kYuvRgb[standard];
    d.ySt = static_cast<int>(w.ySt);
    d.cSt = static_cast<int>(interleavedUV ? 2 * w.cSt : w.cSt);
    d.frameSt = static_cast<int64_t>(w.frame);
    d.dstSt = static_cast<int>(o.rowSt);
    d.dstFrameSt = static_cast<int64_t>(o.frameSt);
    // frames per launch: the kernel counts (frame, row, pixel group) items in 31 bits, groups of 4 at the least
    const size_t perFrame = static_cast<size_t>(py.dstH) * ((static_cast<size_t>(py.dstW) + 3) / 4);
    const size_t chunk = std::max<size_t>(1, ((size_t(1) << 31) - 1) / perFrame);
    for (size_t f0 = 0; f0 < nFrames; f0 += chunk) {
        d.frames = static_cast<int>(std::min(chunk, nFrames - f0));
        d.y = ws + f0 * w.frame;
        d.u = d.y + w.ySt * static_cast<size_t>(py.dstH);
        d.v = d.u + w.cSt * w.cRows;
        d.dst = static_cast<uint8_t *>(o.dst) + f0 * o.frameSt;
        int order[4] = {0, 0, 0, 0};
        for (int c = 0; !o.norm && c < o.channels; ++c)
            order[c] = o.order[c];
        const hipError_t e = o.norm ? iqo_amd::launch_yuv_rgb_norm(d, interleavedUV, full, nd, s)
                                    : iqo_amd::launch_yuv_rgb_bytes(d, interleavedUV, full, o.channels, order, s);
        if (e == hipErrorInvalidValue)
            return IQO_HIP_EINVAL;
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return IQO_HIP_OK;
}

static int nv12_rgb(iqo_hip_nv12_plan *np, size_t nFrames, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                    const uint8_t *srcY, const uint8_t *srcUV, int standard, const YuvRgbOut &o, void *workspace,
                    size_t workspaceBytes, void *stream)
{
    if (!np || !np->y || !np->uv || !srcY || !srcUV)
        return IQO_HIP_EINVAL;
    const Plan &py = np->y->p;
    iqo_amd::NormDev nd{};
    const bool full = np->chroma == IQO_CHROMA_FULL;
    if (full && !np->uvf)
        return IQO_HIP_EINVAL;
    const int rc = yuv_rgb_check(py, np->chroma, nFrames, standard, o, workspace, workspaceBytes, &nd);
    if (rc)
        return rc;
    if (!yuv_src_ok(py, 1, srcStY) || !yuv_src_ok(np->uv->p, 2, srcStUV))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;
    const size_t dstH = static_cast<size_t>(py.dstH);
    const YuvRgbWs w = yuv_rgb_ws(static_cast<size_t>(py.dstW), dstH, np->chroma);
    uint8_t *ws = yuv_rgb_ws_base(workspace), *wuv = ws + w.ySt * dstH;
    int r1;
    if (full) {
        // Y by its plan, UV by the full-grid plan: the launches of iqo_hip_resize_nv12_device
        hipStream_t s = static_cast<hipStream_t>(stream);
        r1 = run_band(np->y, nFrames, 0, dstH, 0, srcStY, srcFrameSt, srcY, w.ySt, w.frame, ws, s);
        if (!r1)
            r1 = run_band(np->uvf, nFrames, 0, dstH, 0, srcStUV, srcFrameSt, srcUV, 2 * w.cSt, w.frame, wuv, s);
    } else {
        r1 = iqo_hip_resize_nv12_device(np, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcUV, w.ySt, 2 * w.cSt, w.frame, ws,
                                        wuv, stream);
    }
    if (r1)
        return r1;
    return yuv_rgb_convert(np->y, np->chroma, nFrames, ws, true, standard, o, nd, static_cast<hipStream_t>(stream));
}

static int yuv420_rgb(iqo_hip_yuv_plan *yp, size_t nFrames, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                      const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV, int standard, const YuvRgbOut &o,
                      void *workspace, size_t workspaceBytes, void *stream, int *fused)
{
    if (fused)
        *fused = 0;
    if (!yp || !yp->y || !yp->c || !srcY || !srcU || !srcV)
        return IQO_HIP_EINVAL;
    const Plan &py = yp->y->p;
    iqo_amd::NormDev nd{};
    const bool full = yp->chroma == IQO_CHROMA_FULL;
    if (full && !yp->cf)
        return IQO_HIP_EINVAL;
    const int rc = yuv_rgb_check(py, yp->chroma, nFrames, standard, o, workspace, workspaceBytes, &nd);
    if (rc)
        return rc;
    if (!yuv_src_ok(py, 1, srcStY) || !yuv_src_ok(yp->c->p, 1, srcStUV))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;
    const size_t dstH = static_cast<size_t>(py.dstH);
    const YuvRgbWs w = yuv_rgb_ws(static_cast<size_t>(py.dstW), dstH, yp->chroma);
    uint8_t *ws = yuv_rgb_ws_base(workspace), *wu = ws + w.ySt * dstH, *wv = wu + w.cSt * w.cRows;
    int r1;
    if (full) {
        // plane by plane: Y by its plan, U and then V by the full-grid plan (*fused stays 0)
        hipStream_t s = static_cast<hipStream_t>(stream);
        r1 = run_band(yp->y, nFrames, 0, dstH, 0, srcStY, srcFrameSt, srcY, w.ySt, w.frame, ws, s);
        if (!r1)
            r1 = run_band(yp->cf, nFrames, 0, dstH, 0, srcStUV, srcFrameSt, srcU, w.cSt, w.frame, wu, s);
        if (!r1)
            r1 = run_band(yp->cf, nFrames, 0, dstH, 0, srcStUV, srcFrameSt, srcV, w.cSt, w.frame, wv, s);
    } else {
        r1 = iqo_hip_resize_yuv420_device(yp, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcU, srcV, w.ySt, w.cSt, w.frame,
                                          ws, wu, wv, stream, fused);
    }
    if (r1)
        return r1;
    return yuv_rgb_convert(yp->y, yp->chroma, nFrames, ws, false, standard, o, nd, static_cast<hipStream_t>(stream));
}

int iqo_hip_resize_nv12_rgb_device(iqo_hip_nv12_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                   size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcUV, int standard,
                                   int channels, const int *order, size_t dstSt, size_t dstFrameSt, uint8_t *dst,
                                   void *workspace, size_t workspaceBytes, void *stream)
{
    const YuvRgbOut o{channels, order, nullptr, dstSt, 0, dstFrameSt, dst};
    return nv12_rgb(plan, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcUV, standard, o, workspace, workspaceBytes, stream);
}

int iqo_hip_resize_nv12_norm_device(iqo_hip_nv12_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                    size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcUV, int standard,
                                    const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt, size_t dstFrameSt,
                                    void *dDst, void *workspace, size_t workspaceBytes, void *stream)
{
    if (!norm)
        return IQO_HIP_EINVAL;
    const YuvRgbOut o{3, nullptr, norm, dstRowSt, dstPlaneSt, dstFrameSt, dDst};
    return nv12_rgb(plan, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcUV, standard, o, workspace, workspaceBytes, stream);
}

int iqo_hip_resize_yuv420_rgb_device(iqo_hip_yuv_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                     size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                     int standard, int channels, const int *order, size_t dstSt, size_t dstFrameSt,
                                     uint8_t *dst, void *workspace, size_t workspaceBytes, void *stream, int *fused)
{
    const YuvRgbOut o{channels, order, nullptr, dstSt, 0, dstFrameSt, dst};
    return yuv420_rgb(plan, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcU, srcV, standard, o, workspace, workspaceBytes,
                      stream, fused);
}

int iqo_hip_resize_yuv420_norm_device(iqo_hip_yuv_plan *plan, size_t nFrames, size_t srcStY, size_t srcStUV,
                                      size_t srcFrameSt, const uint8_t *srcY, const uint8_t *srcU, const uint8_t *srcV,
                                      int standard, const iqo_hip_norm *norm, size_t dstRowSt, size_t dstPlaneSt,
                                      size_t dstFrameSt, void *dDst, void *workspace, size_t workspaceBytes, void *stream,
                                      int *fused)
{
    if (fused)
        *fused = 0;
    if (!norm)
        return IQO_HIP_EINVAL;
    const YuvRgbOut o{3, nullptr, norm, dstRowSt, dstPlaneSt, dstFrameSt, dDst};
    return yuv420_rgb(plan, nFrames, srcStY, srcStUV, srcFrameSt, srcY, srcU, srcV, standard, o, workspace, workspaceBytes,
                      stream, fused);
}

// ---- Planar U8 frames ([F, P, H, W] tensors, grey images, a video frame's Y plane) straight to normalised
// planar floats.  Two passes on the stream: the 1-channel plan's own resize, unchanged (run_band over the
// full frame, so whatever kernel family the layout gets), into the caller's workspace, then
// planes_norm_kernel (kernels_norm.hip) from the workspace to the destination.  Every check runs on the
// host before the first launch, so a rejected call launches nothing and leaves the destination untouched.

// Workspace of one frame: srcPlanes planes of dstH rows, each row padded to the 8 pixels a thread of
// planes_norm_kernel loads and to 16 bytes, so that every plan kernel finds its widest stores aligned.
struct PlanesNormWs {
    size_t st, plane, frame;
};

static PlanesNormWs planes_norm_ws(size_t dstW, size_t dstH, size_t srcPlanes)
{
    PlanesNormWs w;
    w.st = ((dstW + 7) / 8 * 8 + 15) & ~static_cast<size_t>(15);
    w.plane = w.st * dstH;
    w.frame = w.plane * srcPlanes;
    return w;
}

size_t iqo_hip_planes_norm_workspace_bytes(size_t dstW, size_t dstH, int srcPlanes, size_t nFrames)
{
    const size_t kMaxSize = std::numeric_limits<size_t>::max(), kLim = size_t(1) << 31;
    if (dstW >= kLim || dstH >= kLim || srcPlanes < 1 || srcPlanes > 4)
        return kMaxSize;  // (no plan has such a frame)
    // (a plane is below 2^63: four of them can pass 2^64)
    if (planes_norm_ws(dstW, dstH, 1).plane > (kMaxSize - 15) / static_cast<size_t>(srcPlanes))
        return kMaxSize;
    const size_t frame = planes_norm_ws(dstW, dstH, static_cast<size_t>(srcPlanes)).frame;
    if (frame && nFrames > (kMaxSize - 15) / frame)
        return kMaxSize;
    return nFrames * frame + 15;  // + 15: the call rounds the base up to 16 bytes
}

int iqo_hip_resize_planes_norm_device(iqo_hip_plan *h, size_t nFrames, int srcPlanes, size_t srcSt, size_t srcPlaneSt,
                                      size_t srcFrameSt, const uint8_t *dSrc, const iqo_hip_norm *norm, size_t dstRowSt,
                                      size_t dstPlaneSt, size_t dstFrameSt, void *dDst, void *workspace,
                                      size_t workspaceBytes, void *stream)
{
    if (!h || !dSrc || !dDst || !norm || !workspace)
        return IQO_HIP_EINVAL;
    if (h->channels != 1)  // packed plans: iqo_hip_resize_device_norm
        return IQO_HIP_EUNSUP;
    if (srcPlanes < 1 || srcPlanes > 4)
        return IQO_HIP_EINVAL;
    // the norm and its destination, as run_norm
    if (norm->dtype != IQO_OUT_F32 && norm->dtype != IQO_OUT_F16 && norm->dtype != IQO_OUT_BF16)
        return IQO_HIP_EINVAL;
    if (norm->planes < 1 || norm->planes > 4)
        return IQO_HIP_EINVAL;
    unsigned used = 0;  // bit c: source plane c is referenced
    for (int i = 0; i < norm->planes; ++i) {
        if (norm->order[i] < 0 || norm->order[i] >= srcPlanes || !std::isfinite(norm->scale[i]) ||
            !std::isfinite(norm->bias[i]))
            return IQO_HIP_EINVAL;
        used |= 1u << norm->order[i];
    }
    const Plan &p = h->p;
    const size_t elem = norm->dtype == IQO_OUT_F32 ? 4 : 2;
    const size_t dstW = static_cast<size_t>(p.dstW), dstH = static_cast<size_t>(p.dstH);
    const size_t planes = static_cast<size_t>(norm->planes), P = static_cast<size_t>(srcPlanes);
    if (reinterpret_cast<uintptr_t>(dDst) % elem || dstRowSt % elem || dstPlaneSt % elem || dstFrameSt % elem)
        return IQO_HIP_EINVAL;
    // (divisions: no product of caller-supplied strides can wrap)
    if (dstRowSt < dstW * elem || dstPlaneSt / dstH < dstRowSt || (nFrames > 1 && dstFrameSt / planes < dstPlaneSt))
        return IQO_HIP_EINVAL;
    // the kernel addresses one float frame with 32-bit byte offsets
    const size_t kLim = size_t(1) << 31;
    if (dstRowSt >= kLim || dstPlaneSt >= kLim || (planes - 1) * dstPlaneSt + (dstH - 1) * dstRowSt + dstW * elem >= kLim)
        return IQO_HIP_EINVAL;
    if (!yuv_src_ok(p, 1, srcSt))
        return IQO_HIP_EINVAL;
    if (workspaceBytes < iqo_hip_planes_norm_workspace_bytes(dstW, dstH, srcPlanes, nFrames))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;

    hipStream_t s = static_cast<hipStream_t>(stream);
    const PlanesNormWs w = planes_norm_ws(dstW, dstH, P);
    uint8_t *ws = yuv_rgb_ws_base(workspace);
    // First pass.  The contiguous [F, P, H, W] tensor with every plane referenced is one batch of
    // nFrames * srcPlanes frames a plane stride apart, the workspace's planes likewise; otherwise one
    // batch per referenced plane (an unused plane is not resized).
    if (P == 1) {
        const int rc = run_band(h, nFrames, 0, dstH, 0, srcSt, srcFrameSt, dSrc, w.st, w.frame, ws, s);
        if (rc)
            return rc;
    } else if (used == (1u << srcPlanes) - 1u && srcFrameSt / P == srcPlaneSt && srcFrameSt % P == 0) {
        const int rc = run_band(h, nFrames * P, 0, dstH, 0, srcSt, srcPlaneSt, dSrc, w.st, w.plane, ws, s);
        if (rc)
            return rc;
    } else {
        for (size_t c = 0; c < P; ++c) {
            if (!(used >> c & 1u))
                continue;
            const int rc = run_band(h, nFrames, 0, dstH, 0, srcSt, srcFrameSt, dSrc + c * srcPlaneSt, w.st, w.frame,
                                    ws + c * w.plane, s);
            if (rc)
                return rc;
        }
    }

    // Second pass: planes_norm_kernel over the workspace planes.
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    iqo_amd::NormDev nd{};
    nd.dtype = norm->dtype;
    nd.planes = norm->planes;
    nd.planeSt = static_cast<int>(dstPlaneSt);
    for (int i = 0; i < norm->planes; ++i) {
        nd.order[i] = norm->order[i];
        nd.scale[i] = norm->scale[i];
        nd.bias[i] = norm->bias[i];
    }
    iqo_amd::PlanesNormDev d{};
    d.dstW = p.dstW;
    d.dstH = p.dstH;
    d.srcSt = static_cast<int>(w.st);
    d.srcPlaneSt = static_cast<int64_t>(w.plane);
    d.srcFrameSt = static_cast<int64_t>(w.frame);
    d.dstSt = static_cast<int>(dstRowSt);
    d.dstFrameSt = static_cast<int64_t>(dstFrameSt);
    // frames per launch: the kernel counts (frame, row, pixel group) items in 31 bits, groups of 4 at the least
    const size_t perFrame = dstH * ((dstW + 3) / 4);
    const size_t chunk = std::max<size_t>(1, ((size_t(1) << 31) - 1) / perFrame);
    for (size_t f0 = 0; f0 < nFrames; f0 += chunk) {
        d.frames = static_cast<int>(std::min(chunk, nFrames - f0));
        d.src = ws + f0 * w.frame;
        d.dst = static_cast<uint8_t *>(dDst) + f0 * dstFrameSt;
        const hipError_t e = iqo_amd::launch_planes_norm(d, nd, s);
        if (e == hipErrorInvalidValue)
            return IQO_HIP_EINVAL;
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return IQO_HIP_OK;
}

// ---- Packed RGB(A) straight to NV12 / I420, the opposite direction.  Two passes on the stream: the
// packed plan's own resize, unchanged, into the caller's workspace, then rgb_yuv_kernel
// (kernels_color.hip) from the workspace to the planes.  Every check runs on the host before the first
// launch, so a rejected call launches nothing and leaves the destination untouched.

// Workspace of one frame: dstH rows of packed pixels, padded to the 8 pixels a thread of rgb_yuv_kernel
// loads and to 16 bytes, so that the first pass finds its widest stores aligned.
static size_t rgb_yuv_ws_stride(size_t dstW, size_t C)
{
    return ((dstW + 7) / 8 * 8 * C + 15) & ~static_cast<size_t>(15);
}

size_t iqo_hip_rgb_yuv_workspace_bytes(size_t dstW, size_t dstH, int channels, size_t nFrames)
{
    const size_t kMaxSize = std::numeric_limits<size_t>::max(), kLim = size_t(1) << 31;
    if (dstW >= kLim || dstH >= kLim || channels < 3 || channels > 4)
        return kMaxSize;  // (no plan has such a frame)
    const size_t frame = rgb_yuv_ws_stride(dstW, static_cast<size_t>(channels)) * dstH;
    if (frame && nFrames > (kMaxSize - 15) / frame)
        return kMaxSize;
    return nFrames * frame + 15;  // + 15: the calls round the base up to 16 bytes
}

int iqo_host_rgb_to_yuv(int standard, size_t n, const uint8_t *rgb, uint8_t *y, uint8_t *u, uint8_t *v)
{
    if (standard < 0 || standard >= iqo_amd::kYuvRgbStandards || !rgb || !y || !u || !v)
        return IQO_HIP_EINVAL;
    const iqo_amd::RgbYuvCoef &k = iqo_amd::kRgbYuv[standard];
    constexpr int S = iqo_amd::kRgbYuvShift;
    for (size_t i = 0; i < n; ++i) {
        const int R = rgb[3 * i], G = rgb[3 * i + 1], B = rgb[3 * i + 2];
        y[i] = static_cast<uint8_t>(iqo_amd::rgb_y_sum(k, R, G, B) >> S);
        u[i] = static_cast<uint8_t>(iqo_amd::rgb_yuv_min255(iqo_amd::rgb_u_sum<S>(k, R, G, B) >> S));
        v[i] = static_cast<uint8_t>(iqo_amd::rgb_yuv_min255(iqo_amd::rgb_v_sum<S>(k, R, G, B) >> S));
    }
    return IQO_HIP_OK;
}

int iqo_host_rgb_to_yuv420(int standard, size_t w, size_t h, const uint8_t *rgb, uint8_t *y, uint8_t *u, uint8_t *v)
{
    if (standard < 0 || standard >= iqo_amd::kYuvRgbStandards || !rgb || !y || !u || !v || w < 2 || h < 2)
        return IQO_HIP_EINVAL;
    const iqo_amd::RgbYuvCoef &k = iqo_amd::kRgbYuv[standard];
    for (size_t i = 0; i < w * h; ++i)
        y[i] = static_cast<uint8_t>(iqo_amd::rgb_y_sum(k, rgb[3 * i], rgb[3 * i + 1], rgb[3 * i + 2]) >> iqo_amd::kRgbYuvShift);
    constexpr int S = iqo_amd::kRgbYuvSumShift;
    const size_t cw = w / 2, ch = h / 2;
    for (size_t j = 0; j < ch; ++j)
        for (size_t i = 0; i < cw; ++i) {
            int s[3] = {0, 0, 0};
            for (size_t e = 0; e < 4; ++e) {
                const uint8_t *p = rgb + 3 * ((2 * j + e / 2) * w + 2 * i + e % 2);
                for (int c = 0; c < 3; ++c)
                    s[c] += p[c];
            }
            u[j * cw + i] = static_cast<uint8_t>(iqo_amd::rgb_yuv_min255(iqo_amd::rgb_u_sum<S>(k, s[0], s[1], s[2]) >> S));
            v[j * cw + i] = static_cast<uint8_t>(iqo_amd::rgb_yuv_min255(iqo_amd::rgb_v_sum<S>(k, s[0], s[1], s[2]) >> S));
        }
    return IQO_HIP_OK;
}

// A destination plane of one frame: rows of rowB bytes, `rows` of them, `st` apart
struct RgbYuvPlane {
    const uint8_t *p;
    size_t rowB, rows, st;
    uintptr_t begin() const { return reinterpret_cast<uintptr_t>(p); }
    size_t extent() const { return (rows - 1) * st + rowB; }  // first byte to one past the last
};

static int rgb_yuv(iqo_hip_plan *h, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *src, int standard,
                   const int *order, size_t dstStY, size_t dstStUV, size_t dstFrameSt, uint8_t *dstY, uint8_t *dstU,
                   uint8_t *dstV, bool interleavedUV, void *workspace, size_t workspaceBytes, void *stream)
{
    if (!h || !src || !dstY || !dstU || (!interleavedUV && !dstV) || !workspace || !order)
        return IQO_HIP_EINVAL;
    if (h->channels < 3 || h->channels > 4)
        return IQO_HIP_EUNSUP;  // a planar plan, or 2 channels: no R, G, B to take
    if (standard < 0 || standard >= iqo_amd::kYuvRgbStandards)
        return IQO_HIP_EINVAL;
    const size_t C = static_cast<size_t>(h->channels);
    for (int c = 0; c < 3; ++c)
        if (order[c] < 0 || order[c] >= h->channels || order[c] == order[(c + 1) % 3])
            return IQO_HIP_EINVAL;
    const Plan &p = h->p;
    const size_t dstW = static_cast<size_t>(p.dstW), dstH = static_cast<size_t>(p.dstH), kLim = size_t(1) << 31;
    if (dstW < 2 || dstH < 2)
        return IQO_HIP_EINVAL;
    const size_t cw = dstW / 2, ch = dstH / 2;
    // the planes of one frame, lowest address first; none may reach into the next
    RgbYuvPlane pl[3] = {{dstY, dstW, dstH, dstStY}, {dstU, interleavedUV ? 2 * cw : cw, ch, dstStUV}, {dstV, cw, ch, dstStUV}};
    const int nPl = interleavedUV ? 2 : 3;
    for (int i = 0; i < nPl; ++i)
        if (pl[i].st < pl[i].rowB || pl[i].st >= kLim || pl[i].extent() >= kLim)
            return IQO_HIP_EINVAL;
    std::sort(pl, pl + nPl, [](const RgbYuvPlane &a, const RgbYuvPlane &b) { return a.begin() < b.begin(); });
    for (int i = 0; i + 1 < nPl; ++i)
        if (pl[i + 1].begin() - pl[i].begin() < pl[i].extent())
            return IQO_HIP_EINVAL;
    // frames follow each other dstFrameSt apart: the highest plane must end before the lowest begins again
    if (nFrames > 1 && dstFrameSt < pl[nPl - 1].begin() - pl[0].begin() + pl[nPl - 1].extent())
        return IQO_HIP_EINVAL;
    if (!yuv_src_ok(p, C, srcSt))
        return IQO_HIP_EINVAL;
    // the kernel addresses one workspace frame with 32-bit offsets
    const size_t wsSt = rgb_yuv_ws_stride(dstW, C), wsFrame = wsSt * dstH;
    if (wsFrame >= kLim || workspaceBytes < iqo_hip_rgb_yuv_workspace_bytes(dstW, dstH, h->channels, nFrames))
        return IQO_HIP_EINVAL;
    if (nFrames == 0)
        return IQO_HIP_OK;
    hipStream_t s = static_cast<hipStream_t>(stream);
    uint8_t *ws = yuv_rgb_ws_base(workspace);
    const int r1 = run_band(h, nFrames, 0, dstH, 0, srcSt, srcFrameSt, src, wsSt, wsFrame, ws, s);
    if (r1)
        return r1;
    DeviceGuard guard(h->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    iqo_amd::RgbYuvDev d{};
    d.dstW = p.dstW;
    d.dstH = p.dstH;
    d.k = iqo_amd::kRgbYuv[standard];
    for (int c = 0; c < 3; ++c)
        d.order[c] = order[c];
    d.srcSt = static_cast<int>(wsSt);
    d.srcFrameSt = static_cast<int64_t>(wsFrame);
    d.ySt = static_cast<int>(dstStY);
    d.cSt = static_cast<int>(dstStUV);
    d.dstFrameSt = static_cast<int64_t>(dstFrameSt);
    // frames per launch: the kernel counts (frame, row pair, pixel group) items in 31 bits
    const size_t perFrame = ((dstH + 1) / 2) * ((dstW + 7) / 8);
    const size_t chunk = std::max<size_t>(1, ((size_t(1) << 31) - 1) / perFrame);
    for (size_t f0 = 0; f0 < nFrames; f0 += chunk) {
        d.frames = static_cast<int>(std::min(chunk, nFrames - f0));
        d.src = ws + f0 * wsFrame;
        d.y = dstY + f0 * dstFrameSt;
        d.u = dstU + f0 * dstFrameSt;
        d.v = interleavedUV ? nullptr : dstV + f0 * dstFrameSt;
        const hipError_t e = iqo_amd::launch_rgb_yuv(d, h->channels, interleavedUV, s);
        if (e == hipErrorInvalidValue)
            return IQO_HIP_EINVAL;
        if (e != hipSuccess)
            return IQO_HIP_EHIP;
    }
    return IQO_HIP_OK;
}

int iqo_hip_resize_rgb_nv12_device(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *src,
                                   int standard, const int *order, size_t dstStY, size_t dstStUV, size_t dstFrameSt,
                                   uint8_t *dstY, uint8_t *dstUV, void *workspace, size_t workspaceBytes, void *stream)
{
    return rgb_yuv(plan, nFrames, srcSt, srcFrameSt, src, standard, order, dstStY, dstStUV, dstFrameSt, dstY, dstUV, nullptr,
                   true, workspace, workspaceBytes, stream);
}

int iqo_hip_resize_rgb_yuv420_device(iqo_hip_plan *plan, size_t nFrames, size_t srcSt, size_t srcFrameSt, const uint8_t *src,
                                     int standard, const int *order, size_t dstStY, size_t dstStUV, size_t dstFrameSt,
                                     uint8_t *dstY, uint8_t *dstU, uint8_t *dstV, void *workspace, size_t workspaceBytes,
                                     void *stream)
{
    return rgb_yuv(plan, nFrames, srcSt, srcFrameSt, src, standard, order, dstStY, dstStUV, dstFrameSt, dstY, dstU, dstV,
                   false, workspace, workspaceBytes, stream);
}

int iqo_hip_resize_yuv420(iqo_hip_yuv_plan *yp, size_t srcStY, const uint8_t *srcY, size_t srcStUV,
                          const uint8_t *srcU, const uint8_t *srcV, size_t dstStY, uint8_t *dstY, size_t dstStUV,
                          uint8_t *dstU, uint8_t *dstV)
{
    if (!yp || !yp->y || !yp->c || !srcY || !srcU || !srcV || !dstY || !dstU || !dstV)
        return IQO_HIP_EINVAL;
    {
        // small frames: the three planes staged into one buffer, one upload, the fused device
        // launch (iqo_hip_resize_yuv420_device), one download, one synchronisation
        const Plan &py = yp->y->p, &pc = yp->c->p;
        const size_t W = static_cast<size_t>(py.srcW), H = static_cast<size_t>(py.srcH);
        const size_t Wc = static_cast<size_t>(pc.srcW), Hc = static_cast<size_t>(pc.srcH);
        const size_t w = static_cast<size_t>(py.dstW), hh = static_cast<size_t>(py.dstH);
        const size_t wc = static_cast<size_t>(pc.dstW), hc = static_cast<size_t>(pc.dstH);
        if (srcStY < W || srcStUV < Wc || dstStY < w || dstStUV < wc)
            return IQO_HIP_EINVAL;
        const size_t sY = (W + 15) & ~size_t(15), sC = (Wc + 15) & ~size_t(15);
        const size_t dY = (w + 15) & ~size_t(15), dC = (wc + 15) & ~size_t(15);
        const size_t oU = sY * H, oV = oU + sC * Hc, sBytes = oV + sC * Hc;
        const size_t ou = dY * hh, ov = ou + dC * hc, dBytes = ov + dC * hc;
        if (sBytes < kHostPipeMinBytes) {
            DeviceGuard guard(yp->y->device);
            if (!guard.ok())
                return IQO_HIP_ENODEV;
            HostStage *st = acquire_stage(yp->y->device);
            if (!st)
                return IQO_HIP_EHIP;
            int rc = IQO_HIP_OK;
            if (grow_device(&st->dSrc, &st->dSrcCap, sBytes) || grow_device(&st->dDst, &st->dDstCap, dBytes) ||
                grow_pinned(&st->hSrc, &st->hSrcCap, sBytes) || grow_pinned(&st->hDst, &st->hDstCap, dBytes))
                rc = IQO_HIP_ENOMEM;
            if (!rc) {
                const RowCopy in[3] = {{st->hSrc, sY, srcY, srcStY, W, H}, {st->hSrc + oU, sC, srcU, srcStUV, Wc, Hc},
                                       {st->hSrc + oV, sC, srcV, srcStUV, Wc, Hc}};
                copy_planes_par(in, 3);
                if (hipMemcpyAsync(st->dSrc, st->hSrc, sBytes, hipMemcpyHostToDevice, st->sK) != hipSuccess)
                    rc = IQO_HIP_EHIP;
            }
            if (!rc)
                rc = iqo_hip_resize_yuv420_device(yp, 1, sY, sC, sBytes, st->dSrc, st->dSrc + oU, st->dSrc + oV, dY, dC,
                                                  dBytes, st->dDst, st->dDst + ou, st->dDst + ov, st->sK, nullptr);
            if (!rc && (hipMemcpyAsync(st->hDst, st->dDst, dBytes, hipMemcpyDeviceToHost, st->sK) != hipSuccess ||
                        hipStreamSynchronize(st->sK) != hipSuccess))
                rc = IQO_HIP_EHIP;
            if (!rc) {
                const RowCopy out[3] = {{dstY, dstStY, st->hDst, dY, w, hh}, {dstU, dstStUV, st->hDst + ou, dC, wc, hc},
                                        {dstV, dstStUV, st->hDst + ov, dC, wc, hc}};
                copy_planes_par(out, 3);
            } else {
                (void)hipStreamSynchronize(st->sK);
            }
            release_stage(st);
            return rc;
        }
    }
    // large frames: the three planes through ONE host pipeline (their uploads, kernels and
    // downloads overlap each other; one synchronisation per output chunk at the end)
    const Plan &py = yp->y->p, &pc = yp->c->p;
    const size_t sY = (static_cast<size_t>(py.srcW) + 15) & ~size_t(15), sC = (static_cast<size_t>(pc.srcW) + 15) & ~size_t(15);
    const size_t dY = (static_cast<size_t>(py.dstW) + 15) & ~size_t(15), dC = (static_cast<size_t>(pc.dstW) + 15) & ~size_t(15);
    const size_t oU = sY * static_cast<size_t>(py.srcH), oV = oU + sC * static_cast<size_t>(pc.srcH);
    const size_t sBytes = oV + sC * static_cast<size_t>(pc.srcH);
    const size_t ou = dY * static_cast<size_t>(py.dstH), ov = ou + dC * static_cast<size_t>(pc.dstH);
    const size_t dBytes = ov + dC * static_cast<size_t>(pc.dstH);
    DeviceGuard guard(yp->y->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    HostStage *st = acquire_stage(yp->y->device);
    if (!st)
        return IQO_HIP_EHIP;
    int rc = IQO_HIP_OK;
    if (grow_device(&st->dSrc, &st->dSrcCap, sBytes) || grow_device(&st->dDst, &st->dDstCap, dBytes))
        rc = IQO_HIP_ENOMEM;
    const bool pinY = is_pinned_host(srcY), pinU = is_pinned_host(srcU), pinV = is_pinned_host(srcV);
    const bool pinYd = is_pinned_host(dstY), pinUd = is_pinned_host(dstU), pinVd = is_pinned_host(dstV);
    // (pinned staging only for the banded pipeline, host_stage = 1: host_direct copies straight
    // from the caller's buffers)
    const bool staged = yp->y->hostStage != 0;
    if (!rc && staged && !(pinY && pinU && pinV) && grow_pinned(&st->hSrc, &st->hSrcCap, sBytes))
        rc = IQO_HIP_ENOMEM;
    if (!rc && staged && !(pinYd && pinUd && pinVd) && grow_pinned(&st->hDst, &st->hDstCap, dBytes))
        rc = IQO_HIP_ENOMEM;
    if (!rc) {
        HostPlane pl[3] = {{yp->y, srcStY, srcY, dstStY, dstY, 0, 0, sY, dY, pinY, pinYd},
                           {yp->c, srcStUV, srcU, dstStUV, dstU, oU, ou, sC, dC, pinU, pinUd},
                           {yp->c, srcStUV, srcV, dstStUV, dstV, oV, ov, sC, dC, pinV, pinVd}};
        rc = yp->y->hostStage ? host_pipeline(st, pl, 3) : host_direct(st, pl, 3);
    }
    if (rc) {
        (void)hipStreamSynchronize(st->sIn);
        (void)hipStreamSynchronize(st->sIn2);
        (void)hipStreamSynchronize(st->sK);
        (void)hipStreamSynchronize(st->sOut);
    }
    release_stage(st);
    return rc;
}

// ---- multi-GPU data movement (row-band windows out, bands back; no collective)

namespace {

// Peer access dst -> src enabled once per process and pair (hipDeviceEnablePeerAccess is
// per-context state; a second call reports hipErrorPeerAccessAlreadyEnabled).
bool enable_peer(int dst, int src)
{
    static std::mutex mu;
    static std::vector<std::pair<int, int>> done;
    std::lock_guard<std::mutex> g(mu);
    for (const auto &d : done)
        if (d.first == dst && d.second == src)
            return true;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, dst, src) != hipSuccess || !can)
        return false;
    DeviceGuard guard(dst);
    const hipError_t e = hipDeviceEnablePeerAccess(src, 0);
    if (e != hipSuccess && e != hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        return false;
    }
    (void)hipGetLastError();
    done.emplace_back(dst, src);
    return true;
}

// nFrames blocks of `bytes` at frame strides, one 2-D copy (the frame stride is the pitch).
hipError_t copy_blocks(void *dst, size_t dfs, const void *src, size_t sfs, size_t bytes, size_t n, hipMemcpyKind k,
                       hipStream_t s)
{
    if (n == 1 || (dfs == bytes && sfs == bytes))
        return hipMemcpyAsync(dst, src, bytes * n, k, s);
    return hipMemcpy2DAsync(dst, dfs, src, sfs, bytes, n, k, s);
}

} // namespace

int iqo_hip_copy_frames(void *dst, int dstDevice, size_t dstFrameSt, const void *src, int srcDevice, size_t srcFrameSt,
                        size_t bytesPerFrame, size_t nFrames, void *stream, int *path)
{
    if (path)
        *path = -1;
    if (!dst || !src || (dstDevice < 0 && srcDevice < 0))
        return IQO_HIP_EINVAL;
    if (bytesPerFrame == 0 || nFrames == 0)
        return IQO_HIP_OK;
    if (nFrames > 1 && (dstFrameSt < bytesPerFrame || srcFrameSt < bytesPerFrame))
        return IQO_HIP_EINVAL;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || dstDevice >= count || srcDevice >= count)
        return IQO_HIP_ENODEV;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const auto u8 = [](const void *p) { return static_cast<const uint8_t *>(p); };
    if (dstDevice < 0 || srcDevice < 0) {  // host <-> device
        DeviceGuard guard(dstDevice >= 0 ? dstDevice : srcDevice);
        if (!guard.ok())
            return IQO_HIP_ENODEV;
        const hipMemcpyKind k = srcDevice < 0 ? hipMemcpyHostToDevice : hipMemcpyDeviceToHost;
        if (copy_blocks(dst, dstFrameSt, src, srcFrameSt, bytesPerFrame, nFrames, k, s) != hipSuccess)
            return IQO_HIP_EHIP;
        if (path)
            *path = 3;
        return IQO_HIP_OK;
    }
    DeviceGuard guard(dstDevice);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    if (dstDevice == srcDevice) {
        if (copy_blocks(dst, dstFrameSt, src, srcFrameSt, bytesPerFrame, nFrames, hipMemcpyDeviceToDevice, s) != hipSuccess)
            return IQO_HIP_EHIP;
        if (path)
            *path = 0;
        return IQO_HIP_OK;
    }
    if (enable_peer(dstDevice, srcDevice)) {
        // peer DMA over xGMI, one copy per frame block (contiguous blocks: one copy in all)
        const bool contig = nFrames == 1 || (dstFrameSt == bytesPerFrame && srcFrameSt == bytesPerFrame);
        const size_t n = contig ? 1 : nFrames, b = contig ? bytesPerFrame * nFrames : bytesPerFrame;
        for (size_t f = 0; f < n; ++f)
            if (hipMemcpyPeerAsync(static_cast<uint8_t *>(dst) + f * dstFrameSt, dstDevice, u8(src) + f * srcFrameSt,
                                   srcDevice, b, s) != hipSuccess)
                return IQO_HIP_EHIP;
        if (path)
            *path = 1;
        return IQO_HIP_OK;
    }
    // no peer path: stage through pinned host memory, block by block, synchronously.  The blocking
    // hipMemcpy calls run on the devices' null streams, which a caller's non-blocking stream does
    // not order against: first drain `stream` (work still writing src or reading dst) and the
    // source device, so this route is ordered like the stream-ordered ones; when it returns the
    // copy has landed (iqo_hip.h).
    if (s && hipStreamSynchronize(s) != hipSuccess)
        return IQO_HIP_EHIP;
    {
        DeviceGuard sg(srcDevice);
        if (!sg.ok() || hipDeviceSynchronize() != hipSuccess)
            return IQO_HIP_EHIP;
    }
    uint8_t *h = nullptr;
    if (hipHostMalloc(reinterpret_cast<void **>(&h), bytesPerFrame, hipHostMallocDefault) != hipSuccess)
        return IQO_HIP_ENOMEM;
    int rc = IQO_HIP_OK;
    for (size_t f = 0; f < nFrames && rc == IQO_HIP_OK; ++f) {
        {
            DeviceGuard sg(srcDevice);
            if (!sg.ok() || hipMemcpy(h, u8(src) + f * srcFrameSt, bytesPerFrame, hipMemcpyDeviceToHost) != hipSuccess)
                rc = IQO_HIP_EHIP;
        }
        if (rc == IQO_HIP_OK &&
            hipMemcpy(static_cast<uint8_t *>(dst) + f * dstFrameSt, h, bytesPerFrame, hipMemcpyHostToDevice) != hipSuccess)
            rc = IQO_HIP_EHIP;
    }
    (void)hipHostFree(h);
    if (path && rc == IQO_HIP_OK)
        *path = 2;
    return rc;
}

int iqo_hip_ipc_export(const void *devPtr, iqo_hip_ipc_handle *handle)
{
    static_assert(sizeof(hipIpcMemHandle_t) <= sizeof(handle->bytes), "IPC handle size");
    if (!devPtr || !handle)
        return IQO_HIP_EINVAL;
    hipDeviceptr_t base = nullptr;
    size_t size = 0;
    if (hipMemGetAddressRange(&base, &size, const_cast<void *>(devPtr)) != hipSuccess || !base)
        return IQO_HIP_EHIP;
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, base) != hipSuccess)
        return IQO_HIP_EHIP;
    std::memset(handle, 0, sizeof(*handle));
    std::memcpy(handle->bytes, &h, sizeof(h));
    handle->offset = static_cast<uint64_t>(static_cast<const uint8_t *>(devPtr) - static_cast<const uint8_t *>(base));
    return IQO_HIP_OK;
}

int iqo_hip_ipc_open(const iqo_hip_ipc_handle *handle, int device, void **devPtr)
{
    if (!handle || !devPtr)
        return IQO_HIP_EINVAL;
    *devPtr = nullptr;
    DeviceGuard guard(device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle->bytes, sizeof(h));
    void *base = nullptr;
    if (hipIpcOpenMemHandle(&base, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess || !base)
        return IQO_HIP_EHIP;
    *devPtr = static_cast<uint8_t *>(base) + handle->offset;
    return IQO_HIP_OK;
}

int iqo_hip_ipc_close(void *devPtr, const iqo_hip_ipc_handle *handle)
{
    if (!devPtr || !handle)
        return IQO_HIP_EINVAL;
    return hipIpcCloseMemHandle(static_cast<uint8_t *>(devPtr) - handle->offset) == hipSuccess ? IQO_HIP_OK
                                                                                                : IQO_HIP_EHIP;
}

const char *iqo_hip_strerror(int status)
{
    switch (status) {
    case IQO_HIP_OK:
        return "ok";
    case IQO_HIP_EINVAL:
        return "invalid argument";
    case IQO_HIP_ENODEV:
        return "no usable gfx950 device";
    case IQO_HIP_ENOMEM:
        return "out of memory";
    case IQO_HIP_EHIP:
        return "HIP runtime or kernel launch failure";
    case IQO_HIP_EUNSUP:
        return "unsupported shape or layout";
    default:
        return "unknown status";
    }
}

const char *iqo_hip_version(void) { return "libiqo_amd 0.1 (gfx950)"; }

int iqo_host_tables(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale,
                    int axis, int *nTaps, int *nPhases, int32_t *buf, size_t cap)
{
    if (method < 0 || method > 2)
        return IQO_HIP_EINVAL;
    AxisPlan x, y;
    std::string err;
    if (!iqo_amd::build_tables(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &x, &y, &err))
        return IQO_HIP_EINVAL;
    const AxisPlan &a = axis ? y : x;
    if (nTaps)
        *nTaps = a.taps;
    if (nPhases)
        *nPhases = a.phases;
    if (buf && cap >= a.table.size())
        std::memcpy(buf, a.table.data(), a.table.size() * sizeof(int32_t));
    return static_cast<int>(a.table.size());
}

int iqo_host_band_src_rows(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                           size_t pxScale, size_t dstRow0, size_t dstRows, size_t *srcRow0, size_t *srcRows)
{
    if (method < 0 || method > 2 || !srcRow0 || !srcRows)
        return IQO_HIP_EINVAL;
    Plan p;
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &p, &err))
        return IQO_HIP_EINVAL;
    if (dstRow0 + dstRows > dstH)
        return IQO_HIP_EINVAL;
    int s0, s1;
    iqo_amd::band_src_rows(p, static_cast<int>(dstRow0), static_cast<int>(dstRow0 + dstRows), &s0, &s1);
    *srcRow0 = static_cast<size_t>(s0);
    *srcRows = static_cast<size_t>(s1 - s0);
    return IQO_HIP_OK;
}

int iqo_host_kernel_for_layout(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale,
                               size_t srcAlign, size_t dstAlign)
{
    if (method < 0 || method > 2 || !valid_align(srcAlign) || !valid_align(dstAlign))
        return IQO_HIP_EINVAL;
    const Layout l{srcAlign, dstAlign};  // multiples of the alignment and of nothing larger
    iqo_hip_plan h;  // host half of a plan only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &h.p, &err))
        return IQO_HIP_EINVAL;
    // a streamer family with the alignment it needs is what select_kernel returns: no table build
    if (h.p.kernel != IQO_KERNEL_GENERAL && layout_fits(&h, h.p.kernel, l))
        return h.p.kernel;
    build_host_tables(&h);
    return select_kernel(&h, l);
}

int iqo_host_kernel_for(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale)
{
    return iqo_host_kernel_for_layout(method, degree, srcW, srcH, dstW, dstH, pxScale, 16, 16);
}

int iqo_host_instance_for(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale,
                          const iqo_hip_option *options, size_t nOptions, size_t srcAlign, size_t dstAlign,
                          iqo_hip_instance *desc)
{
    if (method < 0 || method > 2 || !desc || !valid_align(srcAlign) || !valid_align(dstAlign) || (nOptions && !options))
        return IQO_HIP_EINVAL;
    iqo_hip_plan h;  // host half of a plan only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &h.p, &err))
        return IQO_HIP_EINVAL;
    build_host_tables(&h);
    for (size_t i = 0; i < nOptions; ++i) {
        const int rc = iqo_hip_plan_set_option(&h, options[i].key, options[i].value);
        if (rc)
            return rc;
    }
    return plan_instance(&h, Layout{srcAlign, dstAlign}, desc);
}

int iqo_host_launch_grid(int method, unsigned degree, int channels, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                         size_t pxScale, const iqo_hip_option *options, size_t nOptions, size_t nFrames,
                         iqo_hip_launch_grid *desc)
{
    if (method < 0 || method > 2 || channels < 1 || channels > 4 || !desc || (nOptions && !options))
        return IQO_HIP_EINVAL;
    iqo_hip_plan h;  // host half of a plan only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &h.p, &err))
        return IQO_HIP_EINVAL;
    h.channels = channels;
    build_host_tables(&h);
    for (size_t i = 0; i < nOptions; ++i) {
        const int rc = iqo_hip_plan_set_option(&h, options[i].key, options[i].value);
        if (rc)
            return rc;
    }
    return plan_launch_grid(&h, nFrames, 0, dstH, desc);
}

int iqo_host_lanczos_yfold(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH, size_t pxScale)
{
    if (method < 0 || method > 2)
        return IQO_HIP_EINVAL;
    iqo_hip_plan h;  // host half of a plan only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &h.p, &err))
        return IQO_HIP_EINVAL;
    if (h.p.kernel != IQO_KERNEL_LANCZOS_STREAM)
        return 0;
    return iqo_amd::symb_yfold(lanczos_dev(&h)) ? 1 : 0;
}

int iqo_host_layout_limits(int kernel, iqo_hip_layout_limits *out)
{
    static_assert(iqo_amd::kFamGeneral == IQO_KERNEL_GENERAL && iqo_amd::kFamLanczosStream == IQO_KERNEL_LANCZOS_STREAM &&
                      iqo_amd::kFamAreaInt == IQO_KERNEL_AREA_INT && iqo_amd::kFamLinearUp2 == IQO_KERNEL_LINEAR_UP2 &&
                      iqo_amd::kFamPackedTile == IQO_KERNEL_PACKED_TILE &&
                      iqo_amd::kFamPackedGeneral == IQO_KERNEL_PACKED_GENERAL &&
                      iqo_amd::kFamCount == IQO_KERNEL_PACKED_GENERAL + 1 && iqo_amd::kOobOffset == IQO_HIP_DROP_OFFSET,
                  "kernels.hpp kFam* are iqo_hip.h IQO_KERNEL_*");
    if (!out || kernel < 0 || kernel >= iqo_amd::kFamCount)
        return IQO_HIP_EINVAL;
    const iqo_amd::LayoutLimits m = iqo_amd::layout_limits(kernel);
    out->srcSpanMax = static_cast<uint64_t>(m.srcSpanMax);
    out->dstSpanMax = static_cast<uint64_t>(m.dstSpanMax);
    out->srcStMax = static_cast<uint64_t>(m.srcStMax);
    out->dstStMax = static_cast<uint64_t>(m.dstStMax);
    return IQO_HIP_OK;
}

int iqo_host_instance_count(int family) { return iqo_amd::instances(family).count; }

int iqo_host_instance_at(int family, int index, iqo_hip_instance *desc)
{
    const iqo_amd::InstanceList l = iqo_amd::instances(family);
    if (!desc || index < 0 || index >= l.count)
        return IQO_HIP_EINVAL;
    *desc = to_desc(l.first[index]);
    return IQO_HIP_OK;
}

int iqo_host_packed_kernel_for(int method, unsigned degree, int channels, size_t srcW, size_t srcH, size_t dstW,
                               size_t dstH, size_t pxScale)
{
    if (method < 0 || method > 2 || channels < 1 || channels > 4)
        return IQO_HIP_EINVAL;
    if (channels == 1)
        return iqo_host_kernel_for(method, degree, srcW, srcH, dstW, dstH, pxScale);
    iqo_hip_plan h;  // host half of a plan only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(static_cast<iqo_amd::Method>(method), degree, srcW, srcH, dstW, dstH, pxScale, &h.p, &err))
        return IQO_HIP_EINVAL;
    h.channels = channels;
    build_host_tables(&h);
    return plan_kernel(&h);
}

int iqo_host_yuv_chroma_full_kernel(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH,
                                    int interleavedUV)
{
    // the requests iqo_hip_plan_nv12 / iqo_hip_plan_yuv420 reject, then set_chroma's own rule and plan
    if (method < 0 || method > 2 || srcW < 2 || srcH < 2 || dstW < 2 || dstH < 2)
        return IQO_HIP_EINVAL;
    const int rc = chroma_full_status(method, srcW, srcH, dstW, dstH);
    if (rc)
        return rc;
    const unsigned deg = method == IQO_METHOD_LANCZOS ? degree : 0;
    return iqo_host_packed_kernel_for(method, deg, interleavedUV ? 2 : 1, srcW / 2, srcH / 2, dstW, dstH, 1);
}

int iqo_host_yuv420_fused(int method, unsigned degree, size_t srcW, size_t srcH, size_t dstW, size_t dstH)
{
    static_assert(int(IQO_YUV420_LZ_SYMB10) == int(iqo_amd::kYuvLzSymb10) &&
                      int(IQO_YUV420_LZ_SYM8) == int(iqo_amd::kYuvLzSym8) &&
                      int(IQO_YUV420_AREA44) == int(iqo_amd::kYuvArea44) &&
                      int(IQO_YUV420_LIN_D2) == int(iqo_amd::kYuvLinD2) &&
                      int(IQO_YUV420_LIN_UP2) == int(iqo_amd::kYuvLinUp2) &&
                      int(IQO_YUV420_LIN_UP2) + 1 == int(iqo_amd::kYuvFusedCount),
                  "iqo_hip.h IQO_YUV420_* are kernels.hpp Yuv420Fused");
    // the requests iqo_hip_plan_yuv420 rejects, and the planes as it builds them
    if (method < 0 || method > 2 || srcW < 2 || srcH < 2 || dstW < 2 || dstH < 2)
        return IQO_HIP_EINVAL;
    const iqo_amd::Method m = static_cast<iqo_amd::Method>(method);
    iqo_hip_plan hy, hc;  // host halves of the two plans only: no device memory
    std::string err;
    if (!iqo_amd::build_plan(m, degree, srcW, srcH, dstW, dstH, 1, &hy.p, &err) ||
        !iqo_amd::build_plan(m, degree, srcW / 2, srcH / 2, dstW / 2, dstH / 2, m == iqo_amd::kLanczos ? 2 : 1, &hc.p,
                             &err))
        return IQO_HIP_EINVAL;
    // as iqo_hip_resize_yuv420_device with aligned planes: one of the three fusable families on both
    const int k = hy.p.kernel;
    if (k != hc.p.kernel)
        return IQO_YUV420_NONE;
    if (k == IQO_KERNEL_LANCZOS_STREAM)
        return iqo_amd::yuv420_fused(lanczos_dev(&hy), lanczos_dev(&hc)).label;
    if (k == IQO_KERNEL_AREA_INT)
        return iqo_amd::yuv420_fused(area_dev(&hy), area_dev(&hc)).label;
    if (k == IQO_KERNEL_LINEAR_UP2)
        return iqo_amd::yuv420_fused(linear_dev(&hy), linear_dev(&hc)).label;
    return IQO_YUV420_NONE;
}

} // extern "C"

// ---------------------------------------------------------------- batched crop-and-resize (roi.hpp)

// What a plan of either box family holds.  Two arenas, used alternately: pinned host words, their device copy
// and the event recorded after the launch that reads the device copy.
struct RoiPlanCore {
    RoiPlanCore(int method, unsigned degree, size_t dstW, size_t dstH, int device_)
        : cache(static_cast<iqo_amd::Method>(method), degree, static_cast<int>(dstW), static_cast<int>(dstH)), device(device_)
    {
    }
    iqo_amd::RoiTableCache cache;
    iqo_amd::RoiLayout layout;
    int device;
    struct Arena {
        uint32_t *h = nullptr, *d = nullptr;
        size_t capWords = 0;
        hipEvent_t ev = nullptr;
        bool pending = false;
    } arena[2];
    int next = 0;
};
struct iqo_hip_roi_plan {
    RoiPlanCore core;
    int channels;
};
struct iqo_hip_roi_yuv_plan {
    RoiPlanCore core;
    int layout;
};

namespace {

static_assert(sizeof(iqo_hip_roi) == sizeof(iqo_amd::RoiBox), "iqo_hip_roi is roi.hpp RoiBox");
static_assert(IQO_HIP_ROI_MAX_TAPS == iqo_amd::kRoiMaxTaps && IQO_HIP_ROI_LDS_BYTES == iqo_amd::kRoiLdsMax,
              "iqo_hip.h roi limits are roi.hpp's");
static_assert(IQO_ROI_NV12 == iqo_amd::kRoiNv12 && IQO_ROI_I420 == iqo_amd::kRoiI420, "iqo_hip.h layouts are roi.hpp's");

int roi_status(int st) { return st == iqo_amd::kRoiOk ? IQO_HIP_OK : st == iqo_amd::kRoiInvalid ? IQO_HIP_EINVAL : IQO_HIP_EUNSUP; }

// A layout call that failed at box `bad`
int roi_fail(int st, int bad, int *badRoi)
{
    if (badRoi)
        *badRoi = bad;
    return roi_status(st);
}

bool roi_dst_dims_ok(size_t dstW, size_t dstH) { return dstW && dstH && dstW <= (1u << 20) && dstH <= (1u << 20); }

const iqo_amd::RoiBox *roi_boxes(const iqo_hip_roi *rois) { return reinterpret_cast<const iqo_amd::RoiBox *>(rois); }

// What a fit call brings beyond its stretch twin (nullptr in the calls below: a stretch call)
struct RoiFit {
    const iqo_hip_roi_rect *rects;  // nRois of them, or nullptr: the whole output
    const uint8_t *pad;             // 4 bytes, or nullptr: zeros
    const iqo_amd::RoiRect *rois() const { return reinterpret_cast<const iqo_amd::RoiRect *>(rects); }
    void colour(uint8_t out[4]) const
    {
        for (int c = 0; c < 4; ++c)
            out[c] = pad ? pad[c] : 0;
    }
};
static_assert(sizeof(iqo_hip_roi_rect) == sizeof(iqo_amd::RoiRect), "iqo_hip_roi_rect is roi.hpp RoiRect");
static_assert(IQO_FIT_STRETCH == iqo_amd::kFitStretch && IQO_FIT_LETTERBOX == iqo_amd::kFitLetterbox &&
                  IQO_FIT_LETTERBOX_TOPLEFT == iqo_amd::kFitLetterboxTopLeft,
              "iqo_hip.h fit modes are roi.hpp's");

// The destination checks of both forms (norm == nullptr: interleaved bytes); fills *rn for the twin.
int roi_check_dst(int channels, size_t dstW, size_t dstH, size_t nRois, const iqo_hip_norm *norm, bool isNorm,
                  size_t dstSt, size_t planeSt, size_t dstRoiSt, const void *dst, iqo_amd::RoiNorm *rn)
{
    *rn = iqo_amd::RoiNorm();
    if ((!dst && nRois) || !roi_dst_dims_ok(dstW, dstH))
        return IQO_HIP_EINVAL;
    if (!isNorm) {
        if (dstSt < dstW * static_cast<size_t>(channels) || (nRois > 1 && dstRoiSt / dstH < dstSt))
            return IQO_HIP_EINVAL;
        return IQO_HIP_OK;
    }
    if (!norm || (norm->dtype != IQO_OUT_F32 && norm->dtype != IQO_OUT_F16 && norm->dtype != IQO_OUT_BF16) ||
        norm->planes < 1 || norm->planes > 4)
        return IQO_HIP_EINVAL;
    for (int i = 0; i < norm->planes; ++i)
        if (norm->order[i] < 0 || norm->order[i] >= channels || !std::isfinite(norm->scale[i]) ||
            !std::isfinite(norm->bias[i]))
            return IQO_HIP_EINVAL;
    const size_t elem = norm->dtype == IQO_OUT_F32 ? 4 : 2, planes = static_cast<size_t>(norm->planes);
    if (reinterpret_cast<uintptr_t>(dst) % elem || dstSt % elem || planeSt % elem || dstRoiSt % elem)
        return IQO_HIP_EINVAL;
    if (dstSt < dstW * elem || planeSt / dstH < dstSt || (nRois > 1 && dstRoiSt / planes < planeSt) ||
        planeSt >= (size_t(1) << 31))
        return IQO_HIP_EINVAL;
    rn->dtype = norm->dtype;
    rn->planes = norm->planes;
    for (int i = 0; i < norm->planes; ++i) {
        rn->order[i] = norm->order[i];
        rn->scale[i] = norm->scale[i];
        rn->bias[i] = norm->bias[i];
    }
    return IQO_HIP_OK;
}

iqo_amd::NormDev norm_dev(const iqo_amd::RoiNorm &rn, size_t planeSt)
{
    iqo_amd::NormDev n;
    n.dtype = rn.dtype;
    n.planes = rn.planes;
    n.planeSt = static_cast<int>(planeSt);
    for (int i = 0; i < 4; ++i) {
        n.order[i] = rn.order[i];
        n.scale[i] = rn.scale[i];
        n.bias[i] = rn.bias[i];
    }
    return n;
}

void roi_stats(const iqo_amd::RoiLayout &l, int recWords, iqo_hip_roi_arena_stats *stats)
{
    stats->arenaBytes = l.words * 4;
    stats->xTables = l.nXTables;
    stats->yTables = l.nYTables;
    stats->workgroups = l.groups;
    stats->ldsBytes = l.ldsBytes;
    stats->recordBytes = static_cast<size_t>(recWords) * 4;
}

void roi_arena_free(RoiPlanCore::Arena *a)
{
    if (a->h)
        (void)hipHostFree(a->h);
    if (a->d)
        (void)hipFree(a->d);
    a->h = a->d = nullptr;
    a->capWords = 0;
}

// Makes `a` ready to be filled with `words` words: waits for the launch that last read it, and grows it.
int roi_arena_reserve(RoiPlanCore::Arena *a, size_t words)
{
    if (a->pending) {
        if (hipEventSynchronize(a->ev) != hipSuccess)
            return IQO_HIP_EHIP;
        a->pending = false;
    }
    if (a->capWords < words) {
        roi_arena_free(a);
        const size_t cap2 = std::max(words + words / 2, size_t(1) << 16);
        if (hipHostMalloc(reinterpret_cast<void **>(&a->h), cap2 * 4, hipHostMallocDefault) != hipSuccess ||
            hipMalloc(reinterpret_cast<void **>(&a->d), cap2 * 4) != hipSuccess) {
            roi_arena_free(a);
            return IQO_HIP_ENOMEM;
        }
        a->capWords = cap2;
    }
    return IQO_HIP_OK;
}

template <typename Plan>
void roi_plan_destroy(Plan *h)
{
    if (!h)
        return;
    {
        DeviceGuard guard(h->core.device);
        for (auto &a : h->core.arena) {
            if (a.pending)
                (void)hipEventSynchronize(a.ev);
            if (a.ev)
                (void)hipEventDestroy(a.ev);
            roi_arena_free(&a);
        }
    }
    delete h;
}

// A plan of either family; `variant` (channels / layout) was found to be `variantStatus` by the caller.
template <typename Plan>
int roi_plan_create(int method, unsigned degree, int variant, int variantStatus, size_t dstW, size_t dstH, int device,
                    Plan **out)
{
    if (!out)
        return IQO_HIP_EINVAL;
    *out = nullptr;
    if (method < 0 || method > 2 || (method == IQO_METHOD_LANCZOS && degree < 1) || !roi_dst_dims_ok(dstW, dstH))
        return IQO_HIP_EINVAL;
    if (variantStatus)
        return variantStatus;
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count || !is_gfx950(device))
        return IQO_HIP_ENODEV;
    DeviceGuard guard(device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    Plan *h = new (std::nothrow) Plan{RoiPlanCore(method, degree, dstW, dstH, device), variant};
    if (!h)
        return IQO_HIP_ENOMEM;
    for (auto &a : h->core.arena)
        if (hipEventCreateWithFlags(&a.ev, hipEventDisableTiming) != hipSuccess) {
            roi_plan_destroy(h);
            return IQO_HIP_EHIP;
        }
    *out = h;
    return IQO_HIP_OK;
}

// The laid-out call of p->layout on stream s: fill(host words) writes the arena, launch(device words) starts the
// kernel on its copy.
template <typename Fill, typename Launch>
int roi_submit(RoiPlanCore *p, Fill fill, Launch launch, hipStream_t s)
{
    const size_t words = p->layout.words;
    DeviceGuard guard(p->device);
    if (!guard.ok())
        return IQO_HIP_ENODEV;
    hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &cap) != hipSuccess)
        return IQO_HIP_EHIP;
    if (cap != hipStreamCaptureStatusNone)
        return IQO_HIP_EUNSUP;  // the tables are per call: nothing to replay
    RoiPlanCore::Arena &a = p->arena[p->next];
    const int ra = roi_arena_reserve(&a, words);
    if (ra)
        return ra;
    fill(a.h);
    if (hipMemcpyAsync(a.d, a.h, words * 4, hipMemcpyHostToDevice, s) != hipSuccess)
        return IQO_HIP_EHIP;
    a.pending = true;  // from here on the arena is in flight, whatever follows
    const hipError_t e = launch(a.d);
    const hipError_t e2 = hipEventRecord(a.ev, s);
    p->next ^= 1;
    if (e == hipErrorInvalidValue)
        return IQO_HIP_EINVAL;
    return e == hipSuccess && e2 == hipSuccess ? IQO_HIP_OK : IQO_HIP_EHIP;
}

int host_rois(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois, const iqo_hip_roi *rois,
              size_t nFrames, size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt, const uint8_t *src,
              const iqo_hip_norm *norm, bool isNorm, size_t dstSt, size_t planeSt, size_t dstRoiSt, void *dst,
              iqo_hip_roi_arena_stats *stats, int *badRoi, const RoiFit *fit = nullptr)
{
    int bad = -1;
    if (badRoi)
        *badRoi = -1;
    if (method < 0 || method > 2)
        return IQO_HIP_EINVAL;
    if (channels != 1 && channels != 3 && channels != 4)
        return IQO_HIP_EUNSUP;
    iqo_amd::RoiNorm rn;
    if (!stats) {
        if (!src && nRois)
            return IQO_HIP_EINVAL;
        const int rc = roi_check_dst(channels, dstW, dstH, nRois, norm, isNorm, dstSt, planeSt, dstRoiSt, dst, &rn);
        if (rc)
            return rc;
    } else if (!roi_dst_dims_ok(dstW, dstH)) {
        return IQO_HIP_EINVAL;
    }
    iqo_amd::RoiTableCache cache(static_cast<iqo_amd::Method>(method), degree, static_cast<int>(dstW), static_cast<int>(dstH));
    iqo_amd::RoiLayout l;
    const int st = fit ? iqo_amd::roi_fit_layout(&cache, channels, nRois, roi_boxes(rois), fit->rois(), nFrames, frameW, frameH,
                                                 srcSt, srcFrameSt, &l, &bad)
                       : iqo_amd::roi_layout(&cache, channels, nRois, roi_boxes(rois), nFrames, frameW, frameH, srcSt, srcFrameSt,
                                             &l, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_fail(st, bad, badRoi);
    if (stats) {
        roi_stats(l, fit ? iqo_amd::kRoiFitRecWords : iqo_amd::kRoiRecWords, stats);
        return IQO_HIP_OK;
    }
    std::vector<uint32_t> arena(l.words);
    if (fit) {
        uint8_t pad[4];
        fit->colour(pad);
        iqo_amd::roi_fit_fill(cache, l, frameW, arena.data());
        iqo_amd::roi_fit_walk(arena.data(), src, srcSt, dstSt, planeSt, dstRoiSt, dst, rn, pad);
        return IQO_HIP_OK;
    }
    iqo_amd::roi_fill(cache, l, frameW, arena.data());
    iqo_amd::roi_walk(arena.data(), src, srcSt, dstSt, planeSt, dstRoiSt, dst, rn);
    return IQO_HIP_OK;
}

int run_rois(iqo_hip_roi_plan *h, size_t nRois, const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
             size_t srcSt, size_t srcFrameSt, const uint8_t *src, const iqo_hip_norm *norm, bool isNorm, size_t dstSt,
             size_t planeSt, size_t dstRoiSt, void *dst, hipStream_t s, int *badRoi, const RoiFit *fit = nullptr)
{
    if (badRoi)
        *badRoi = -1;
    if (!h || (!src && nRois))
        return IQO_HIP_EINVAL;
    RoiPlanCore &p = h->core;
    iqo_amd::RoiNorm rn;
    const int rc = roi_check_dst(h->channels, static_cast<size_t>(p.cache.dstW()), static_cast<size_t>(p.cache.dstH()), nRois,
                                 norm, isNorm, dstSt, planeSt, dstRoiSt, dst, &rn);
    if (rc)
        return rc;
    int bad = -1;
    const int st = fit ? iqo_amd::roi_fit_layout(&p.cache, h->channels, nRois, roi_boxes(rois), fit->rois(), nFrames, frameW,
                                                 frameH, srcSt, srcFrameSt, &p.layout, &bad)
                       : iqo_amd::roi_layout(&p.cache, h->channels, nRois, roi_boxes(rois), nFrames, frameW, frameH, srcSt,
                                             srcFrameSt, &p.layout, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_fail(st, bad, badRoi);
    if (nRois == 0)
        return IQO_HIP_OK;
    return roi_submit(
        &p,
        [&](uint32_t *words) {
            if (fit)
                iqo_amd::roi_fit_fill(p.cache, p.layout, frameW, words);
            else
                iqo_amd::roi_fill(p.cache, p.layout, frameW, words);
        },
        [&](const uint32_t *words) {
            iqo_amd::RoiDev d;
            d.arena = words;
            d.src = src;
            d.dst = static_cast<uint8_t *>(dst);
            d.srcSt = static_cast<int64_t>(srcSt);
            d.dstSt = static_cast<int64_t>(dstSt);
            d.dstRoiSt = static_cast<int64_t>(dstRoiSt);
            d.lanczos = p.cache.method() == iqo_amd::kLanczos;
            d.channels = h->channels;
            d.groups = p.layout.groups;
            d.ldsBytes = p.layout.ldsBytes;
            d.fit = fit != nullptr;
            if (fit)
                fit->colour(d.pad);
            const iqo_amd::NormDev n = norm_dev(rn, planeSt);
            return iqo_amd::launch_roi(d, isNorm ? &n : nullptr, s);
        },
        s);
}

} // namespace

extern "C" {

int iqo_hip_plan_rois(int method, unsigned degree, int channels, size_t dstW, size_t dstH, int device,
                      iqo_hip_roi_plan **out)
{
    const bool ok = channels == 1 || channels == 3 || channels == 4;
    return roi_plan_create(method, degree, channels, ok ? IQO_HIP_OK : IQO_HIP_EUNSUP, dstW, dstH, device, out);
}

void iqo_hip_roi_plan_destroy(iqo_hip_roi_plan *h) { roi_plan_destroy(h); }

int iqo_hip_resize_rois_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                               size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                               size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream, int *badRoi)
{
    return run_rois(plan, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, dSrc, nullptr, false, dstSt, 0,
                    dstRoiSt, dDst, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_hip_resize_rois_norm_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                    size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                                    const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt,
                                    void *dDst, void *stream, int *badRoi)
{
    return run_rois(plan, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, dSrc, norm, true, dstSt, dstPlaneSt,
                    dstRoiSt, dDst, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_host_resize_rois(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                         const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                         size_t srcFrameSt, const uint8_t *src, size_t dstSt, size_t dstRoiSt, uint8_t *dst, int *badRoi)
{
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, src,
                     nullptr, false, dstSt, 0, dstRoiSt, dst, nullptr, badRoi);
}

int iqo_host_resize_rois_norm(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                              const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                              size_t srcFrameSt, const uint8_t *src, const iqo_hip_norm *norm, size_t dstSt,
                              size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi)
{
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, src,
                     norm, true, dstSt, dstPlaneSt, dstRoiSt, dst, nullptr, badRoi);
}

int iqo_host_roi_arena_stats(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                             const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                             iqo_hip_roi_arena_stats *stats, int *badRoi)
{
    if (!stats)
        return IQO_HIP_EINVAL;
    const size_t C = channels > 0 ? static_cast<size_t>(channels) : 1;
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, frameW * C,
                     frameW * C * frameH, nullptr, nullptr, false, 0, 0, 0, nullptr, stats, badRoi);
}

int iqo_hip_resize_rois_fit_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                   size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                                   size_t dstSt, size_t dstRoiSt, uint8_t *dDst, void *stream, int *badRoi,
                                   const iqo_hip_roi_rect *rects, const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    return run_rois(plan, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, dSrc, nullptr, false, dstSt, 0,
                    dstRoiSt, dDst, static_cast<hipStream_t>(stream), badRoi, &fit);
}

int iqo_hip_resize_rois_fit_norm_device(iqo_hip_roi_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                        size_t frameW, size_t frameH, size_t srcSt, size_t srcFrameSt, const uint8_t *dSrc,
                                        const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt,
                                        void *dDst, void *stream, int *badRoi, const iqo_hip_roi_rect *rects,
                                        const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    return run_rois(plan, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, dSrc, norm, true, dstSt, dstPlaneSt,
                    dstRoiSt, dDst, static_cast<hipStream_t>(stream), badRoi, &fit);
}

int iqo_host_resize_rois_fit(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                             const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                             size_t srcFrameSt, const uint8_t *src, size_t dstSt, size_t dstRoiSt, uint8_t *dst, int *badRoi,
                             const iqo_hip_roi_rect *rects, const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, src,
                     nullptr, false, dstSt, 0, dstRoiSt, dst, nullptr, badRoi, &fit);
}

int iqo_host_resize_rois_fit_norm(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                                  const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcSt,
                                  size_t srcFrameSt, const uint8_t *src, const iqo_hip_norm *norm, size_t dstSt,
                                  size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi, const iqo_hip_roi_rect *rects,
                                  const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, srcSt, srcFrameSt, src,
                     norm, true, dstSt, dstPlaneSt, dstRoiSt, dst, nullptr, badRoi, &fit);
}

int iqo_host_roi_fit_arena_stats(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                 iqo_hip_roi_arena_stats *stats, int *badRoi, const iqo_hip_roi_rect *rects)
{
    if (!stats)
        return IQO_HIP_EINVAL;
    const size_t C = channels > 0 ? static_cast<size_t>(channels) : 1;
    const RoiFit fit = {rects, nullptr};
    return host_rois(method, degree, channels, dstW, dstH, nRois, rois, nFrames, frameW, frameH, frameW * C,
                     frameW * C * frameH, nullptr, nullptr, false, 0, 0, 0, nullptr, stats, badRoi, &fit);
}

int iqo_host_fit_rect(int mode, size_t w, size_t h, size_t dstW, size_t dstH, iqo_hip_roi_rect *out)
{
    iqo_amd::RoiRect r;
    if (!out || !iqo_amd::fit_rect(mode, w, h, dstW, dstH, &r))
        return IQO_HIP_EINVAL;
    *out = iqo_hip_roi_rect{r.x, r.y, r.w, r.h};
    return IQO_HIP_OK;
}

} // extern "C"

namespace {

// The pad words of a one-box fit layout's record
template <typename Out>
void fit_box_pads(const uint32_t *ext, Out *out)
{
    out->padAbove = ext[iqo_amd::kFPadAbove];
    out->padBelow = ext[iqo_amd::kFPadBelow];
    out->padRows = iqo_amd::kRoiPadRows;
}

// iqo_host_roi_box_layout (fit == nullptr) and iqo_host_roi_fit_box_layout (*pads: its pad words)
int roi_box_layout(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t w, size_t h, const RoiFit *fit,
                   iqo_hip_roi_box_layout *out, iqo_hip_roi_fit_box_layout *pads)
{
    if (!out || method < 0 || method > 2 || !roi_dst_dims_ok(dstW, dstH) || !w || !h || w > (1u << 24) || h > (1u << 24))
        return IQO_HIP_EINVAL;
    // the box as the whole of one tightly packed frame: roi_layout on a one-box call, as the device call
    const size_t C = channels > 0 ? static_cast<size_t>(channels) : 1;
    const iqo_amd::RoiBox box = {0, 0, 0, static_cast<int>(w), static_cast<int>(h), 0};
    iqo_amd::RoiTableCache cache(static_cast<iqo_amd::Method>(method), degree, static_cast<int>(dstW), static_cast<int>(dstH));
    iqo_amd::RoiLayout l;
    int bad = -1;
    const int st = fit ? iqo_amd::roi_fit_layout(&cache, channels, 1, &box, fit->rois(), 1, w, h, w * C, w * C * h, &l, &bad)
                       : iqo_amd::roi_layout(&cache, channels, 1, &box, 1, w, h, w * C, w * C * h, &l, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_status(st);
    if (fit)
        fit_box_pads(l.rec.data() + iqo_amd::kRoiFitExt, pads);
    const uint32_t *xt = l.tables[static_cast<size_t>(l.xIdx[0].second)].first->data();
    const uint32_t *yt = l.tables[static_cast<size_t>(l.yIdx[0].second)].first->data();
    out->rows = static_cast<int>(l.rec[iqo_amd::kRRows]);
    out->workgroups = l.rec[iqo_amd::kRGroups];
    out->ldsBytes = l.ldsBytes;
    out->nYp = static_cast<int>(yt[0]);
    out->np = static_cast<int>(xt[0]);
    out->pitchDw = static_cast<int>(l.rec[iqo_amd::kRPitch]);
    return IQO_HIP_OK;
}

} // namespace

extern "C" {

int iqo_host_roi_box_layout(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t w, size_t h,
                            iqo_hip_roi_box_layout *out)
{
    return roi_box_layout(method, degree, channels, dstW, dstH, w, h, nullptr, out, nullptr);
}

int iqo_host_roi_fit_box_layout(int method, unsigned degree, int channels, size_t dstW, size_t dstH, size_t w, size_t h,
                                const iqo_hip_roi_rect *rect, iqo_hip_roi_fit_box_layout *out)
{
    const RoiFit fit = {rect, nullptr};
    return roi_box_layout(method, degree, channels, dstW, dstH, w, h, &fit, out ? &out->box : nullptr, out);
}

} // extern "C"

// ---------------------------------------------------------------- boxes of NV12 / I420 frames to RGB (roi.hpp)

namespace {

// The source and the output of a YUV box call, as the C entries take them.
struct RoiYuvCall {
    size_t nRois;
    const iqo_hip_roi *rois;
    size_t nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt;
    const uint8_t *y, *u, *v;
    int standard, channels;
    const int *order;          // packed bytes: channels entries
    const iqo_hip_norm *norm;  // float planes (isNorm)
    bool isNorm;
    size_t dstSt, planeSt, dstRoiSt;
    void *dst;
    const RoiFit *fit;         // nullptr: a stretch call
};

// The checks of a call's own arguments that roi_yuv_layout does not make; fills *src and *out.
int roi_yuv_check(int layout, size_t dstW, size_t dstH, const RoiYuvCall &c, bool needPlanes, iqo_amd::RoiYuvSrc *src,
                  iqo_amd::RoiYuvOut *out)
{
    if (layout != IQO_ROI_NV12 && layout != IQO_ROI_I420)
        return IQO_HIP_EINVAL;
    if (c.standard < 0 || c.standard >= iqo_amd::kYuvRgbStandards)
        return IQO_HIP_EINVAL;
    if (needPlanes && c.nRois && (!c.y || !c.u || (layout == IQO_ROI_I420 && !c.v)))
        return IQO_HIP_EINVAL;
    *out = iqo_amd::RoiYuvOut();
    out->standard = c.standard;
    if (!c.isNorm) {
        if ((c.channels != 3 && c.channels != 4) || !c.order)
            return IQO_HIP_EINVAL;
        for (int i = 0; i < c.channels; ++i) {
            if (c.order[i] < 0 || c.order[i] > 3)
                return IQO_HIP_EINVAL;
            out->order[i] = c.order[i];
        }
        out->channels = c.channels;
    }
    if (needPlanes) {
        const int rc = roi_check_dst(c.isNorm ? 3 : c.channels, dstW, dstH, c.nRois, c.norm, c.isNorm, c.dstSt, c.planeSt,
                                     c.dstRoiSt, c.dst, &out->n);
        if (rc)
            return rc;
    } else if (!roi_dst_dims_ok(dstW, dstH)) {
        return IQO_HIP_EINVAL;
    }
    src->layout = layout;
    src->nFrames = c.nFrames;
    src->frameW = c.frameW;
    src->frameH = c.frameH;
    src->stY = c.srcStY;
    src->stUV = c.srcStUV;
    src->frameSt = c.srcFrameSt;
    return IQO_HIP_OK;
}

int host_rois_yuv(int method, unsigned degree, int layout, size_t dstW, size_t dstH, const RoiYuvCall &c,
                  iqo_hip_roi_arena_stats *stats, int *badRoi)
{
    int bad = -1;
    if (badRoi)
        *badRoi = -1;
    if (method < 0 || method > 2)
        return IQO_HIP_EINVAL;
    iqo_amd::RoiYuvSrc src;
    iqo_amd::RoiYuvOut out;
    const int rc = roi_yuv_check(layout, dstW, dstH, c, !stats, &src, &out);
    if (rc)
        return rc;
    iqo_amd::RoiTableCache cache(static_cast<iqo_amd::Method>(method), degree, static_cast<int>(dstW), static_cast<int>(dstH));
    iqo_amd::RoiLayout l;
    const int st = c.fit ? iqo_amd::roi_yuv_fit_layout(&cache, src, c.nRois, roi_boxes(c.rois), c.fit->rois(), &l, &bad)
                         : iqo_amd::roi_yuv_layout(&cache, src, c.nRois, roi_boxes(c.rois), &l, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_fail(st, bad, badRoi);
    if (stats) {
        roi_stats(l, c.fit ? iqo_amd::kRoiYuvFitRecWords : iqo_amd::kRoiYuvRecWords, stats);
        return IQO_HIP_OK;
    }
    std::vector<uint32_t> arena(l.words);
    if (c.fit) {
        uint8_t pad[4];
        c.fit->colour(pad);
        iqo_amd::roi_yuv_fit_fill(cache, l, src, arena.data());
        iqo_amd::roi_yuv_fit_walk(arena.data(), c.y, c.u, c.v, out, c.dstSt, c.planeSt, c.dstRoiSt, c.dst, pad);
        return IQO_HIP_OK;
    }
    iqo_amd::roi_yuv_fill(cache, l, src, arena.data());
    iqo_amd::roi_yuv_walk(arena.data(), c.y, c.u, c.v, out, c.dstSt, c.planeSt, c.dstRoiSt, c.dst);
    return IQO_HIP_OK;
}

int run_rois_yuv(iqo_hip_roi_yuv_plan *h, const RoiYuvCall &c, hipStream_t s, int *badRoi)
{
    if (badRoi)
        *badRoi = -1;
    if (!h)
        return IQO_HIP_EINVAL;
    RoiPlanCore &p = h->core;
    iqo_amd::RoiYuvSrc src;
    iqo_amd::RoiYuvOut out;
    const int rc = roi_yuv_check(h->layout, static_cast<size_t>(p.cache.dstW()), static_cast<size_t>(p.cache.dstH()), c, true,
                                 &src, &out);
    if (rc)
        return rc;
    int bad = -1;
    const int st = c.fit ? iqo_amd::roi_yuv_fit_layout(&p.cache, src, c.nRois, roi_boxes(c.rois), c.fit->rois(), &p.layout, &bad)
                         : iqo_amd::roi_yuv_layout(&p.cache, src, c.nRois, roi_boxes(c.rois), &p.layout, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_fail(st, bad, badRoi);
    if (c.nRois == 0)
        return IQO_HIP_OK;
    return roi_submit(
        &p,
        [&](uint32_t *words) {
            if (c.fit)
                iqo_amd::roi_yuv_fit_fill(p.cache, p.layout, src, words);
            else
                iqo_amd::roi_yuv_fill(p.cache, p.layout, src, words);
        },
        [&](const uint32_t *words) {
            iqo_amd::RoiYuvDev d;
            d.arena = words;
            d.y = c.y;
            d.u = c.u;
            d.v = c.v;
            d.dst = static_cast<uint8_t *>(c.dst);
            d.dstSt = static_cast<int64_t>(c.dstSt);
            d.dstRoiSt = static_cast<int64_t>(c.dstRoiSt);
            d.lanczos = p.cache.method() == iqo_amd::kLanczos;
            d.interleavedUV = h->layout == IQO_ROI_NV12;
            d.k = iqo_amd::kYuvRgb[c.standard];
            d.channels = out.channels;
            for (int i = 0; i < 4; ++i)
                d.order[i] = out.order[i];
            d.groups = p.layout.groups;
            d.ldsBytes = p.layout.ldsBytes;
            d.fit = c.fit != nullptr;
            if (c.fit)
                c.fit->colour(d.pad);
            const iqo_amd::NormDev n = norm_dev(out.n, c.planeSt);
            return iqo_amd::launch_roi_yuv(d, c.isNorm ? &n : nullptr, s);
        },
        s);
}

} // namespace

extern "C" {

int iqo_hip_plan_rois_yuv(int method, unsigned degree, int layout, size_t dstW, size_t dstH, int device,
                          iqo_hip_roi_yuv_plan **out)
{
    const bool ok = layout == IQO_ROI_NV12 || layout == IQO_ROI_I420;
    return roi_plan_create(method, degree, layout, ok ? IQO_HIP_OK : IQO_HIP_EINVAL, dstW, dstH, device, out);
}

void iqo_hip_roi_yuv_plan_destroy(iqo_hip_roi_yuv_plan *h) { roi_plan_destroy(h); }

int iqo_hip_resize_rois_yuv_rgb_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                       size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                                       const uint8_t *dY, const uint8_t *dUorUV, const uint8_t *dV, int standard,
                                       int channels, const int *order, size_t dstSt, size_t dstRoiSt, uint8_t *dDst,
                                       void *stream, int *badRoi)
{
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, dY, dUorUV, dV, standard,
                          channels, order, nullptr, false, dstSt, 0, dstRoiSt, dDst, nullptr};
    return run_rois_yuv(plan, c, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_hip_resize_rois_yuv_norm_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                        size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                                        const uint8_t *dY, const uint8_t *dUorUV, const uint8_t *dV, int standard,
                                        const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt,
                                        void *dDst, void *stream, int *badRoi)
{
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, dY, dUorUV, dV, standard,
                          3, nullptr, norm, true, dstSt, dstPlaneSt, dstRoiSt, dDst, nullptr};
    return run_rois_yuv(plan, c, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_host_resize_rois_yuv_rgb(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                 size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                 const uint8_t *v, int standard, int channels, const int *order, size_t dstSt,
                                 size_t dstRoiSt, uint8_t *dst, int *badRoi)
{
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, y, uOrUV, v, standard,
                          channels, order, nullptr, false, dstSt, 0, dstRoiSt, dst, nullptr};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, nullptr, badRoi);
}

int iqo_host_resize_rois_yuv_norm(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                  const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                  size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                  const uint8_t *v, int standard, const iqo_hip_norm *norm, size_t dstSt,
                                  size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi)
{
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, y, uOrUV, v, standard,
                          3, nullptr, norm, true, dstSt, dstPlaneSt, dstRoiSt, dst, nullptr};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, nullptr, badRoi);
}

int iqo_host_roi_yuv_arena_stats(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                 const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                 iqo_hip_roi_arena_stats *stats, int *badRoi)
{
    if (!stats)
        return IQO_HIP_EINVAL;
    const size_t stUV = layout == IQO_ROI_NV12 ? frameW : frameW / 2;
    // (no planes and no destination: tightly packed frames, and the output form plays no part in the arena)
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, frameW, stUV, frameW * frameH * 3 / 2, nullptr, nullptr,
                          nullptr, 0, 3, nullptr, nullptr, true, 0, 0, 0, nullptr, nullptr};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, stats, badRoi);
}

int iqo_hip_resize_rois_yuv_fit_rgb_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                           size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                                           const uint8_t *dY, const uint8_t *dUorUV, const uint8_t *dV, int standard,
                                           int channels, const int *order, size_t dstSt, size_t dstRoiSt, uint8_t *dDst,
                                           void *stream, int *badRoi, const iqo_hip_roi_rect *rects, const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, dY, dUorUV, dV, standard,
                          channels, order, nullptr, false, dstSt, 0, dstRoiSt, dDst, &fit};
    return run_rois_yuv(plan, c, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_hip_resize_rois_yuv_fit_norm_device(iqo_hip_roi_yuv_plan *plan, size_t nRois, const iqo_hip_roi *rois, size_t nFrames,
                                            size_t frameW, size_t frameH, size_t srcStY, size_t srcStUV, size_t srcFrameSt,
                                            const uint8_t *dY, const uint8_t *dUorUV, const uint8_t *dV, int standard,
                                            const iqo_hip_norm *norm, size_t dstSt, size_t dstPlaneSt, size_t dstRoiSt,
                                            void *dDst, void *stream, int *badRoi, const iqo_hip_roi_rect *rects,
                                            const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, dY, dUorUV, dV, standard,
                          3, nullptr, norm, true, dstSt, dstPlaneSt, dstRoiSt, dDst, &fit};
    return run_rois_yuv(plan, c, static_cast<hipStream_t>(stream), badRoi);
}

int iqo_host_resize_rois_yuv_fit_rgb(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                     const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                     size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                     const uint8_t *v, int standard, int channels, const int *order, size_t dstSt,
                                     size_t dstRoiSt, uint8_t *dst, int *badRoi, const iqo_hip_roi_rect *rects,
                                     const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, y, uOrUV, v, standard,
                          channels, order, nullptr, false, dstSt, 0, dstRoiSt, dst, &fit};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, nullptr, badRoi);
}

int iqo_host_resize_rois_yuv_fit_norm(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                      const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH, size_t srcStY,
                                      size_t srcStUV, size_t srcFrameSt, const uint8_t *y, const uint8_t *uOrUV,
                                      const uint8_t *v, int standard, const iqo_hip_norm *norm, size_t dstSt,
                                      size_t dstPlaneSt, size_t dstRoiSt, void *dst, int *badRoi,
                                      const iqo_hip_roi_rect *rects, const uint8_t pad[4])
{
    const RoiFit fit = {rects, pad};
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, srcStY, srcStUV, srcFrameSt, y, uOrUV, v, standard,
                          3, nullptr, norm, true, dstSt, dstPlaneSt, dstRoiSt, dst, &fit};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, nullptr, badRoi);
}

int iqo_host_roi_yuv_fit_arena_stats(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t nRois,
                                     const iqo_hip_roi *rois, size_t nFrames, size_t frameW, size_t frameH,
                                     iqo_hip_roi_arena_stats *stats, int *badRoi, const iqo_hip_roi_rect *rects)
{
    if (!stats)
        return IQO_HIP_EINVAL;
    const size_t stUV = layout == IQO_ROI_NV12 ? frameW : frameW / 2;
    const RoiFit fit = {rects, nullptr};
    const RoiYuvCall c = {nRois, rois, nFrames, frameW, frameH, frameW, stUV, frameW * frameH * 3 / 2, nullptr, nullptr,
                          nullptr, 0, 3, nullptr, nullptr, true, 0, 0, 0, nullptr, &fit};
    return host_rois_yuv(method, degree, layout, dstW, dstH, c, stats, badRoi);
}

} // extern "C"

namespace {

// iqo_host_roi_yuv_box_layout (fit == nullptr) and iqo_host_roi_yuv_fit_box_layout (*pads: its pad words)
int roi_yuv_box_layout(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t w, size_t h, const RoiFit *fit,
                       iqo_hip_roi_yuv_box_layout *out, iqo_hip_roi_yuv_fit_box_layout *pads)
{
    if (!out || method < 0 || method > 2 || !roi_dst_dims_ok(dstW, dstH) || !w || !h || w > (1u << 24) || h > (1u << 24))
        return IQO_HIP_EINVAL;
    // the box as the whole of one tightly packed frame: roi_yuv_layout on a one-box call, as the device call
    const iqo_amd::RoiBox box = {0, 0, 0, static_cast<int>(w), static_cast<int>(h), 0};
    iqo_amd::RoiYuvSrc src;
    src.layout = layout;
    src.nFrames = 1;
    src.frameW = src.stY = w;
    src.frameH = h;
    src.stUV = layout == IQO_ROI_NV12 ? w : w / 2;
    src.frameSt = w * h * 3 / 2;
    iqo_amd::RoiTableCache cache(static_cast<iqo_amd::Method>(method), degree, static_cast<int>(dstW), static_cast<int>(dstH));
    iqo_amd::RoiLayout l;
    int bad = -1;
    const int st = fit ? iqo_amd::roi_yuv_fit_layout(&cache, src, 1, &box, fit->rois(), &l, &bad)
                       : iqo_amd::roi_yuv_layout(&cache, src, 1, &box, &l, &bad);
    if (st != iqo_amd::kRoiOk)
        return roi_status(st);
    const uint32_t *r = l.rec.data();
    if (fit)
        fit_box_pads(r + iqo_amd::kRoiYuvFitExt, pads);
    auto tab = [&](int word) {  // the table at arena word offset r[word]
        for (const auto &t : l.tables)
            if (t.second == r[word])
                return t.first->data();
        return static_cast<const uint32_t *>(nullptr);
    };
    out->rows = static_cast<int>(r[iqo_amd::kYRows]);
    out->workgroups = r[iqo_amd::kYGroups];
    out->ldsBytes = l.ldsBytes;
    out->nYp = static_cast<int>(tab(iqo_amd::kYYTab)[0]);
    out->np = static_cast<int>(tab(iqo_amd::kYXTab)[0]);
    out->pitchDw = static_cast<int>(r[iqo_amd::kYPitch]);
    out->nYpC = static_cast<int>(tab(iqo_amd::kYYTabC)[0]);
    out->npC = static_cast<int>(tab(iqo_amd::kYXTabC)[0]);
    out->pitchDwC = static_cast<int>(r[iqo_amd::kYPitchC]);
    return IQO_HIP_OK;
}

} // namespace

extern "C" {

int iqo_host_roi_yuv_box_layout(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t w, size_t h,
                                iqo_hip_roi_yuv_box_layout *out)
{
    return roi_yuv_box_layout(method, degree, layout, dstW, dstH, w, h, nullptr, out, nullptr);
}

int iqo_host_roi_yuv_fit_box_layout(int method, unsigned degree, int layout, size_t dstW, size_t dstH, size_t w, size_t h,
                                    const iqo_hip_roi_rect *rect, iqo_hip_roi_yuv_fit_box_layout *out)
{
    const RoiFit fit = {rect, nullptr};
    return roi_yuv_box_layout(method, degree, layout, dstW, dstH, w, h, &fit, out ? &out->box : nullptr, out);
}

} // extern "C"
