// kernels_color.hip -- gfx950 kernel for the second pass of the NV12 / I420 "resize to RGB" entries
// (include/iqo_hip.h iqo_hip_resize_nv12_rgb_device and its three siblings): resized Y and chroma
// planes in, packed RGB(A) bytes or normalised planar fp32 / fp16 / bf16 tensors out.
//
//   yuv_rgb_kernel<UV2, NORM, PX, C444>   UV2: interleaved UV plane (NV12) / separate U and V planes (I420)
//                                         NORM: planar floats (kernels.hpp NormDev) / packed bytes
//                                         PX: pixels per thread, 8 (4 for fp32 planes)
//                                         C444: chroma planes on the output grid (IQO_CHROMA_FULL) /
//                                               at half size, replicated 2 x 2 (IQO_CHROMA_REPLICATE)
//
// Memory-bound, no LDS.  A thread owns 8 adjacent output pixels of one row: one 8-byte load of Y,
// 4 chroma pairs (one 8-byte load of UV, or 4 bytes each of U and V), the integer matrix of
// colorspace.hpp in registers, then 16- or 8-byte stores where the destination address allows and
// single elements otherwise (the rule of packed_tile_kernel's epilogue: no alignment of the
// destination beyond its element size).  With fp32 planes a thread owns 4 pixels and loads half of
// that (see yuv_rgb_kernel).  Threads run over (frame, row, pixel group) in that order,
// so a wave's loads and stores are contiguous within a row and follow on into the next one.
// With C444 pixel (y, x) takes chroma sample (y, x): 8 chroma pairs per thread (one 16-byte load of
// UV, or 8 bytes each of U and V), the chroma terms once per pixel, and no index clamp or edge fetch.
//
// The opposite direction, rgb_yuv_kernel<C, UV2> (resized packed RGB(A) pixels in, a Y plane and 4:2:0
// chroma out: the second pass of iqo_hip_resize_rgb_nv12_device / _rgb_yuv420_device), is at the end of
// the file with its own description.
#include "kernels_dev.hpp"

namespace iqo_amd {
namespace {

struct YuvRgbBytesArgs {
    YuvRgbDev d;
    int nG;             // pixel groups (one per thread) per row
    unsigned items;     // frames x dstH x nG
    int C;              // 3 or 4 bytes per pixel
    // v_perm selectors over a pixel's word (R, G, B, 255).  C = 4: sel[0] gives the pixel's 4 bytes.
    // C = 3: 4 pixels are 3 words; word i takes its bytes from pixels i and i + 1 by sel[i].
    uint32_t sel[3];
};

struct YuvRgbNormArgs {
    YuvRgbDev d;
    int nG;
    unsigned items;
    NormDev n;
};

__device__ __forceinline__ uint32_t byte_of(uint32_t w, int i) { return (w >> (8 * i)) & 0xffu; }

// (sat_u8(r >> 14), sat_u8(g >> 14), sat_u8(b >> 14), 255) as the four bytes of a word: the shift and
// both clamps of colorspace.hpp's yuv_to_rgb in gfx950's v_ashr_pk_u8_i32 (kernels_dev.hpp).
__device__ __forceinline__ uint32_t rgb_word(int r, int g, int b)
{
    return ashr_pk_hi<kYuvRgbShift>(ashr_pk_lo<kYuvRgbShift>(r, g), b, 255 << kYuvRgbShift);
}

// The PX pixels [PX g, PX g + PX) of output row `row` of frame f, each a word (R, G, B, 255).
template <bool UV2, int PX, bool C444>
__device__ __forceinline__ void rgb_run(const YuvRgbDev &d, int f, int row, int g, uint32_t (&w)[PX])
{
    static_assert(PX == 8 || PX == 4, "a thread's run: 8 Y bytes and 4 chroma pairs, or half of that");
    constexpr int NC = PX / 2;  // chroma samples of the run at half size (C444: PX of them)
    const int64_t fo = static_cast<int64_t>(f) * d.frameSt;
    const uint8_t *yp = d.y + fo + static_cast<int64_t>(row) * d.ySt + PX * g;
    uint32_t yy[2] = {0u, 0u};
    if constexpr (PX == 8) {
        const u32x2 v2 = *reinterpret_cast<const u32x2 *>(yp);
        yy[0] = v2.x;
        yy[1] = v2.y;
    } else {
        yy[0] = *reinterpret_cast<const uint32_t *>(yp);
    }
    if constexpr (C444) {
        // chroma on the output grid: samples PX g .. PX g + PX - 1 of row `row`, one per byte of UU / VV
        const int64_t co = fo + static_cast<int64_t>(row) * d.cSt;
        uint32_t UU[2] = {0u, 0u}, VV[2] = {0u, 0u};
        if constexpr (UV2 && PX == 8) {
            const u32x4 uv = *reinterpret_cast<const u32x4 *>(d.u + co + 16 * g);
            UU[0] = __builtin_amdgcn_perm(uv.y, uv.x, 0x06040200u);
            VV[0] = __builtin_amdgcn_perm(uv.y, uv.x, 0x07050301u);
            UU[1] = __builtin_amdgcn_perm(uv.w, uv.z, 0x06040200u);
            VV[1] = __builtin_amdgcn_perm(uv.w, uv.z, 0x07050301u);
        } else if constexpr (UV2) {
            const u32x2 uv = *reinterpret_cast<const u32x2 *>(d.u + co + 8 * g);
            UU[0] = __builtin_amdgcn_perm(uv.y, uv.x, 0x06040200u);
            VV[0] = __builtin_amdgcn_perm(uv.y, uv.x, 0x07050301u);
        } else if constexpr (PX == 8) {
            const u32x2 u2 = *reinterpret_cast<const u32x2 *>(d.u + co + 8 * g);
            const u32x2 v2 = *reinterpret_cast<const u32x2 *>(d.v + co + 8 * g);
            UU[0] = u2.x;
            UU[1] = u2.y;
            VV[0] = v2.x;
            VV[1] = v2.y;
        } else {
            UU[0] = *reinterpret_cast<const uint32_t *>(d.u + co + 4 * g);
            VV[0] = *reinterpret_cast<const uint32_t *>(d.v + co + 4 * g);
        }
#pragma unroll
        for (int k = 0; k < PX; ++k) {
            const YuvChroma c = yuv_chroma_terms(d.k, static_cast<int>(byte_of(UU[k >> 2], k & 3)),
                                                 static_cast<int>(byte_of(VV[k >> 2], k & 3)));
            int r, gg, b;
            yuv_sums(d.k, static_cast<int>(byte_of(yy[k >> 2], k & 3)), c, r, gg, b);
            w[k] = rgb_word(r, gg, b);
        }
        return;
    }
    const int cr = min(row >> 1, d.ch - 1);
    const int64_t co = fo + static_cast<int64_t>(cr) * d.cSt;
    uint32_t U, V;  // chroma samples NC g .. NC g + NC - 1 of the row, one per byte
    if constexpr (UV2 && PX == 8) {
        const u32x2 uv = *reinterpret_cast<const u32x2 *>(d.u + co + 8 * g);
        U = __builtin_amdgcn_perm(uv.y, uv.x, 0x06040200u);
        V = __builtin_amdgcn_perm(uv.y, uv.x, 0x07050301u);
    } else if constexpr (UV2) {
        const uint32_t uv = *reinterpret_cast<const uint32_t *>(d.u + co + 4 * g);
        U = __builtin_amdgcn_perm(0u, uv, 0x0c0c0200u);
        V = __builtin_amdgcn_perm(0u, uv, 0x0c0c0301u);
    } else if constexpr (PX == 8) {
        U = *reinterpret_cast<const uint32_t *>(d.u + co + 4 * g);
        V = *reinterpret_cast<const uint32_t *>(d.v + co + 4 * g);
    } else {
        U = *reinterpret_cast<const uint16_t *>(d.u + co + 2 * g);
        V = *reinterpret_cast<const uint16_t *>(d.v + co + 2 * g);
    }
    // An odd dstW's last pixel x = 2 cw has no chroma sample of its own and takes sample cw - 1,
    // which byte x >> 1 = cw of the loads above does not hold: fetch it (one thread per row).
    const int j = d.cw - NC * g;  // sample cw sits in byte j
    if ((d.dstW & 1) && j >= 0 && j < NC) {
        const uint32_t ue = UV2 ? d.u[co + 2 * (d.cw - 1)] : d.u[co + d.cw - 1];
        const uint32_t ve = UV2 ? d.u[co + 2 * (d.cw - 1) + 1] : d.v[co + d.cw - 1];
        const uint32_t keep = ~(0xffu << (8 * j));
        U = (U & keep) | (ue << (8 * j));
        V = (V & keep) | (ve << (8 * j));
    }
#pragma unroll
    for (int q = 0; q < NC; ++q) {
        const YuvChroma c = yuv_chroma_terms(d.k, static_cast<int>(byte_of(U, q)), static_cast<int>(byte_of(V, q)));
#pragma unroll
        for (int e = 0; e < 2; ++e) {
            const int k = 2 * q + e;
            int r, gg, b;
            yuv_sums(d.k, static_cast<int>(byte_of(yy[k >> 2], k & 3)), c, r, gg, b);
            w[k] = rgb_word(r, gg, b);
        }
    }
}

// 8 C bytes (2 C words o[]) to p; `full`: all 8 pixels are inside the row, else the first `valid`
template <int C>
__device__ __forceinline__ void store_bytes(uint8_t *p, const uint32_t (&o)[2 * C], bool full, int valid)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    if (full && C == 4 && !(a & 15)) {
#pragma unroll
        for (int i = 0; i < 2; ++i)
            reinterpret_cast<u32x4 *>(p)[i] = u32x4{o[4 * i], o[4 * i + 1], o[4 * i + 2], o[4 * i + 3]};
    } else if (full && !(a & 7)) {
#pragma unroll
        for (int i = 0; i < C; ++i)
            reinterpret_cast<u32x2 *>(p)[i] = u32x2{o[2 * i], o[2 * i + 1]};
    } else {
#pragma unroll
        for (int b = 0; b < 8 * C; ++b)
            if (b / C < valid)
                p[b] = static_cast<uint8_t>(o[b >> 2] >> (8 * (b & 3)));
    }
}

// PX pixels per thread: 8 (bytes, fp16, bf16), and 4 for fp32 planes, PX = 4's only form.  With 8 a
// thread's fp32 run is 32 bytes, two 16-byte stores per plane with neighbouring lanes 32 bytes apart,
// so every store instruction fills half of each cache line it touches; with 4 pixels a wave's store
// is 1 KiB contiguous.
template <bool UV2, bool NORM, int PX, bool C444>
__global__ __launch_bounds__(256) void yuv_rgb_kernel(std::conditional_t<NORM, YuvRgbNormArgs, YuvRgbBytesArgs> a)
{
    static_assert(NORM || PX == 8, "the byte form owns 8 pixels per thread");
    const YuvRgbDev &d = a.d;
    const unsigned nG = static_cast<unsigned>(a.nG), H = static_cast<unsigned>(d.dstH);
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < a.items; it += gridDim.x * 256u) {
        const unsigned t = it / nG;
        const int g = static_cast<int>(it - t * nG), f = static_cast<int>(t / H), row = static_cast<int>(t - (t / H) * H);
        uint32_t w[PX];  // the pixels' (R, G, B, 255)
        rgb_run<UV2, PX, C444>(d, f, row, g, w);
        const int x0 = PX * g, valid = min(PX, d.dstW - x0);
        const bool full = valid == PX;
        uint8_t *rowp = d.dst + static_cast<int64_t>(f) * d.dstFrameSt + static_cast<int64_t>(row) * d.dstSt;
        if constexpr (NORM) {
            const NormDev &n = a.n;
#pragma unroll
            for (int p = 0; p < 4; ++p) {
                if (p >= n.planes)
                    break;
                const int sh = 8 * n.order[p];  // uniform: the plane's byte of the pixel words
                float v[PX];
#pragma unroll
                for (int k = 0; k < PX; ++k)
                    v[k] = norm_affine((w[k] >> sh) & 0xffu, n.scale[p], n.bias[p]);
                uint8_t *pp = rowp + static_cast<int64_t>(p) * n.planeSt;
                if constexpr (PX == 4) {  // fp32 (the launcher's choice of PX)
                    uint8_t *q = pp + 4 * x0;
                    const uintptr_t al = reinterpret_cast<uintptr_t>(q);
                    if (full && !(al & 15)) {
                        *reinterpret_cast<u32x4 *>(q) = u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]),
                                                             __float_as_uint(v[2]), __float_as_uint(v[3])};
                    } else if (full && !(al & 7)) {
#pragma unroll
                        for (int i = 0; i < 2; ++i)
                            reinterpret_cast<u32x2 *>(q)[i] = u32x2{__float_as_uint(v[2 * i]), __float_as_uint(v[2 * i + 1])};
                    } else {
#pragma unroll
                        for (int k = 0; k < 4; ++k)
                            if (k < valid)
                                reinterpret_cast<float *>(q)[k] = v[k];
                    }
                } else {  // fp16 / bf16
                    uint32_t h[8];
                    if (n.dtype == 2) {
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            h[k] = f16_bits(v[k]);
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            h[k] = bf16_bits(v[k]);
                    }
                    uint8_t *q = pp + 2 * x0;
                    const uintptr_t al = reinterpret_cast<uintptr_t>(q);
                    if (full && !(al & 15)) {
                        *reinterpret_cast<u32x4 *>(q) =
                            u32x4{h[0] | (h[1] << 16), h[2] | (h[3] << 16), h[4] | (h[5] << 16), h[6] | (h[7] << 16)};
                    } else if (full && !(al & 7)) {
#pragma unroll
                        for (int i = 0; i < 2; ++i)
                            reinterpret_cast<u32x2 *>(q)[i] =
                                u32x2{h[4 * i] | (h[4 * i + 1] << 16), h[4 * i + 2] | (h[4 * i + 3] << 16)};
                    } else {
#pragma unroll
                        for (int k = 0; k < 8; ++k)
                            if (k < valid)
                                reinterpret_cast<uint16_t *>(q)[k] = static_cast<uint16_t>(h[k]);
                    }
                }
            }
        } else {
            // the bytes are placed by v_perm with uniform selectors
            if (a.C == 4) {
                uint32_t o[8];
#pragma unroll
                for (int k = 0; k < 8; ++k)
                    o[k] = __builtin_amdgcn_perm(0u, w[k], a.sel[0]);
                store_bytes<4>(rowp + 4 * x0, o, full, valid);
            } else {
                uint32_t o[6];
#pragma unroll
                for (int q = 0; q < 2; ++q)
#pragma unroll
                    for (int i = 0; i < 3; ++i)
                        o[3 * q + i] = __builtin_amdgcn_perm(w[4 * q + i + 1], w[4 * q + i], a.sel[i]);
                store_bytes<3>(rowp + 3 * x0, o, full, valid);
            }
        }
    }
}

// Grid: 256-thread blocks over the items, capped at kernels.hpp kGridStrideBlocks (8 blocks per CU of a
// 256-CU device); the kernel strides over the rest.

// c444: the chroma planes are on the output grid (cw x ch = dstW x dstH) and a thread loads as many
// chroma samples per component as pixels -- 16 bytes of UV, or 8 each of U and V, for 8 pixels.
bool dev_ok(const YuvRgbDev &d, bool uv2, bool c444)
{
    if (d.dstW < 2 || d.dstH < 2 || d.cw != (c444 ? d.dstW : d.dstW / 2) || d.ch != (c444 ? d.dstH : d.dstH / 2) ||
        d.frames < 0 || !d.y || !d.u || (!uv2 && !d.v) || !d.dst || d.dstSt < 0)
        return false;
    const int nG = (d.dstW + 7) / 8;
    const uintptr_t ca = c444 ? (uv2 ? 15 : 7) : (uv2 ? 7 : 3);  // a thread's widest chroma load
    const uintptr_t fa = c444 && uv2 ? 15 : 7;
    if (d.ySt < 8 * nG || d.cSt < static_cast<int>(ca + 1) * nG || (d.ySt & 7) || (static_cast<uintptr_t>(d.cSt) & ca) ||
        (static_cast<uintptr_t>(d.frameSt) & fa) || (reinterpret_cast<uintptr_t>(d.y) & 7) ||
        (reinterpret_cast<uintptr_t>(d.u) & ca) || (!uv2 && (reinterpret_cast<uintptr_t>(d.v) & ca)))
        return false;
    // (counted in 4-pixel groups, the finer of the two runs a thread can own)
    return static_cast<uint64_t>(d.frames) * static_cast<uint64_t>(d.dstH) * static_cast<uint64_t>((d.dstW + 3) / 4) < (uint64_t(1) << 31);
}

// the instantiation of a launch
template <bool NORM, int PX>
const void *kernel_of(bool uv2, bool c444)
{
    if (c444)
        return uv2 ? reinterpret_cast<const void *>(yuv_rgb_kernel<true, NORM, PX, true>)
                   : reinterpret_cast<const void *>(yuv_rgb_kernel<false, NORM, PX, true>);
    return uv2 ? reinterpret_cast<const void *>(yuv_rgb_kernel<true, NORM, PX, false>)
               : reinterpret_cast<const void *>(yuv_rgb_kernel<false, NORM, PX, false>);
}

} // namespace

hipError_t launch_yuv_rgb_bytes(const YuvRgbDev &d, bool interleavedUV, bool chroma444, int channels,
                                const int (&order)[4], hipStream_t s)
{
    if (!dev_ok(d, interleavedUV, chroma444) || channels < 3 || channels > 4)
        return hipErrorInvalidValue;
    for (int c = 0; c < channels; ++c)
        if (order[c] < 0 || order[c] > 3)
            return hipErrorInvalidValue;
    if (d.frames == 0)
        return hipSuccess;
    YuvRgbBytesArgs a{};
    a.d = d;
    a.nG = (d.dstW + 7) / 8;
    a.items = static_cast<unsigned>(d.frames) * static_cast<unsigned>(d.dstH) * static_cast<unsigned>(a.nG);
    a.C = channels;
    const uint32_t o0 = static_cast<uint32_t>(order[0]), o1 = static_cast<uint32_t>(order[1]),
                   o2 = static_cast<uint32_t>(order[2]);
    if (channels == 4) {
        a.sel[0] = o0 | (o1 << 8) | (o2 << 16) | (static_cast<uint32_t>(order[3]) << 24);
    } else {
        // v_perm(hi = pixel i + 1, lo = pixel i): selector bytes 0 .. 3 pick from lo, 4 .. 7 from hi
        a.sel[0] = o0 | (o1 << 8) | (o2 << 16) | ((o0 + 4) << 24);
        a.sel[1] = o1 | (o2 << 8) | ((o0 + 4) << 16) | ((o1 + 4) << 24);
        a.sel[2] = o2 | ((o0 + 4) << 8) | ((o1 + 4) << 16) | ((o2 + 4) << 24);
    }
    const unsigned blocks = std::min((a.items + 255u) / 256u, kGridStrideBlocks);
    const void *kern = kernel_of<false, 8>(interleavedUV, chroma444);
    void *args[] = {&a};
    return hipLaunchKernel(kern, dim3(blocks), dim3(256), args, 0, s);
}

hipError_t launch_yuv_rgb_norm(const YuvRgbDev &d, bool interleavedUV, bool chroma444, const NormDev &n, hipStream_t s)
{
    if (!dev_ok(d, interleavedUV, chroma444) || n.dtype < 1 || n.dtype > 3 || n.planes < 1 || n.planes > 4 || n.planeSt < 0)
        return hipErrorInvalidValue;
    for (int p = 0; p < n.planes; ++p)
        if (n.order[p] < 0 || n.order[p] > 2)
            return hipErrorInvalidValue;
    if (d.frames == 0)
        return hipSuccess;
    YuvRgbNormArgs a{};
    a.d = d;
    const int px = n.dtype == 1 ? 4 : 8;  // fp32: 4 pixels per thread (yuv_rgb_kernel)
    a.nG = (d.dstW + px - 1) / px;
    a.items = static_cast<unsigned>(d.frames) * static_cast<unsigned>(d.dstH) * static_cast<unsigned>(a.nG);
    a.n = n;
    const unsigned blocks = std::min((a.items + 255u) / 256u, kGridStrideBlocks);
    const void *kern = px == 4 ? kernel_of<true, 4>(interleavedUV, chroma444) : kernel_of<true, 8>(interleavedUV, chroma444);
    void *args[] = {&a};
    return hipLaunchKernel(kern, dim3(blocks), dim3(256), args, 0, s);
}

// ---- rgb_yuv_kernel<C, UV2>: the second pass of the "resize to NV12 / I420" entries
// (include/iqo_hip.h iqo_hip_resize_rgb_nv12_device / _rgb_yuv420_device): resized packed pixels in, a Y
// plane and 4:2:0 chroma out.  C: 3 or 4 bytes per pixel; UV2: one interleaved UV plane (NV12) / separate
// U and V planes (I420).
//
// Memory-bound, no LDS.  A thread owns 8 adjacent pixels of a ROW PAIR (rows 2 p and 2 p + 1): whole
// loads of its 8 C bytes of both rows (two 16-byte loads per row at C = 4, 16 + 8 bytes at C = 3), the
// forward matrix of colorspace.hpp in registers, 8 Y bytes per row, and 4 chroma samples from the sums of
// its four 2 x 2 blocks: one 8-byte UV store, or 4 bytes each of U and V.  Stores follow store_bytes'
// rule: the widest the address allows, single bytes in a row's partial last group or at a misaligned
// destination.  Threads run over (frame, row pair, pixel group) in that order.
// An odd dstH's last row has no partner: it is a pair of its own whose second row is neither loaded nor
// given chroma.  An odd dstW's last column lies past the last whole 2 x 2 block and gives Y only.  The
// workspace's pad pixels past dstW are read (whatever they hold) and never stored: chroma sample i takes
// columns 2 i and 2 i + 1 <= 2 cw - 1 < dstW.
namespace {

struct RgbYuvArgs {
    RgbYuvDev d;
    int nG, nP;         // pixel groups (one per thread) per row, row pairs per frame
    unsigned items;     // frames x nP x nG
    // Where R, G, B sit in a pixel, built from d.order by the launcher.
    // C = 4: a pixel is a word, sel[c] = 8 order[c] is the bit offset of R, G, B in it.
    // C = 3: 4 pixels are 3 words; pixel j's (R, G, B, 0) is v_perm(word min(j, 2), word max(j, 1) - 1, sel[j]).
    uint32_t sel[4];
};

typedef u32x4 u32x4_a8 __attribute__((aligned(8)));  // C = 3: a thread's 24 bytes start at a multiple of 8

// The 8 pixels a thread owns of one workspace row, p at the first of them
template <int C>
__device__ __forceinline__ void rgb_load(const uint8_t *p, const uint32_t (&sel)[4], int (&R)[8], int (&G)[8], int (&B)[8])
{
    if constexpr (C == 4) {
        const u32x4 a = reinterpret_cast<const u32x4 *>(p)[0], b = reinterpret_cast<const u32x4 *>(p)[1];
        const uint32_t w[8] = {a.x, a.y, a.z, a.w, b.x, b.y, b.z, b.w};
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            R[k] = static_cast<int>((w[k] >> sel[0]) & 0xffu);
            G[k] = static_cast<int>((w[k] >> sel[1]) & 0xffu);
            B[k] = static_cast<int>((w[k] >> sel[2]) & 0xffu);
        }
    } else {
        const u32x4_a8 a = *reinterpret_cast<const u32x4_a8 *>(p);
        const u32x2 b = *reinterpret_cast<const u32x2 *>(p + 16);
        const uint32_t w[6] = {a.x, a.y, a.z, a.w, b.x, b.y};
#pragma unroll
        for (int q = 0; q < 2; ++q)
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const uint32_t px = __builtin_amdgcn_perm(w[3 * q + (j < 2 ? j : 2)], w[3 * q + (j > 1 ? j - 1 : 0)], sel[j]);
                R[4 * q + j] = static_cast<int>(byte_of(px, 0));
                G[4 * q + j] = static_cast<int>(byte_of(px, 1));
                B[4 * q + j] = static_cast<int>(byte_of(px, 2));
            }
    }
}

// (v[0] >> S, ..., v[3] >> S) as the bytes of a word, each saturated to 255 (v_ashr_pk_u8_i32; the
// accumulators of colorspace.hpp's forward matrix are never negative)
template <int S>
__device__ __forceinline__ uint32_t pack4(int a, int b, int c, int e)
{
    return ashr_pk_hi<S>(ashr_pk_lo<S>(a, b), c, e);
}

// NB = 8 or 4 bytes (the words o[]) to p, of which the first `valid` are inside the row
template <int NB>
__device__ __forceinline__ void store_run(uint8_t *p, const uint32_t (&o)[NB / 4], int valid)
{
    const uintptr_t a = reinterpret_cast<uintptr_t>(p);
    const bool full = valid == NB;
    if (NB == 8 && full && !(a & 7)) {
        *reinterpret_cast<u32x2 *>(p) = u32x2{o[0], o[NB / 4 - 1]};
    } else if (full && !(a & 3)) {
#pragma unroll
        for (int i = 0; i < NB / 4; ++i)
            reinterpret_cast<uint32_t *>(p)[i] = o[i];
    } else {
#pragma unroll
        for (int b = 0; b < NB; ++b)
            if (b < valid)
                p[b] = static_cast<uint8_t>(o[b >> 2] >> (8 * (b & 3)));
    }
}

__device__ __forceinline__ void store_y(uint8_t *p, const RgbYuvCoef &k, const int (&R)[8], const int (&G)[8],
                                        const int (&B)[8], int valid)
{
    int y[8];
#pragma unroll
    for (int i = 0; i < 8; ++i)
        y[i] = rgb_y_sum(k, R[i], G[i], B[i]);
    const uint32_t o[2] = {pack4<kRgbYuvShift>(y[0], y[1], y[2], y[3]), pack4<kRgbYuvShift>(y[4], y[5], y[6], y[7])};
    store_run<8>(p, o, valid);
}

template <int C, bool UV2>
__global__ __launch_bounds__(256) void rgb_yuv_kernel(RgbYuvArgs a)
{
    const RgbYuvDev &d = a.d;
    const unsigned nG = static_cast<unsigned>(a.nG), nP = static_cast<unsigned>(a.nP);
    const int cw = d.dstW >> 1;
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < a.items; it += gridDim.x * 256u) {
        const unsigned t = it / nG;
        const int g = static_cast<int>(it - t * nG), f = static_cast<int>(t / nP), rp = static_cast<int>(t - (t / nP) * nP);
        const int row = 2 * rp, valid = min(8, d.dstW - 8 * g);
        const uint8_t *sp = d.src + static_cast<int64_t>(f) * d.srcFrameSt + static_cast<int64_t>(row) * d.srcSt + 8 * C * g;
        const int64_t fo = static_cast<int64_t>(f) * d.dstFrameSt;
        uint8_t *yp = d.y + fo + static_cast<int64_t>(row) * d.ySt + 8 * g;
        int R[8], G[8], B[8];
        rgb_load<C>(sp, a.sel, R, G, B);
        store_y(yp, d.k, R, G, B, valid);
        if (row + 1 >= d.dstH)
            continue;  // an odd dstH's last row: no second row, no chroma
        int R1[8], G1[8], B1[8];
        rgb_load<C>(sp + d.srcSt, a.sel, R1, G1, B1);
        store_y(yp + d.ySt, d.k, R1, G1, B1, valid);
        const int nc = min(4, cw - 4 * g);  // chroma samples of the run inside the plane
        if (nc <= 0)
            continue;
        int u[4], v[4];
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int sr = R[2 * q] + R[2 * q + 1] + R1[2 * q] + R1[2 * q + 1];
            const int sg = G[2 * q] + G[2 * q + 1] + G1[2 * q] + G1[2 * q + 1];
            const int sb = B[2 * q] + B[2 * q + 1] + B1[2 * q] + B1[2 * q + 1];
            u[q] = rgb_u_sum<kRgbYuvSumShift>(d.k, sr, sg, sb);
            v[q] = rgb_v_sum<kRgbYuvSumShift>(d.k, sr, sg, sb);
        }
        const int64_t co = fo + static_cast<int64_t>(rp) * d.cSt;
        if constexpr (UV2) {
            const uint32_t o[2] = {pack4<kRgbYuvSumShift>(u[0], v[0], u[1], v[1]),
                                   pack4<kRgbYuvSumShift>(u[2], v[2], u[3], v[3])};
            store_run<8>(d.u + co + 8 * g, o, 2 * nc);
        } else {
            const uint32_t ou[1] = {pack4<kRgbYuvSumShift>(u[0], u[1], u[2], u[3])};
            const uint32_t ov[1] = {pack4<kRgbYuvSumShift>(v[0], v[1], v[2], v[3])};
            store_run<4>(d.u + co + 4 * g, ou, nc);
            store_run<4>(d.v + co + 4 * g, ov, nc);
        }
    }
}

} // namespace

hipError_t launch_rgb_yuv(const RgbYuvDev &d, int channels, bool interleavedUV, hipStream_t s)
{
    if (channels < 3 || channels > 4 || d.dstW < 2 || d.dstH < 2 || d.frames < 0 || !d.src || !d.y || !d.u ||
        (!interleavedUV && !d.v))
        return hipErrorInvalidValue;
    for (int c = 0; c < 3; ++c)
        if (d.order[c] < 0 || d.order[c] >= channels || d.order[c] == d.order[(c + 1) % 3])
            return hipErrorInvalidValue;
    const int nG = (d.dstW + 7) / 8, nP = (d.dstH + 1) / 2, cw = d.dstW / 2;
    if (d.srcSt < 8 * channels * nG || (d.srcSt & 15) || (d.srcFrameSt & 15) || (reinterpret_cast<uintptr_t>(d.src) & 15) ||
        d.ySt < d.dstW || d.cSt < (interleavedUV ? 2 : 1) * cw)
        return hipErrorInvalidValue;
    if (static_cast<uint64_t>(d.frames) * static_cast<uint64_t>(nP) * static_cast<uint64_t>(nG) >= (uint64_t(1) << 31))
        return hipErrorInvalidValue;
    if (d.frames == 0)
        return hipSuccess;
    RgbYuvArgs a{};
    a.d = d;
    a.nG = nG;
    a.nP = nP;
    a.items = static_cast<unsigned>(d.frames) * static_cast<unsigned>(nP) * static_cast<unsigned>(nG);
    if (channels == 4) {
        for (int c = 0; c < 3; ++c)
            a.sel[c] = 8u * static_cast<uint32_t>(d.order[c]);
    } else {
        // pixel j of 4 starts at byte 3 j of the 3 words: byte `off` of the pair (lo, hi) v_perm selects from
        // (selector bytes 0 .. 3 pick from lo, 4 .. 7 from hi, 0x0c is the constant 0)
        const uint32_t off[4] = {0, 3, 2, 1};
        for (int j = 0; j < 4; ++j)
            a.sel[j] = (off[j] + static_cast<uint32_t>(d.order[0])) | ((off[j] + static_cast<uint32_t>(d.order[1])) << 8) |
                       ((off[j] + static_cast<uint32_t>(d.order[2])) << 16) | (0x0cu << 24);
    }
    const unsigned blocks = std::min((a.items + 255u) / 256u, kGridStrideBlocks);
    const void *kern = channels == 4 ? (interleavedUV ? reinterpret_cast<const void *>(rgb_yuv_kernel<4, true>)
                                                      : reinterpret_cast<const void *>(rgb_yuv_kernel<4, false>))
                                     : (interleavedUV ? reinterpret_cast<const void *>(rgb_yuv_kernel<3, true>)
                                                      : reinterpret_cast<const void *>(rgb_yuv_kernel<3, false>));
    void *args[] = {&a};
    return hipLaunchKernel(kern, dim3(blocks), dim3(256), args, 0, s);
}

} // namespace iqo_amd
