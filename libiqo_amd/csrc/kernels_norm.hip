// kernels_norm.hip -- gfx950 kernel for the second pass of iqo_hip_resize_planes_norm_device
// (include/iqo_hip.h): resized U8 planes in, normalised planar fp32 / fp16 / bf16 tensors out.
//
//   planes_norm_kernel<PX>   PX: pixels per thread, 8 (fp16, bf16) or 4 (fp32)
//
// Memory-bound, no LDS: yuv_rgb_kernel's NORM form (kernels_color.hip) without the matrix.  A thread
// owns PX adjacent output pixels of one row.  For each output plane p it loads its PX bytes of
// workspace plane order[p] in one aligned load (kept from plane p - 1 when order repeats), applies
// norm_affine -- two separately rounded fp32 operations -- and the dtype's conversion, and stores 16
// bytes where the destination address allows, 8 otherwise, and single elements in a row's partial last
// group or at a misaligned destination (the rule of packed_tile_kernel's epilogue: no alignment of the
// destination beyond its element size).  fp32 takes 4 pixels for the reason given at yuv_rgb_kernel:
// with 8 every store instruction fills half of each cache line it touches.  Threads run over
// (frame, row, pixel group) in that order, so a wave's loads and stores are contiguous within a row
// and follow on into the next one.  scale, bias, order and dtype are kernel arguments: the plane loop
// is unrolled and nothing is indexed at run time.
#include "kernels_dev.hpp"

namespace iqo_amd {
namespace {

struct PlanesNormArgs {
    PlanesNormDev d;
    int nG;             // pixel groups (one per thread) per row
    unsigned items;     // frames x dstH x nG
    NormDev n;
};

template <int PX>
__global__ __launch_bounds__(256) void planes_norm_kernel(PlanesNormArgs a)
{
    static_assert(PX == 8 || PX == 4, "a thread's run: one 8- or 4-byte load per plane");
    const PlanesNormDev &d = a.d;
    const NormDev &n = a.n;
    const unsigned nG = static_cast<unsigned>(a.nG), H = static_cast<unsigned>(d.dstH);
    for (unsigned it = blockIdx.x * 256u + threadIdx.x; it < a.items; it += gridDim.x * 256u) {
        const unsigned t = it / nG;
        const int g = static_cast<int>(it - t * nG), f = static_cast<int>(t / H), row = static_cast<int>(t - (t / H) * H);
        const int x0 = PX * g, valid = min(PX, d.dstW - x0);
        const bool full = valid == PX;
        const uint8_t *sp = d.src + static_cast<int64_t>(f) * d.srcFrameSt + static_cast<int64_t>(row) * d.srcSt + x0;
        uint8_t *rowp = d.dst + static_cast<int64_t>(f) * d.dstFrameSt + static_cast<int64_t>(row) * d.dstSt;
        uint32_t w[2] = {0u, 0u};  // the run's bytes of the current workspace plane
#pragma unroll
        for (int p = 0; p < 4; ++p) {
            if (p >= n.planes)
                break;
            if (p == 0 || n.order[p] != n.order[p - 1]) {  // uniform
                const uint8_t *q = sp + static_cast<int64_t>(n.order[p]) * d.srcPlaneSt;
                if constexpr (PX == 8) {
                    const u32x2 v2 = *reinterpret_cast<const u32x2 *>(q);
                    w[0] = v2.x;
                    w[1] = v2.y;
                } else {
                    w[0] = *reinterpret_cast<const uint32_t *>(q);
                }
            }
            float v[PX];
#pragma unroll
            for (int k = 0; k < PX; ++k)
                v[k] = norm_affine((w[k >> 2] >> (8 * (k & 3))) & 0xffu, n.scale[p], n.bias[p]);
            uint8_t *pp = rowp + static_cast<int64_t>(p) * n.planeSt;
            if constexpr (PX == 4) {  // fp32 (the launcher's choice of PX)
                uint8_t *q = pp + 4 * x0;
                const uintptr_t al = reinterpret_cast<uintptr_t>(q);
                if (full && !(al & 15)) {
                    *reinterpret_cast<u32x4 *>(q) =
                        u32x4{__float_as_uint(v[0]), __float_as_uint(v[1]), __float_as_uint(v[2]), __float_as_uint(v[3])};
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
    }
}

// Grid: 256-thread blocks over the items, capped at kernels.hpp kGridStrideBlocks (8 blocks per CU of a
// 256-CU device); the kernel strides over the rest.

// a thread loads 8 bytes whole at a multiple of 8 from the plane's row start (fp32: 4 at a multiple of 4)
bool dev_ok(const PlanesNormDev &d)
{
    if (d.dstW < 1 || d.dstH < 1 || d.frames < 0 || !d.src || !d.dst || d.dstSt < 0)
        return false;
    const int nG = (d.dstW + 7) / 8;
    if (d.srcSt < 8 * nG || (d.srcSt & 7) || d.srcPlaneSt < 0 || (d.srcPlaneSt & 7) || d.srcFrameSt < 0 ||
        (d.srcFrameSt & 7) || (reinterpret_cast<uintptr_t>(d.src) & 7))
        return false;
    // (counted in 4-pixel groups, the finer of the two runs a thread can own)
    return static_cast<uint64_t>(d.frames) * static_cast<uint64_t>(d.dstH) * static_cast<uint64_t>((d.dstW + 3) / 4) < (uint64_t(1) << 31);
}

} // namespace

hipError_t launch_planes_norm(const PlanesNormDev &d, const NormDev &n, hipStream_t s)
{
    if (!dev_ok(d) || n.dtype < 1 || n.dtype > 3 || n.planes < 1 || n.planes > 4 || n.planeSt < 0)
        return hipErrorInvalidValue;
    for (int p = 0; p < n.planes; ++p)
        if (n.order[p] < 0 || n.order[p] > 3)
            return hipErrorInvalidValue;
    if (d.frames == 0)
        return hipSuccess;
    PlanesNormArgs a{};
    a.d = d;
    const int px = n.dtype == 1 ? 4 : 8;  // fp32: 4 pixels per thread (planes_norm_kernel)
    a.nG = (d.dstW + px - 1) / px;
    a.items = static_cast<unsigned>(d.frames) * static_cast<unsigned>(d.dstH) * static_cast<unsigned>(a.nG);
    a.n = n;
    const unsigned blocks = std::min((a.items + 255u) / 256u, kGridStrideBlocks);
    const void *kern = px == 4 ? reinterpret_cast<const void *>(planes_norm_kernel<4>)
                               : reinterpret_cast<const void *>(planes_norm_kernel<8>);
    void *args[] = {&a};
    return hipLaunchKernel(kern, dim3(blocks), dim3(256), args, 0, s);
}

} // namespace iqo_amd
