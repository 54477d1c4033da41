// colorspace.hpp -- the one integer YUV -> RGB definition of the library, and the one RGB -> YUV
// definition (further down), both of include/iqo_hip.h's IQO_CS_* standards, included by the host code
// (abi.hip: iqo_host_yuv_to_rgb, iqo_host_rgb_to_yuv, iqo_host_rgb_to_yuv420) and the device code
// (kernels_color.hip).
//
// With S = 14, y' = Y - yOff, u = U - 128, v = V - 128 in int32 and >> an arithmetic shift:
//
//   R = clamp255((cY y' + cRV v         + 8192) >> 14)
//   G = clamp255((cY y' - cGU u - cGV v + 8192) >> 14)
//   B = clamp255((cY y' + cBU u         + 8192) >> 14)
//
// The constants are round(k 2^14) of the standards' real coefficients (Kr / Kb = 0.299 / 0.114 for
// BT.601, 0.2126 / 0.0722 for BT.709; limited range scales luma by 255/219 and chroma by 255/224).
// Over all 2^24 (Y, U, V) the largest |accumulator| is 8,954,873: int32 has ample room.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define IQO_HD __host__ __device__
#else
#define IQO_HD
#endif
// a product of two values that fit 24 signed bits (v_mad_i32_i24 with the sum around it on the device)
#if defined(__HIP_DEVICE_COMPILE__)
#define IQO_MUL24(a, b) __mul24((a), (b))
#else
#define IQO_MUL24(a, b) ((a) * (b))
#endif

namespace iqo_amd {

struct YuvRgbCoef {
    int yOff, cY, cRV, cGU, cGV, cBU;
};

constexpr int kYuvRgbStandards = 4;
constexpr int kYuvRgbShift = 14;

// rows: IQO_CS_BT601_LIMITED, IQO_CS_BT601_FULL, IQO_CS_BT709_LIMITED, IQO_CS_BT709_FULL
constexpr YuvRgbCoef kYuvRgb[kYuvRgbStandards] = {
    {16, 19077, 26149, 6419, 13320, 33050},
    {0, 16384, 22970, 5638, 11700, 29032},
    {16, 19077, 29372, 3494, 8731, 34610},
    {0, 16384, 25802, 3069, 7670, 30402},
};

IQO_HD inline int yuv_clamp255(int v) { return v < 0 ? 0 : (v > 255 ? 255 : v); }

// The chroma terms of a pixel's sums, shared by the pixels of one chroma sample.
struct YuvChroma {
    int r, g, b;  // cRV v, -cGU u - cGV v, cBU u
};

IQO_HD inline YuvChroma yuv_chroma_terms(const YuvRgbCoef &k, int U, int V)
{
    const int u = U - 128, v = V - 128;
    return YuvChroma{k.cRV * v, -k.cGU * u - k.cGV * v, k.cBU * u};
}

// The three sums of one pixel before the shift, rounding term included.
IQO_HD inline void yuv_sums(const YuvRgbCoef &k, int Y, const YuvChroma &c, int &r, int &g, int &b)
{
    const int l = k.cY * (Y - k.yOff) + (1 << (kYuvRgbShift - 1));
    r = l + c.r;
    g = l + c.g;
    b = l + c.b;
}

IQO_HD inline void yuv_to_rgb(const YuvRgbCoef &k, int Y, const YuvChroma &c, int &R, int &G, int &B)
{
    int r, g, b;
    yuv_sums(k, Y, c, r, g, b);
    R = yuv_clamp255(r >> kYuvRgbShift);
    G = yuv_clamp255(g >> kYuvRgbShift);
    B = yuv_clamp255(b >> kYuvRgbShift);
}

// ---- RGB -> YUV, the forward matrix of the same standards (the "resize to NV12 / I420" entries).
//
// All int32, >> a shift of a non-negative value.  A pixel (R, G, B):
//
//   Y = (cYR R + cYG G + cYB B + (yOff << 14) + 8192) >> 14
//   U = min(255, (cUB B - cUR R - cUG G + (128 << 14) + 8192) >> 14)
//   V = min(255, (cVR R - cVG G - cVB B + (128 << 14) + 8192) >> 14)
//
// A 4:2:0 chroma sample takes the sums SR, SG, SB over its 2 x 2 pixels and is rounded once:
//
//   U = min(255, (cUB SB - cUR SR - cUG SG + (128 << 16) + 32768) >> 16)      (V likewise)
//
// The constants are round(k 2^14) of the real coefficients: Kr, Kg, Kb for Y; Kr / (2 (1 - Kb)),
// Kg / (2 (1 - Kb)), 1/2 for U; 1/2, Kg / (2 (1 - Kr)), Kb / (2 (1 - Kr)) for V; limited range scales luma
// by 219/255 and chroma by 224/255.  Rounded one by one they keep cUR + cUG = cUB, cVG + cVB = cVR and
// cYR + cYG + cYB = round(sy 2^14), so grey gives U = V = 128 and the accumulators are never negative
// (the smallest is 8192; the largest is 2^22 per pixel and 2^24 per 2 x 2 sum): no lower clamp, no clamp
// of Y, and the min is live in the full-range standards only (pure blue, pure red: 256).
struct RgbYuvCoef {
    int yOff, cYR, cYG, cYB, cUR, cUG, cUB, cVR, cVG, cVB;
};

constexpr int kRgbYuvShift = 14;      // one pixel
constexpr int kRgbYuvSumShift = 16;   // the sum of a 2 x 2 block

// rows: IQO_CS_BT601_LIMITED, IQO_CS_BT601_FULL, IQO_CS_BT709_LIMITED, IQO_CS_BT709_FULL
constexpr RgbYuvCoef kRgbYuv[kYuvRgbStandards] = {
    {16, 4207, 8260, 1604, 2428, 4768, 7196, 7196, 6026, 1170},
    {0, 4899, 9617, 1868, 2765, 5427, 8192, 8192, 6860, 1332},
    {16, 2991, 10064, 1016, 1649, 5547, 7196, 7196, 6536, 660},
    {0, 3483, 11718, 1183, 1877, 6315, 8192, 8192, 7441, 751},
};

// The accumulators before the shift, rounding term included.  Y: shift kRgbYuvShift.
IQO_HD inline int rgb_y_sum(const RgbYuvCoef &k, int R, int G, int B)
{
    return IQO_MUL24(k.cYR, R) + IQO_MUL24(k.cYG, G) + IQO_MUL24(k.cYB, B) + (k.yOff << kRgbYuvShift) +
           (1 << (kRgbYuvShift - 1));
}

// U and V of (R, G, B) one pixel (S = kRgbYuvShift) or the sums of four (S = kRgbYuvSumShift)
template <int S>
IQO_HD inline int rgb_u_sum(const RgbYuvCoef &k, int R, int G, int B)
{
    return IQO_MUL24(k.cUB, B) + IQO_MUL24(-k.cUR, R) + IQO_MUL24(-k.cUG, G) + (128 << S) + (1 << (S - 1));
}
template <int S>
IQO_HD inline int rgb_v_sum(const RgbYuvCoef &k, int R, int G, int B)
{
    return IQO_MUL24(k.cVR, R) + IQO_MUL24(-k.cVG, G) + IQO_MUL24(-k.cVB, B) + (128 << S) + (1 << (S - 1));
}

IQO_HD inline int rgb_yuv_min255(int v) { return v > 255 ? 255 : v; }

} // namespace iqo_amd
