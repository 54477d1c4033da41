// colorspace.hpp -- the one integer YUV -> RGB definition of the library (include/iqo_hip.h,
// IQO_CS_*), included by the host code (abi.hip: iqo_host_yuv_to_rgb) and the device code
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

} // namespace iqo_amd
