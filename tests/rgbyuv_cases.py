"""The expected value and the shapes of the packed RGB(A) "resize to NV12 / I420" tests
(tests/test_rgbyuv_host.py, tests/test_rgbyuv_gpu.py).  Test infrastructure only.

The definition (include/iqo_hip.h, "Packed RGB(A) straight to NV12 / I420") is written once here, in numpy
int32, independently of the library's table.  A pixel (R, G, B):

    Y = (cYR R + cYG G + cYB B + (yOff << 14) + 8192) >> 14
    U = min(255, (cUB B - cUR R - cUG G + (128 << 14) + 8192) >> 14)        (4:4:4)
    V = min(255, (cVR R - cVG G - cVB B + (128 << 14) + 8192) >> 14)

and chroma sample (j, i) of the 4:2:0 planes, on the sums SR, SG, SB of rows 2j, 2j+1 x columns 2i, 2i+1:

    U = min(255, (cUB SB - cUR SR - cUG SG + (128 << 16) + 32768) >> 16)    (V likewise)

The expected value of a GPU case is the 4:2:0 form applied to packed_cases.oracle_packed of the source
frames: the reference's per-channel Generic resize stays the parity base.
"""
import functools

import numpy as np

import packed_cases as pc

SHIFT, SUM_SHIFT = 14, 16
BT601_LIMITED, BT601_FULL, BT709_LIMITED, BT709_FULL = 0, 1, 2, 3
# IQO_CS_*: (yOff, cYR, cYG, cYB, cUR, cUG, cUB, cVR, cVG, cVB)
TABLE = {
    BT601_LIMITED: (16, 4207, 8260, 1604, 2428, 4768, 7196, 7196, 6026, 1170),
    BT601_FULL: (0, 4899, 9617, 1868, 2765, 5427, 8192, 8192, 6860, 1332),
    BT709_LIMITED: (16, 2991, 10064, 1016, 1649, 5547, 7196, 7196, 6536, 660),
    BT709_FULL: (0, 3483, 11718, 1183, 1877, 6315, 8192, 8192, 7441, 751),
}
STANDARDS = sorted(TABLE)
FULL_RANGE = (BT601_FULL, BT709_FULL)
NAMES = {BT601_LIMITED: "bt601", BT601_FULL: "bt601-full", BT709_LIMITED: "bt709", BT709_FULL: "bt709-full"}
# the real coefficients the table rounds: (Kr, Kb, limited range)
REAL = {BT601_LIMITED: (0.299, 0.114, True), BT601_FULL: (0.299, 0.114, False),
        BT709_LIMITED: (0.2126, 0.0722, True), BT709_FULL: (0.2126, 0.0722, False)}
# where R, G, B sit in a source pixel
ORDERS = {"rgb": (0, 1, 2), "bgr": (2, 1, 0)}


def real_constants(standard):
    """(yOff, round(k 2^14) of the nine coefficients) from the standard's Kr / Kb and range scales."""
    kr, kb, limited = REAL[standard]
    kg = 1.0 - kr - kb
    sy, sc = (219.0 / 255.0, 224.0 / 255.0) if limited else (1.0, 1.0)
    ks = (kr * sy, kg * sy, kb * sy,
          kr / (2.0 * (1.0 - kb)) * sc, kg / (2.0 * (1.0 - kb)) * sc, 0.5 * sc,
          0.5 * sc, kg / (2.0 * (1.0 - kr)) * sc, kb / (2.0 * (1.0 - kr)) * sc)
    return (16 if limited else 0,) + tuple(int(round(k * (1 << SHIFT))) for k in ks)


def luma_scale(standard):
    """round(sy 2^14): what cYR + cYG + cYB must be."""
    return int(round((219.0 / 255.0 if REAL[standard][2] else 1.0) * (1 << SHIFT)))


def accumulators(standard, r, g, b, shift):
    """The three sums before the shift (int32 arrays, rounding term included) of int arrays r, g, b: one
    pixel's bytes with shift = SHIFT, the sums of four with shift = SUM_SHIFT (Y is per pixel: SHIFT only)."""
    yoff, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb = (np.int32(c) for c in TABLE[standard])
    r, g, b = (a.astype(np.int32) for a in (r, g, b))
    half, mid = np.int32(1 << (shift - 1)), np.int32(128 << shift)
    y = cyr * r + cyg * g + cyb * b + np.int32(int(yoff) << SHIFT) + np.int32(1 << (SHIFT - 1))
    u = cub * b - cur * r - cug * g + mid + half
    v = cvr * r - cvg * g - cvb * b + mid + half
    return y, u, v


def rgb_to_yuv(standard, rgb, raw=False):
    """The 4:4:4 form on uint8 [..., 3]: (y, u, v) uint8 [...]; raw: int32, U and V before the min."""
    y, u, v = accumulators(standard, rgb[..., 0], rgb[..., 1], rgb[..., 2], SHIFT)
    y, u, v = y >> SHIFT, u >> SHIFT, v >> SHIFT
    if raw:
        return y, u, v
    return y.astype(np.uint8), np.minimum(u, 255).astype(np.uint8), np.minimum(v, 255).astype(np.uint8)


def block_sums(rgb):
    """int32 [..., h/2, w/2, 3]: the sums over the whole 2 x 2 blocks of [..., h, w, 3] (an odd last row or
    column belongs to none)."""
    h, w = rgb.shape[-3:-1]
    ch, cw = h // 2, w // 2
    a = rgb[..., :2 * ch, :2 * cw, :].astype(np.int32)
    return a[..., 0::2, 0::2, :] + a[..., 0::2, 1::2, :] + a[..., 1::2, 0::2, :] + a[..., 1::2, 1::2, :]


def rgb_to_yuv420(standard, rgb, raw=False):
    """The 4:2:0 form on uint8 [..., h, w, 3]: y [..., h, w], u and v [..., h/2, w/2]."""
    y = (accumulators(standard, rgb[..., 0], rgb[..., 1], rgb[..., 2], SHIFT)[0] >> SHIFT)
    s = block_sums(rgb)
    _, u, v = accumulators(standard, s[..., 0], s[..., 1], s[..., 2], SUM_SHIFT)
    u, v = u >> SUM_SHIFT, v >> SUM_SHIFT
    if raw:
        return y, u, v
    return y.astype(np.uint8), np.minimum(u, 255).astype(np.uint8), np.minimum(v, 255).astype(np.uint8)


def tight(layout, y, u, v):
    """Planes [F, ...] in the tight frame layout [F, bytes] of Nv12Resizer / Yuv420Resizer.resize_frames."""
    n = y.shape[0]
    chroma = np.stack([u, v], axis=3) if layout == "nv12" else np.stack([u, v], axis=1)
    return np.ascontiguousarray(np.concatenate([y.reshape(n, -1), chroma.reshape(n, -1)], axis=1))


# ---- host sizes (w, h) of test_rgbyuv_host.py
HOST_SIZES = [(2, 2), (3, 2), (2, 3), (9, 7), (16, 4), (33, 17)]

# ---- GPU shapes (packed_cases rows: method, degree, sw, sh, dw, dh, pxScale).  Every method with an
# up-scale and a down-scale, the one packed_general shape, and the smallest outputs at which rgb_yuv_kernel
# can go wrong: dstW of 2 and 3 (narrower than a thread's 8 pixels), dstW % 8 in {1, 4, 7} (tail stores),
# dstH = 2 (one row pair), dstH = 3 (the last row has no partner and no chroma), odd x odd, several groups
# per row and several row pairs.
GPU_SHAPES = [
    ("lanczos", 3, 64, 32, 33, 17, 1),     # down-scale, odd x odd, dstW % 8 = 1
    ("lanczos", 2, 24, 16, 52, 36, 1),     # up-scale, dstW % 8 = 4, seven groups per row
    ("area", 0, 80, 48, 47, 23, 1),        # down-scale, odd x odd, dstW % 8 = 7
    ("area", 0, 16, 16, 2, 2, 1),          # dstW = 2, dstH = 2: one chroma sample
    ("area", 0, 12, 10, 30, 25, 1),        # up-scale, odd dstH
    ("area", 0, 40, 24, 20, 3, 1),         # dstH = 3 with several groups per row
    ("linear", 0, 16, 16, 3, 3, 1),        # dstW = 3, dstH = 3: one chroma sample, a Y-only column and row
    ("linear", 0, 20, 12, 40, 24, 1),      # up-scale 2x, whole groups only
    ("linear", 0, 64, 48, 36, 26, 1),      # down-scale, dstW % 8 = 4
    pc.GENERAL_SHAPE,                      # packed_general: Lanczos-8 96x64 -> 48x32
]
COMBOS = [(3, "nv12"), (3, "i420"), (4, "nv12"), (4, "i420")]  # every rgb_yuv_kernel<C, UV2>
# (shape, C, layout, order, standard): both orders and the four standards dealt over the rows, so that
# every combo meets both orders and all four standards
GPU_CASES = [(shape, C, layout, ("rgb", "bgr")[(i + k // 2 + k) % 2], STANDARDS[(i + k) % 4])
             for i, shape in enumerate(GPU_SHAPES) for k, (C, layout) in enumerate(COMBOS)]
LAYOUT_SHAPE = GPU_SHAPES[0]

N_FRAMES = 3


def first_pass_kernel(shape, C):
    """The packed kernel the first pass runs, written out (tests/test_rgbyuv_host.py compares it with the
    host query, tests/test_rgbyuv_gpu.py with describe())."""
    return "packed_general" if shape == pc.GENERAL_SHAPE else "packed_tile"


def gid(row):
    shape, C, layout, order, standard = row
    return "%s-c%d-%s-%s-%s" % (pc.sid(shape), C, layout, order, NAMES[standard])


@functools.lru_cache(maxsize=None)
def frames_for(shape, C, order):
    """[3, sh, sw, C] uint8, read-only: packed_cases.frames_for noise, constant pure blue, constant pure red
    (R, G, B at the bytes ORDERS[order]; a fourth byte holds 77, which must not reach any output)."""
    _, _, sw, sh, _, _, _ = shape
    o = ORDERS[order]
    flat = np.zeros((2, sh, sw, C), np.uint8)
    if C == 4:
        flat[..., 3] = 77
    flat[0, ..., o[2]] = 255
    flat[1, ..., o[0]] = 255
    out = np.concatenate([pc.frames_for(shape, C, 1), flat])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def resized_for(shape, C, order):
    """Per-channel oracle results [3, dh, dw, C] of frames_for, computed once and read-only."""
    out = np.stack([pc.oracle_packed(shape, f) for f in frames_for(shape, C, order)])
    out.setflags(write=False)
    return out


def expected_planes(shape, C, order, standard, raw=False):
    """(y [3, dh, dw], u, v [3, dh/2, dw/2]) of frames_for(shape, C, order)."""
    rgb = resized_for(shape, C, order)[..., list(ORDERS[order])]
    return rgb_to_yuv420(standard, rgb, raw)


def expected_frames(row):
    """The tight frames [3, dw dh + 2 cw ch] of a GPU_CASES row."""
    shape, C, layout, order, standard = row
    return tight(layout, *expected_planes(shape, C, order, standard))
