"""The expected value and the shapes of the full-grid chroma (IQO_CHROMA_FULL, chroma="full") tests of the
NV12 / I420 "resize to RGB" entries (tests/test_yuv444_host.py, tests/test_yuv444_gpu.py).  Test
infrastructure only.

The definition (include/iqo_hip.h, IQO_CHROMA_FULL) is written once here: with the inputs of
yuvrgb_cases.planes_for (5 frames, the two clamp frames included),

    Y    = oracle_lib.run_oracle(method, degree, sw,      sh      -> dw, dh, pxScale 1)
    U, V = oracle_lib.run_oracle(method, degree, sw // 2, sh // 2 -> dw, dh, pxScale 1)

and pixel (y, x) is yuvrgb_cases.yuv_to_rgb of (Y, U, V) at (y, x): elementwise, no index shift, no clamp
of an index.  Float outputs are norm_cases.expected_bits of these bytes.

Shapes: the smallest at which the new path can go wrong.  Every row names the kernel family the full-grid
chroma plan runs (libiqo_amd.host_chroma_full_kernel); the standards are dealt over each list in turn.
"""
import functools

import numpy as np

import oracle_lib as ol
import yuvrgb_cases as yr

# (method, degree, srcW, srcH, dstW, dstH), family of the 2-channel packed chroma plan
NV12_SHAPES = [
    (("lanczos", 3, 64, 32, 33, 17), "packed_tile"),     # odd x odd, dstW % 8 = 1: the last column's own sample
    (("lanczos", 2, 24, 16, 52, 36), "packed_tile"),     # 4.3x chroma up-scale, dstW % 8 = 4
    (("lanczos", 3, 64, 32, 32, 16), "packed_tile"),     # luma 2:1: the chroma plan is the identity
    (("lanczos", 3, 96, 64, 22, 15), "packed_tile"),     # chroma down-scale, dstW % 8 = 6
    (("area", 0, 80, 48, 47, 23), "packed_tile"),        # dstW % 8 = 7, chroma up in X and down in Y
    (("area", 0, 16, 16, 2, 2), "packed_tile"),          # dstW = 2
    (("area", 0, 12, 10, 30, 25), "packed_general"),     # odd dstH
    (("area", 0, 32, 16, 16, 8), "packed_tile"),
    (("linear", 0, 16, 16, 3, 2), "packed_tile"),        # dstW = 3
    (("linear", 0, 64, 48, 36, 26), "packed_tile"),
    (("linear", 0, 40, 24, 40, 24), "packed_tile"),      # chroma exactly 2x
    (("linear", 0, 128, 16, 64, 8), "packed_tile"),
]

# ... and of the planar chroma plan
I420_SHAPES = [
    (("lanczos", 3, 64, 32, 64, 32), "lanczos_up2"),
    (("lanczos", 3, 96, 48, 64, 32), "ryg"),
    (("lanczos", 3, 384, 96, 128, 32), "lanczos_d32"),
    (("lanczos", 3, 256, 64, 64, 16), "lanczos_stream"),
    (("lanczos", 3, 64, 32, 32, 16), "walk"),
    (("lanczos", 4, 128, 64, 48, 24), "ryg"),
    (("area", 0, 128, 16, 32, 4), "area_int"),
    (("area", 0, 192, 48, 32, 8), "area_int"),
    (("area", 0, 96, 48, 64, 32), "walk"),
    (("area", 0, 12, 10, 30, 25), "general"),
    (("area", 0, 16, 16, 2, 2), "tile"),
    (("linear", 0, 64, 16, 64, 16), "linear_up2"),
    (("linear", 0, 128, 32, 32, 8), "area_int"),
    (("linear", 0, 96, 48, 64, 32), "walk"),
    (("linear", 0, 16, 16, 3, 2), "tile"),
]


def _rows(shapes, layout):
    return [(shape + (layout,), yr.STANDARDS[i % 4], family) for i, (shape, family) in enumerate(shapes)]


# (case, standard, family): `case` is a yuv_cases / yuvrgb_cases row (the shape and a label, here the layout)
NV12_CASES = _rows(NV12_SHAPES, "nv12")
I420_CASES = _rows(I420_SHAPES, "i420")

# set_chroma("full") is rejected for these, under plans that are accepted: (shape, status)
EINVAL, EUNSUP = -1, -5
REJECTED = [
    (("linear", 0, 20, 12, 40, 24), EUNSUP),   # chroma 10x6 -> 40x24: Linear 4x
    (("linear", 0, 48, 6, 144, 18), EUNSUP),   # Linear 6x
    (("lanczos", 3, 16, 3, 16, 3), EINVAL),    # chroma 8x1 -> 16x3 has no defined rows
]


def cid(row):
    case, standard, _ = row
    return "%s%d-%dx%d-%dx%d-%s-%s" % (case + (yr.NAMES[standard],))


def chroma_shape(case):
    """(srcW, srcH, dstW, dstH, pxScale) of the full-grid U and V planes."""
    _, _, sw, sh, dw, dh, _ = case
    return sw // 2, sh // 2, dw, dh, 1


@functools.lru_cache(maxsize=None)
def expected_planes(case):
    """Per-plane oracle outputs Y, U, V, each [5, dh, dw], of yuvrgb_cases.planes_for(case); read-only."""
    m, d, sw, sh, dw, dh, _ = case
    y, u, v = yr.planes_for(case)
    cw, ch, cdw, cdh, px = chroma_shape(case)
    n = y.shape[0]
    out = (np.stack([ol.run_oracle(m, d, sw, sh, dw, dh, 1, y[f]) for f in range(n)]),
           np.stack([ol.run_oracle(m, d, cw, ch, cdw, cdh, px, u[f]) for f in range(n)]),
           np.stack([ol.run_oracle(m, d, cw, ch, cdw, cdh, px, v[f]) for f in range(n)]))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_rgb(case, standard):
    """RGB bytes [5, dh, dw, 3] of chroma="full"; read-only."""
    y, u, v = expected_planes(case)
    out = yr.yuv_to_rgb(standard, y, u, v)
    out.setflags(write=False)
    return out


def raw_rgb(case, standard):
    """The shifted sums before the clamp, int32 [5, dh, dw, 3]."""
    y, u, v = expected_planes(case)
    return yr.raw_rgb(standard, y, u, v)


def frames(case):
    """yuvrgb_cases.planes_for(case) in the tight frame layout of the case's resizer: [5, bytes]."""
    return yr.nv12_frames(case) if case[6] == "nv12" else yr.i420_frames(case)
