"""Shared cases of the NV12 / I420 crop-and-resize tests (tests/test_roi_yuv_host.py, tests/test_roi_yuv_gpu.py).
Test infrastructure only.

Frames are 3 NV12 frames of 160 x 120 with splitmix noise in Y and in UV (the I420 frames are the same frames
de-interleaved); the output is 32 x 24.  The expected output of a box is the Generic oracle per component on the
cropped planes -- Y: (w, h) -> (32, 24); U and V: (w/2, h/2) -> (32, 24); pixel scale 1 -- then the integer matrix
of yuvrgb_cases, reversed along the columns for a flipped box.  Every box goes through
oracle_lib.lanczos_rows_defined, for h and for h/2, before the oracle is called on it.
"""
import functools

import numpy as np

import oracle_lib as ol
import yuvrgb_cases as yr

FRAMES, FW, FH = 3, 160, 120
DW, DH = 32, 24
METHODS = (("lanczos", 2), ("lanczos", 3), ("lanczos", 5), ("area", 0), ("linear", 0))
# the four standards dealt over the methods
STANDARD = {m: yr.STANDARDS[i % 4] for i, m in enumerate(METHODS)}
LAYOUTS = ("nv12", "i420")
EINVAL, EUNSUP = -1, -5

# (frame, x, y, w, h[, flip]), all even
BOXES = (
    (0, 0, 0, 64, 48),         # luma 2:1, chroma the identity
    (0, 2, 6, 32, 24),         # luma the identity, chroma exactly 2x up
    (1, 4, 10, 90, 62),        # multi-phase down on all four axes
    (1, 6, 14, 40, 26),        # up in luma and chroma
    (2, 30, 20, 130, 100),     # about 4:1; ends at the last frame's corner
    (2, 10, 40, 96, 48),       # chroma Y axis the identity
    (0, 40, 2, 90, 100),       # shares the X tables of width 90
    (0, 8, 58, 100, 62),       # shares the Y tables of height 62 (y = 58: the box ends at the frame's last row)
    (1, 4, 10, 90, 62, 1),     # mirrored
    (2, 16, 12, 128, 96),      # its chroma tables are the luma tables of 64 x 48
    (0, 156, 116, 4, 4),       # frame 0's last bytes; chroma 2 x 2
    (1, 100, 50, 14, 10),      # no main region
    (1, 148, 60, 2, 20),       # chroma one column wide
)
# what a method's case list may leave out, at most
MAY_LEAVE_OUT = {("lanczos", 5): BOXES[10:11], ("linear", 0): BOXES[10:]}

# (method, degree, boxes, status, first offending box): the rejections
GOOD = BOXES[0]
REJECTED = (
    ("lanczos", 3, [GOOD, (0, 0, 0, 16, 2)], EINVAL, 1),   # luma 2 -> 24 is defined, chroma 1 -> 24 is not
    ("lanczos", 5, [GOOD, (0, 0, 0, 16, 4)], EINVAL, 1),
    ("lanczos", 5, [(0, 0, 0, 16, 6)], EINVAL, 0),
    ("linear", 0, [GOOD, GOOD, (0, 0, 0, 14, 10)], EUNSUP, 2),
    ("area", 0, [GOOD, (0, 1, 0, 16, 16)], EINVAL, 1),    # odd x, y, w, h, each alone
    ("area", 0, [(0, 0, 3, 16, 16)], EINVAL, 0),
    ("lanczos", 3, [GOOD, (0, 0, 0, 15, 16)], EINVAL, 1),
    ("lanczos", 3, [GOOD, (0, 0, 0, 16, 17)], EINVAL, 1),
)


@functools.lru_cache(maxsize=None)
def planes():
    """(Y [3, 120, 160], U [3, 60, 80], V [3, 60, 80]), read-only."""
    y = ol.splitmix_bytes(FRAMES * FH * FW, 20250).reshape(FRAMES, FH, FW)
    uv = ol.splitmix_bytes(FRAMES * FH * FW // 2, 20251).reshape(FRAMES, FH // 2, FW // 2, 2)
    out = (y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]))
    for a in out:
        a.setflags(write=False)
    return out


def frames_of(y, u, v, layout):
    """Planes [F, h, w], [F, h/2, w/2] x 2 in the tight frame layout [F, w*h*3/2]."""
    n = y.shape[0]
    if layout == "nv12":
        chroma = [np.stack([u, v], axis=3).reshape(n, -1)]
    else:
        chroma = [u.reshape(n, -1), v.reshape(n, -1)]
    return np.ascontiguousarray(np.concatenate([y.reshape(n, -1)] + chroma, axis=1))


@functools.lru_cache(maxsize=None)
def frames(layout):
    out = frames_of(*planes(), layout)
    out.setflags(write=False)
    return out


def defined(method, degree, w, h, dh=DH):
    return method != "lanczos" or (ol.lanczos_rows_defined(degree, h, dh) and ol.lanczos_rows_defined(degree, h // 2, dh))


@functools.lru_cache(maxsize=None)
def boxes(method, degree):
    """The case list of a method: what the library accepts and the oracle has an answer for."""
    out = []
    for b in BOXES:
        w, h = b[3], b[4]
        if method == "linear" and (DW > 2 * (w // 2) or DH > 2 * (h // 2)):
            continue
        if not defined(method, degree, w, h):
            continue
        out.append(b)
    assert out and set(BOXES) - set(out) <= set(MAY_LEAVE_OUT.get((method, degree), ())), (method, degree)
    return tuple(out)


def oracle_box(method, degree, y, u, v, b, dw=DW, dh=DH):
    """The oracle's (Y, U, V) [dh, dw] of box b of planes [F, h, w] / [F, h/2, w/2], not flipped."""
    f, x, yy, w, h = b[:5]
    assert defined(method, degree, w, h, dh)
    crops = (y[f, yy:yy + h, x:x + w], u[f, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2],
             v[f, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2])
    return tuple(np.array(ol.run_oracle(method, degree, c.shape[1], c.shape[0], dw, dh, 1, np.ascontiguousarray(c)))
                 for c in crops)


@functools.lru_cache(maxsize=None)
def expected_planes(method, degree):
    """Per box of boxes(method, degree): the oracle's (Y, U, V), not flipped; read-only."""
    out = tuple(oracle_box(method, degree, *planes(), b) for b in boxes(method, degree))
    for t in out:
        for a in t:
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected(method, degree, standard=None):
    """uint8 [N, 24, 32, 3] (R, G, B) of boxes(method, degree), flipped where flagged; read-only."""
    standard = STANDARD[(method, degree)] if standard is None else standard
    bl = boxes(method, degree)
    out = np.zeros((len(bl), DH, DW, 3), np.uint8)
    for i, (b, (y, u, v)) in enumerate(zip(bl, expected_planes(method, degree))):
        rgb = yr.yuv_to_rgb(standard, y, u, v)
        out[i] = rgb[:, ::-1] if len(b) == 6 and b[5] else rgb
    out.setflags(write=False)
    return out


def same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])
