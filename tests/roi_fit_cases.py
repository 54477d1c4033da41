"""Shared cases of the tests of boxes into destination rectangles (tests/test_roi_fit_host.py,
tests/test_roi_fit_gpu.py).  Test infrastructure only.

The frames are roi_cases' (3 x 160 x 120, up to 4 channels) and roi_yuv_cases' (3 NV12 / I420 frames of 160 x 120);
the canvas is 48 x 40.  The expected canvas of a case is the pad colour with the Generic oracle on the cropped
plane, (w, h) -> (iw, ih) per channel (YUV: per component, chroma from (w/2, h/2), then the integer matrix of
yuvrgb_cases), placed at (ox, oy), reversed along the columns inside the rectangle for a flipped box.  A case is
left out of a method's list as roi_cases.boxes leaves boxes out: Lanczos rows without a defined result
(oracle_lib.lanczos_rows_defined(degree, h, ih)), Linear above 2x.
"""
import functools

import numpy as np

import oracle_lib as ol
import roi_cases as rc
import roi_yuv_cases as ryc
import yuvrgb_cases as yr

CW, CH = 48, 40
METHODS = rc.METHODS
PAD = (37, 201, 90, 143)       # channel bytes (packed) / R, G, B (YUV)

# ((frame, x, y, w, h[, flip]), (ox, oy, iw, ih))
CASES = (
    ((0, 1, 3, 64, 48), (0, 0, 48, 40)),        # the whole output
    ((0, 2, 5, 64, 36), (0, 6, 48, 27)),        # letterbox
    ((1, 3, 7, 33, 60), (13, 0, 22, 40)),       # pillarbox, odd offset
    ((1, 2, 5, 45, 31), (5, 7, 31, 19)),        # all four sides
    ((1, 2, 5, 45, 31, 1), (5, 7, 31, 19)),     # the same, flipped
    ((2, 5, 11, 32, 24), (8, 8, 32, 24)),       # identity inside a border
    ((1, 3, 7, 20, 13), (4, 7, 40, 26)),        # upscale (2x: the most Linear takes)
    # (12 columns to one: 120 taps at Lanczos-5, under IQO_HIP_ROI_MAX_TAPS)
    ((2, 29, 20, 12, 1), (47, 39, 1, 1)),       # one pixel in the last corner (a box one row high: Lanczos has no
    ((2, 29, 20, 12, 20), (0, 0, 1, 40)),       # one column                    other height with a defined single row)
    ((2, 29, 20, 30, 1), (0, 0, 48, 1)),        # one row
    ((0, 40, 2, 45, 50), (2, 3, 20, 30)),       # the width of (45, 31) to another iw: two X tables of one source length
    ((0, 9, 60, 45, 40), (10, 0, 31, 33)),      # ... and to the same iw: one shared X table
)
# YUV: the same rectangles, even boxes
YUV_CASES = (
    ((0, 0, 2, 64, 48), (0, 0, 48, 40)),
    ((0, 2, 6, 64, 36), (0, 6, 48, 27)),
    ((1, 4, 8, 34, 60), (13, 0, 22, 40)),
    ((1, 2, 6, 46, 32), (5, 7, 31, 19)),
    ((1, 2, 6, 46, 32, 1), (5, 7, 31, 19)),
    ((2, 6, 12, 32, 24), (8, 8, 32, 24)),
    ((1, 4, 8, 20, 14), (4, 7, 40, 26)),        # up in luma and chroma (left out for Linear: chroma above 2x)
    ((2, 30, 20, 12, 20), (47, 39, 1, 1)),      # (Lanczos: no even height has a defined single row; Area and
    ((2, 30, 20, 12, 20), (0, 0, 1, 40)),       #  Linear take these)
    ((2, 30, 20, 30, 20), (0, 0, 48, 1)),
    ((0, 40, 2, 46, 50), (2, 3, 20, 30)),
    ((0, 10, 60, 46, 40), (10, 0, 31, 33)),
)


def accepted(method, degree, box, rect, yuv=False):
    w, h = box[3], box[4]
    iw, ih = rect[2], rect[3]
    if yuv:
        if method == "linear" and (iw > 2 * (w // 2) or ih > 2 * (h // 2)):
            return False
        return method != "lanczos" or (ol.lanczos_rows_defined(degree, h, ih) and ol.lanczos_rows_defined(degree, h // 2, ih))
    if method == "linear" and (iw > 2 * w or ih > 2 * h):
        return False
    return method != "lanczos" or ol.lanczos_rows_defined(degree, h, ih)


@functools.lru_cache(maxsize=None)
def cases(method, degree, yuv=False):
    """The case list of a method: (boxes, rects)."""
    out = [c for c in (YUV_CASES if yuv else CASES) if accepted(method, degree, c[0], c[1], yuv)]
    assert len(out) >= 9, (method, degree, len(out))
    return tuple(c[0] for c in out), tuple(c[1] for c in out)


@functools.lru_cache(maxsize=None)
def _plane(method, degree, c, frame, x, y, w, h, iw, ih):
    crop = np.ascontiguousarray(rc.frames(4)[frame, y:y + h, x:x + w, c])
    exp = np.array(ol.run_oracle(method, degree, w, h, iw, ih, 1, crop))
    exp.setflags(write=False)
    return exp


def canvas(inner, rect, pad, flip, cw=CW, ch=CH):
    """[ch, cw, C]: pad with inner [ih, iw, C] at the rectangle, reversed along its columns when flipped."""
    ox, oy, iw, ih = rect
    out = np.empty((ch, cw, inner.shape[2]), np.uint8)
    out[...] = np.asarray(pad[:inner.shape[2]], np.uint8)
    out[oy:oy + ih, ox:ox + iw] = inner[:, ::-1] if flip else inner
    return out


@functools.lru_cache(maxsize=None)
def expected(method, degree, C, pad=PAD):
    """uint8 [N, 40, 48] (C = 1) or [N, 40, 48, C] of cases(method, degree); read-only."""
    boxes, rects = cases(method, degree)
    out = np.zeros((len(boxes), CH, CW, C), np.uint8)
    for i, (b, r) in enumerate(zip(boxes, rects)):
        inner = np.stack([_plane(method, degree, c, *b[:5], r[2], r[3]) for c in range(C)], axis=2)
        out[i] = canvas(inner, r, pad, len(b) == 6 and b[5])
    out = np.ascontiguousarray(out[..., 0] if C == 1 else out)
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_yuv(method, degree, standard, pad=PAD):
    """uint8 [N, 40, 48, 3] (R, G, B) of cases(method, degree, yuv=True); read-only."""
    boxes, rects = cases(method, degree, True)
    out = np.zeros((len(boxes), CH, CW, 3), np.uint8)
    for i, (b, r) in enumerate(zip(boxes, rects)):
        y, u, v = ryc.oracle_box(method, degree, *ryc.planes(), b, dw=r[2], dh=r[3])
        out[i] = canvas(yr.yuv_to_rgb(standard, y, u, v), r, pad, len(b) == 6 and b[5])
    out.setflags(write=False)
    return out


def same(got, exp, what):
    ryc.same(got, exp, what)
