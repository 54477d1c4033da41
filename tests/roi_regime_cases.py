"""Case tables of the crop-and-resize regime tests (tests/test_roi_regimes_host.py, tests/test_roi_regimes_gpu.py).
Test infrastructure only.

tests/roi_cases.py runs roi_kernel in one corner: 32 x 24 outputs (three full bands of 8 rows), at most 14 boxes
(one search round), noise, 4-byte aligned pixels at C = 4.  The tables here name the other regimes, one literal
row each:

  A  output sizes, remainder bands and Lanczos degrees         2 x (128 x 96) noise
  B  wide boxes: rows per workgroup 7 .. 1, the largest LDS    1 x (4096 x 40), and one frame at the widest box
  C  box counts: 1 .. 4097 boxes, three search rounds          3 x (64 x 48) noise
  D  extreme frames: the Lanczos tap-sign and border-stress sets of tests/extreme_cases.py, and flat /
     striped frames for Area and Linear, pasted into a canvas of foreign pixels

A case is (regime, method, degree, frame set, boxes, dstW, dstH).  The expected output of a box is the Generic
oracle on the cropped plane, per channel, reversed along the columns for a flipped box; every Lanczos box goes
through oracle_lib.lanczos_rows_defined, and every Linear box through the <= 2x rule, before the oracle is called.
"""
import collections
import functools

import numpy as np

import extreme_cases as ec
import libiqo_amd
import oracle_lib as ol

Case = collections.namedtuple("Case", "regime method degree fid boxes dw dh")
CHANNELS = (1, 3, 4)


def cid(c):
    return "%s%d-%s-%dx%d-n%d" % (c.method, c.degree, c.fid, c.dw, c.dh, len(c.boxes))


def flipped(b):
    return len(b) == 6 and bool(b[5])


def answerable(method, degree, b, dw, dh):
    """What the library accepts and the oracle has an answer for: Lanczos rows defined, Linear at most 2x up, and
    both axes within ROI_MAX_TAPS."""
    w, h = b[3], b[4]
    if method == "linear":
        return dw <= 2 * w and dh <= 2 * h
    if method == "lanczos":
        if not ol.lanczos_rows_defined(degree, h, dh):
            return False
        return max(ol.lanczos_taps(degree, w, dw), ol.lanczos_taps(degree, h, dh)) <= libiqo_amd.ROI_MAX_TAPS
    return True


# ----------------------------------------------------------------------------- frame sets
#
# A frame set is known by its id; _planes(fid, C) gives [F, H, W, C] with the pixel bytes the library sees, and
# frames(fid, C) the array a test hands over ([F, H, W] for C = 1).

A_FRAMES, A_W, A_H = 2, 128, 96
B_W, B_H = 4096, 40
C_FRAMES, C_W, C_H = 3, 64, 48
PASTE_X, PASTE_Y = 3, 2  # where table D's frames lie in their canvas [n, h + 5, w + 7]


def _noise4(n, h, w, seed):
    return ol.splitmix_bytes(n * h * w * 4, seed).reshape(n, h, w, 4)


def _canvas(planes, seed):
    """planes [n, h, w] pasted at (3, 2) into [n, h + 5, w + 7]; the background is the complement of noise."""
    n, h, w = planes.shape
    out = 255 - ol.splitmix_bytes(n * (h + 5) * (w + 7), seed).reshape(n, h + 5, w + 7)
    out[:, PASTE_Y:PASTE_Y + h, PASTE_X:PASTE_X + w] = planes
    return out


def flat_and_stripes(w, h):
    """Area / Linear have no signs to exploit: the unsigned 16-bit work value and the udot2 sum at their largest
    (flat 255), at zero, and swinging between both from one sample to the next along either axis."""
    col = np.broadcast_to((np.arange(w) & 1) * 255, (h, w))
    row = np.broadcast_to(((np.arange(h) & 1) * 255)[:, None], (h, w))
    return np.stack([np.full((h, w), 255), np.zeros((h, w)), col, row, 255 - col, 255 - row]).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _planes(fid, C):
    kind = fid[0]
    if kind == "A":
        out = _noise4(A_FRAMES, A_H, A_W, 31337)[..., :C]
    elif kind == "B":
        # ONE buffer of 4096 x 40 x 4 bytes; the C = 1 and C = 3 frames are views of the same bytes (rows stay
        # 16384 bytes apart): 16384 grey pixels, or 5461 RGB pixels, per row
        buf = ol.splitmix_bytes(B_H * B_W * 4, 4096).reshape(1, B_H, B_W * 4)
        wpx = B_W * 4 // C
        out = np.lib.stride_tricks.as_strided(buf, (1, B_H, wpx, C), (buf.strides[0], buf.strides[1], C, 1))
    elif kind == "W":  # ("W", w): one frame w x 8, the widest box
        out = _noise4(1, 8, fid[1], 8000 + fid[1])[..., :C]
    elif kind == "C":
        out = _noise4(C_FRAMES, C_H, C_W, 5)[..., :C]
    elif kind == "D":  # ("D", degree, w, h, dw, dh): channel c of canvas frame i is plane (i + c) mod n
        _, fr = ec.plane_frames(fid[1], fid[2], fid[3], fid[4], fid[5], 1, stress=True)
        cv = _canvas(fr, 1000 + fid[2])
        n = cv.shape[0]
        out = np.stack([cv[(np.arange(n) + c) % n] for c in range(C)], axis=3)
    elif kind == "E":  # ("E", w, h)
        cv = _canvas(flat_and_stripes(fid[1], fid[2]), 2000 + fid[1])
        n = cv.shape[0]
        out = np.stack([cv[(np.arange(n) + c) % n] for c in range(C)], axis=3)
    else:
        raise ValueError(fid)
    out = out if kind == "B" else np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def frames(fid, C):
    """uint8 [F, H, W] (C = 1) or [F, H, W, C] of a frame set."""
    p = _planes(fid, C)
    return p[..., 0] if C == 1 else p


def _plane_key(fid, C, frame, c):
    """Which plane channel c of frame `frame` is, so that one oracle result serves every C that shows the plane."""
    if fid[0] in ("D", "E"):
        return ((frame + c) % _planes(fid, 1).shape[0], 0, 1)
    if fid[0] == "B":
        return (frame, c, C)
    return (frame, c, 4)


@functools.lru_cache(maxsize=None)
def _oracle(method, degree, fid, pkey, x, y, w, h, dw, dh):
    assert answerable(method, degree, (0, x, y, w, h), dw, dh), (method, degree, w, h, dw, dh)
    frame, c, C = pkey
    crop = np.ascontiguousarray(_planes(fid, C)[frame, y:y + h, x:x + w, c])
    exp = np.array(ol.run_oracle(method, degree, w, h, dw, dh, 1, crop))
    exp.setflags(write=False)
    return exp


def crop(case, C, b, c):
    """Channel c of box b of the case's frames at C channels, as a contiguous plane."""
    frame, ch, planes_c = _plane_key(case.fid, C, b[0], c)
    return np.ascontiguousarray(_planes(case.fid, planes_c)[frame, b[2]:b[2] + b[4], b[1]:b[1] + b[3], ch])


def oracle_plane(case, C, b, c):
    """The oracle on crop(case, C, b, c), unflipped (cached)."""
    return _oracle(case.method, case.degree, case.fid, _plane_key(case.fid, C, b[0], c), b[1], b[2], b[3], b[4], case.dw,
                   case.dh)


def expected(case, C, box_list=None):
    """uint8 [N, dh, dw] (C = 1) or [N, dh, dw, C]: the oracle per box and channel, flipped where flagged."""
    box_list = case.boxes if box_list is None else box_list
    out = np.zeros((len(box_list), case.dh, case.dw, C), np.uint8)
    for i, b in enumerate(box_list):
        for c in range(C):
            p = oracle_plane(case, C, b, c)
            out[i, :, :, c] = p[:, ::-1] if flipped(b) else p
    return out[..., 0] if C == 1 else out


def twin(case, C, box_list=None, **kw):
    box_list = case.boxes if box_list is None else box_list
    return libiqo_amd.host_resize_rois(case.method, case.degree, case.dw, case.dh, frames(case.fid, C), box_list, **kw)


def layout(case, C, b):
    return libiqo_amd.host_roi_box_layout(case.method, case.degree, C, case.dw, case.dh, b[3], b[4])


# ----------------------------------------------------------------------------- A: sizes, bands, degrees

A_BOXES = (
    (0, 1, 2, 64, 48),
    (1, 3, 5, 45, 31),
    (1, 2, 7, 20, 13, 1),
    (0, 5, 0, 123, 96),
    (1, 0, 0, 128, 96, 1),
    (0, 127, 95, 1, 1),
)


def _a(regime, method, degree, dw, dh):
    boxes = tuple(b for b in A_BOXES if answerable(method, degree, b, dw, dh))
    return Case(regime, method, degree, ("A",), boxes, dw, dh)


TABLE_A = [
    _a("one output pixel: a band of one row, one task", "area", 0, 1, 1),
    _a("one output pixel", "linear", 0, 1, 1),
    _a("one output pixel, up to 120 taps", "lanczos", 1, 1, 1),
    _a("one output pixel: what fits the tap cap", "lanczos", 3, 1, 1),
    _a("rows = dstH = 3: a single band shorter than 8", "area", 0, 5, 3),
    _a("rows = dstH = 3", "linear", 0, 5, 3),
    _a("rows = dstH = 3; all six boxes within the cap", "lanczos", 1, 5, 3),
    _a("rows = dstH = 3", "lanczos", 3, 5, 3),
    _a("8 + 1 rows: a remainder band of one row", "area", 0, 7, 9),
    _a("8 + 1 rows", "linear", 0, 7, 9),
    _a("8 + 1 rows", "lanczos", 1, 7, 9),
    _a("8 + 1 rows; five boxes (1 x 1 has no defined rows)", "lanczos", 3, 7, 9),
    _a("8 + 8 + 4 rows", "area", 0, 32, 20),
    _a("8 + 8 + 4 rows", "linear", 0, 32, 20),
    _a("8 + 8 + 4 rows, degree 1: two taps up", "lanczos", 1, 32, 20),
    _a("8 + 8 + 4 rows, degree 3", "lanczos", 3, 32, 20),
    _a("8 + 8 + 4 rows, degree 4", "lanczos", 4, 32, 20),
    _a("8 + 8 + 4 rows, degree 6", "lanczos", 6, 32, 20),
    _a("8 + 8 + 4 rows, degree 9: 18 taps up, 54 down", "lanczos", 9, 32, 20),
    _a("odd width with flips, 8 + 8 + 5 rows", "area", 0, 33, 21),
    _a("odd width with flips", "linear", 0, 33, 21),
    _a("odd width with flips, degree 1", "lanczos", 1, 33, 21),
    _a("odd width with flips, degree 3", "lanczos", 3, 33, 21),
    _a("odd width with flips, degree 4", "lanczos", 4, 33, 21),
    _a("odd width with flips, degree 6", "lanczos", 6, 33, 21),
    _a("odd width with flips, degree 9", "lanczos", 9, 33, 21),
    _a("six full bands and 4 rows; up-scales of the small boxes", "area", 0, 56, 52),
    _a("six full bands and 4 rows", "linear", 0, 56, 52),
    _a("six full bands and 4 rows", "lanczos", 1, 56, 52),
    _a("six full bands and 4 rows", "lanczos", 3, 56, 52),
]
# the (33, 21) rows the instantiation test takes: flips at an odd width
A_INSTANCE = {c.method: c for c in TABLE_A if (c.method, c.degree, c.dw, c.dh) in (("lanczos", 3, 33, 21), ("area", 0, 33, 21))}
assert sorted(A_INSTANCE) == ["area", "lanczos"]

# ----------------------------------------------------------------------------- B: wide boxes

B_DW, B_DH = 512, 12
B_WIDTHS = (520, 1100, 2000, 4093)


def _b(regime, method, degree, boxes):
    return Case(regime, method, degree, ("B",), tuple(boxes), B_DW, B_DH)


TABLE_B = [
    _b("rows 8 (C 1) / 4 (C 3) / 3 (C 4), with a narrow box at rows = 8 in the wide box's LDS", "lanczos", 3,
       [(0, 3, 1, 520, 36), (0, 0, 0, 40, 30)]),
    _b("rows 6 / 2 / 1", "lanczos", 3, [(0, 3, 1, 1100, 36), (0, 0, 0, 40, 30)]),
    _b("rows 3 / 1 / 1", "lanczos", 3, [(0, 3, 1, 2000, 36), (0, 0, 0, 40, 30)]),
    _b("rows 1 at every C: twelve bands of one row", "lanczos", 3, [(0, 3, 1, 4093, 36), (0, 0, 0, 40, 30)]),
    _b("rows 8 / 5 / 3 (5: bands of 5, 5 and 2), flipped, ends at the frame's last column", "area", 0,
       [(0, B_W - 520, 4, 520, 36, 1)]),
    _b("rows 7 / 2 / 1 (7: a band of 7 and a remainder of 5)", "area", 0, [(0, B_W - 1100, 4, 1100, 36, 1)]),
    _b("rows 4 / 1 / 1", "area", 0, [(0, B_W - 2000, 4, 2000, 36, 1)]),
    _b("rows 1 / 1 / 1", "area", 0, [(0, B_W - 4093, 4, 4093, 36, 1)]),
]
assert all(b[1] + b[3] <= B_W for c in TABLE_B for b in c.boxes)

WIDEST_DH = 4
WIDEST_DW = {"lanczos": 1024, "area": 512}  # at most 8:1 (Lanczos-3) and 16:1 (Area) for w <= 8192


@functools.lru_cache(maxsize=None)
def widest(method, degree):
    """The widest box of 8 rows the library accepts at C = 4 (the work row fills ROI_LDS_BYTES), found as
    test_tap_cap finds its widths: every width of a range asked, the last accepted one taken."""
    dw = WIDEST_DW[method]
    ok = {}
    for w in range(8192, 7936, -1):
        try:
            ok[w] = libiqo_amd.host_roi_box_layout(method, degree, 4, dw, WIDEST_DH, w, 8)
        except libiqo_amd.IqoError as e:
            assert e.status == -5, str(e)  # IQO_HIP_EUNSUP
        if len(ok) >= 2:
            break
    at = max(ok)
    assert at < 8192 and at - 1 in ok, "the range does not hold the limit"
    return at


def widest_case(method, degree):
    w = widest(method, degree)
    return Case("the widest box at C = 4: the largest dynamic LDS the library asks for", method, degree, ("W", w),
                ((0, 0, 0, w, 8),), WIDEST_DW[method], WIDEST_DH)


WIDEST = (("lanczos", 3), ("area", 0))

# ----------------------------------------------------------------------------- C: box counts

C_DW, C_DH = 8, 20
C_SHAPES = ((16, 40), (8, 20), (24, 33), (9, 45), (64, 48), (30, 20))
C_COUNTS = (1, 2, 63, 64, 65, 4096, 4097)
# Batches queued on one plan and one stream without synchronisation.  A plan has two arenas and uses them alternately,
# so in C_QUEUE the first arena only ever sees 2, 2 and 65 boxes and the second is ALLOCATED at its large size;
# C_REGROW gives each arena a small batch first, so that each is freed and reallocated (while the launch on the
# other one is in flight), and then reuses both.
C_QUEUE = (2, 4097, 2, 4097, 65)
C_REGROW = (2, 65, 4097, 4096, 65, 4097)


@functools.lru_cache(maxsize=None)
def _count_boxes():
    rs = np.random.RandomState(5)
    out = []
    for i in range(max(C_COUNTS)):
        w, h = C_SHAPES[i % len(C_SHAPES)]
        out.append((int(rs.randint(C_FRAMES)), int(rs.randint(C_W - w + 1)), int(rs.randint(C_H - h + 1)), w, h,
                    1 if i % 5 == 4 else 0))
    return tuple(out)


def _c(regime, method, degree, n):
    return Case(regime, method, degree, ("C",), _count_boxes()[:n], C_DW, C_DH)


TABLE_C = [
    _c("one box: the search loop does not run", "lanczos", 2, 1),
    _c("two boxes: one round", "lanczos", 2, 2),
    _c("63 boxes: one round, the last lane idle", "lanczos", 2, 63),
    _c("64 boxes: one round, every lane a box", "lanczos", 2, 64),
    _c("65 boxes: two rounds, step 2", "lanczos", 2, 65),
    _c("4096 boxes: two rounds, step 64", "lanczos", 2, 4096),
    _c("4097 boxes: three rounds (65, 2, 1); the arena outgrows its first 2^16 words", "lanczos", 2, 4097),
]
C_AREA = _c("4097 boxes, three channels, unsigned arithmetic", "area", 0, 4097)  # at C = 3


def search_rounds(n):
    """Rounds of roi_kernel's 64-way search over n boxes: its recurrence, for a workgroup of box 0 (k = 0)."""
    rounds = 0
    while n > 1:
        n, rounds = min((n + 63) >> 6, n), rounds + 1
    return rounds


# ----------------------------------------------------------------------------- D: extreme frames

def _d(regime, degree, w, h, dw, dh):
    fid = ("D", degree, w, h, dw, dh)
    n = ec.plane_frames(degree, w, h, dw, dh, 1, stress=True)[1].shape[0]
    return Case(regime, "lanczos", degree, fid, tuple((i, PASTE_X, PASTE_Y, w, h, i & 1) for i in range(n)), dw, dh)


def _e(regime, method, w, h, dw, dh):
    n = flat_and_stripes(1, 1).shape[0]
    return Case(regime, method, 0, ("E", w, h), tuple((i, PASTE_X, PASTE_Y, w, h, i & 1) for i in range(n)), dw, dh)


# every shape is a row of DESIGN.md "Extreme inputs"; the crop-and-resize has no pxScale, so the negative X
# denominators of that table (pxScale 2 only) cannot occur here
TABLE_D = [
    _d("negative Y denominators, wrapping quotients; the reference runs it", 7, 256, 26, 128, 13),
    _d("wrapping quotients at a short source; the reference runs it", 5, 120, 30, 50, 9),
    _d("negative Y denominators and wraps at degree 9; the reference runs it", 9, 256, 24, 128, 12),
    _d("wraps at a non-integer ratio; the reference runs it", 7, 120, 24, 50, 13),
    _d("an up-scale with a Y-main stage: both main clamps", 3, 100, 37, 130, 71),
    _d("a Y-main stage at degree 4", 4, 200, 140, 137, 93),
    _d("the 2:1 corner of tests/roi_cases.py on extreme frames", 3, 64, 48, 32, 24),
]
TABLE_E = [
    _e("16:1 on both axes: the udot2 sum and the 16-bit work value at their largest", "area", 512, 128, 32, 8),
    _e("the same at the tap cap: 128 taps on both axes, one output pixel", "area", 128, 128, 1, 1),
    _e("a non-integer Area ratio: weights that do not divide", "area", 45, 31, 32, 24),
    _e("Linear down", "linear", 45, 31, 32, 24),
    _e("Linear up: the replicated edge column carries weight", "linear", 20, 13, 32, 24),
]
# the counters of oracle_lib.run_oracle_stats table D must reach, summed over its shapes
D_COUNTERS = ("ym_neg", "ym_hi", "yb_nume_neg", "yb_deno_neg", "yb_q_wrap", "xm_neg", "xm_hi", "xb_nume_neg",
              "xb_q_lo", "xb_q_hi")


def all_cases():
    """(case, channel counts) of every table."""
    out = [(c, CHANNELS) for c in TABLE_A + TABLE_B]
    out += [(widest_case(m, d), (4,)) for m, d in WIDEST]
    out += [(c, (1,)) for c in TABLE_C] + [(C_AREA, (3,))]
    out += [(c, CHANNELS) for c in TABLE_D + TABLE_E]
    return out
