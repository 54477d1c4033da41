"""Address-range cases: one row per kernel family, and the layouts that put it at its limits
(tests/test_span_host.py, tests/test_span_gpu.py).  Test infrastructure only.

A launcher accepts a layout when the row strides and the SPANS -- bytes from the first byte of the source window
(destination band) to the last byte touched, (rows - 1) * stride + row bytes -- stay within its family's limits
(csrc/kernels.hpp layout_limits, include/iqo_hip.h "Layout limits").  A row here names a shape that reaches the
family and body, the options that get it there, and the family's four limits as LITERALS (largest accepted
value, 0 = unlimited): the host test holds them against libiqo_amd.host_layout_limits.  The layouts are
functions of those literals:

  tight     the control
  src_top   the largest accepted source layout: the largest 16-byte-multiple row stride for which stride and
            span are both accepted (unlimited families: the stride that puts the last row beyond 2^32)
  dst_top   the same for the destination
  over      the smallest rejected layouts, one 16-byte step past a limit: source span, destination span (whole
            frame), source stride, destination stride (a band of ONE output row, so that only the stride is
            over and the buffers still cover every byte the layout names)
  far       3 frames, source frame stride 2^31 + 4096, destination frame stride 2^31 + 8192
  band      the whole frame's spans over the limit, a band of 16 output rows under it (BAND rows only)

Calls with several frames and a top row stride interleave the frames inside the row stride (frame stride = the
row bytes rounded up to 16), so that every layout fits buffers of BUF bytes.
"""
import collections
import functools

import numpy as np

import extreme_cases as ec
import instance_cases as ic
import oracle_lib as ol

DROP = 0x7ff00000                    # iqo_hip.h IQO_HIP_DROP_OFFSET: the offset that drops an access
BUF = 2 ** 32 + 2 ** 25              # bytes of the GPU test's source buffer and of its destination buffer
FAR_SRC, FAR_DST = 2 ** 31 + 4096, 2 ** 31 + 8192
BAND_ROWS = 16

# the four limits (srcSpanMax, dstSpanMax, srcStMax, dstStMax) by family, written out
UNLIMITED = (0, 0, 0, 0)
TILE = (2147483647, 2147483647, 16777215, 2147483647)
STREAM = (2146435071, 2146435071, 2146435071, 2146435071)
WALK = (2146435071, 2146435071, 16777215, 2146435071)
RATIO = (2146435071, 2146435071, 16777215, 16777215)
# iqo_hip_resize_device_norm's own documented limits, whichever packed kernel runs: source frame and float
# frame below 2^31, srcSt below 2^24, float row stride below 2^31
NORM = (2147483647, 2147483647, 16777215, 2147483647)

# families whose dropped accesses include a store or a load whose value is used
SENTINEL_FAMILIES = ("lanczos_stream", "linear_up2", "walk", "lanczos_up2", "lanczos_d32", "lanczos_d31", "lanczos_u23",
                     "linear_u23", "area_d32", "ryx", "ryg")

# name: the case id.  kernel: libiqo_amd.KERNELS name.  inst: the instantiation's parameters where the family has
# more than one (host_instance_for's form), the streamer body for lanczos_stream (stream_body below), else None.
# frames: frames per call of every layout but `far`.  norm: through resize_normalized (fp32) instead of bytes.
Row = collections.namedtuple("Row", "name kernel inst method d sw sh dw dh px C options frames norm limits note")


def _r(name, kernel, inst, method, d, sw, sh, dw, dh, px=1, C=1, options=(), frames=None, norm=False, limits=None,
       note=""):
    if frames is None:
        frames = 2 if method == "lanczos" and C == 1 else 1
    return Row(name, kernel, inst, method, d, sw, sh, dw, dh, px, C, tuple(options), frames, norm, limits, note)


_PK = ("lanczos", 3, 64, 140, 32, 131)
ROWS = [
    # ---- the four Lanczos 2:1 streamer bodies and the frame-stacked one
    _r("symb-1wave", "lanczos_stream", "symb", "lanczos", 3, 384, 264, 192, 132, limits=STREAM),
    _r("symb-4waves", "lanczos_stream", "symb", "lanczos", 3, 3008, 264, 1504, 132, limits=STREAM),
    _r("ring-px2", "lanczos_stream", "ring", "lanczos", 3, 384, 264, 192, 132, px=2, limits=STREAM),
    _r("sym-perwave", "lanczos_stream", "sym", "lanczos", 3, 384, 264, 192, 132, options=(("stream_variant", 2),),
       limits=STREAM),
    _r("stack-5frames", "lanczos_stream", "stack", "lanczos", 2, 208, 264, 104, 132, frames=5, limits=STREAM),
    # ---- area_int: an even KX, KX = 3, Linear 2:1 (linear_d2_body)
    _r("area-2x2", "area_int", None, "area", 0, 384, 264, 192, 132, limits=UNLIMITED),
    _r("area-3x3", "area_int", None, "area", 0, 96, 390, 32, 130, limits=UNLIMITED),
    _r("linear-d2", "area_int", None, "linear", 0, 384, 264, 192, 132, limits=UNLIMITED),
    # ---- linear_up2
    _r("linear-up2", "linear_up2", None, "linear", 0, 192, 132, 384, 264, limits=STREAM),
    _r("linear-up3", "linear_up2", None, "linear", 0, 64, 132, 192, 396, limits=STREAM),
    # ---- general ratios
    _r("tile", "tile", {"LZ": 1, "NP": 6}, "lanczos", 3, 200, 140, 137, 131, options=ic.TILE_ONLY, limits=TILE),
    _r("walk", "walk", {"LZ": 1, "NP": 6, "VY": 10, "NV": 1}, "lanczos", 5, 200, 140, 300, 200, limits=WALK),
    _r("general", "general", None, "lanczos", 3, 40, 140, 24, 131, options=(("force_general", 1),), limits=UNLIMITED),
    # ---- exact ratios
    _r("lanczos_up2", "lanczos_up2", {"NT": 6, "F": 2}, "lanczos", 3, 192, 132, 384, 264, limits=RATIO),
    _r("lanczos_d32", "lanczos_d32", {"PD": 1}, "lanczos", 3, 384, 216, 256, 144, limits=RATIO),
    _r("lanczos_d31", "lanczos_d31", {"PD": 1}, "lanczos", 3, 384, 390, 128, 130, limits=RATIO),
    _r("lanczos_u23", "lanczos_u23", {"PD": 1}, "lanczos", 3, 256, 144, 384, 216, limits=RATIO),
    _r("linear_u23", "linear_u23", {"PD": 2}, "linear", 0, 256, 144, 384, 216, limits=RATIO),
    _r("area_d32", "area_d32", {"PD": 4}, "area", 0, 384, 216, 256, 144, limits=RATIO),
    # ---- ratio rows
    _r("ryx", "ryx", {"LZ": 1, "P": 4, "Q": 9, "T": 6, "NP": 4, "PD": 2, "CPT": 4}, "lanczos", 3, 160, 144, 360, 324,
       limits=RATIO),
    _r("ryg", "ryg", {"LZ": 1, "T": 12, "NP": 7, "PD": 4, "CPT": 3, "NL": 2}, "lanczos", 4, 200, 200, 137, 133,
       limits=RATIO),
    _r("ryu", "ryu", {"T": 6, "NP": 4, "PD": 3, "CPT": 4, "KM": 3}, "lanczos", 3, 240, 136, 500, 275, px=2, limits=RATIO),
    # ---- packed, C = 3: bytes and normalised fp32 planes
    _r("packed_tile", "packed_tile", None, *_PK, C=3, limits=TILE),
    _r("packed_tile-norm", "packed_tile", None, *_PK, C=3, norm=True, limits=NORM),
    _r("packed_general", "packed_general", None, *_PK, C=3, options=(("force_general", 1),), limits=UNLIMITED),
    _r("packed_general-norm", "packed_general", None, *_PK, C=3, options=(("force_general", 1),), norm=True, limits=NORM,
       note="iqo_hip_resize_device_norm limits the float frame whichever kernel runs"),
]
BY_NAME = {r.name: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
BAND = ("symb-1wave", "ryx")


def rid(row):
    return row.name


# ----------------------------------------------------------------------------- the streamer bodies, restated

def stream_body(row, frames):
    """Which lanczos_stream body kernels.hip prep_lanczos picks: "ring" (no symmetric table, or stream_variant 1),
    "sym" (per-wave symmetric), "symb" (block-shared), "stack" (several narrow frames per workgroup), and the
    block-shared body's waves per row."""
    import libiqo_amd
    opt = dict(row.options)
    taps_y = len(libiqo_amd.host_tables(row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px, 1)[0])
    variant = opt.get("stream_variant", 0)
    if taps_y == 4 or variant == 1:
        return "ring", 0
    lanes = (row.dw + 7) // 8
    wpr = (row.dw + 495) // 496
    np_ = min((lanes + wpr - 1) // wpr, row.dw // 8)
    wpr = (row.dw + 8 * np_ - 1) // (8 * np_)
    need = (max(32 + 2 * row.dw, 16 + row.sw) + 15) & ~15
    chunks = (need - 16 + 1023) // 1024
    cpw = (chunks + wpr - 1) // wpr
    if variant == 2 or wpr > 4 or cpw > 2:
        return "sym", wpr
    npf = row.sw // 16
    fpw_max = min(6, 125 // (npf + 1)) if npf else 0
    if (taps_y <= 10 and wpr == 1 and row.sw == 2 * row.dw and row.sw % 16 == 0 and np_ == npf and fpw_max >= 4
            and frames >= 2):
        return "stack", wpr
    return "symb", wpr


# ----------------------------------------------------------------------------- layouts

Layout = collections.namedtuple("Layout", "frames src_st src_fst dst_st dst_fst r0 rows s0 srows")


def a16(n):
    return (n + 15) & ~15


def elem(row):
    return 4 if row.norm else 1


def row_bytes(row):
    """(source, destination) bytes of one row as the span counts them (the walker's source row: whole dwords;
    a normalised row: one plane's floats)."""
    s = row.sw * row.C
    if row.kernel == "walk":
        s = (s + 3) & ~3
    return s, row.dw * (4 if row.norm else row.C)


def window(row, r0=0, rows=None):
    """(first source row, source rows) of output rows [r0, r0 + rows): the window a call passes, from row 0 of the
    frame for a whole-frame call."""
    import libiqo_amd
    rows = row.dh if rows is None else rows
    s0, n = libiqo_amd.host_band_src_rows(row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px, r0, rows)
    return (0, s0 + n) if (r0, rows) == (0, row.dh) else (s0, n)


def span(rows, stride, rb, planes=1, plane_st=0):
    return (planes - 1) * plane_st + (rows - 1) * stride + rb


def norm_dst_rows(row):
    """A float frame's rows, first to last: 3 planes of dh rows, plane stride dh * row stride."""
    return 3 * row.dh if row.norm else row.dh


def top_stride(rows, rb, span_max, st_max):
    """The largest 16-byte-multiple stride with stride and span accepted; unlimited: the smallest that puts the
    last row at or beyond 2^32."""
    if not span_max:
        return a16(-(-2 ** 32 // (rows - 1)))
    st = st_max // 16 * 16
    if rows > 1:
        st = min(st, (span_max - rb) // (rows - 1) // 16 * 16)
    return st


def tight(row, frames=None):
    frames = row.frames if frames is None else frames
    sst, dst = a16(row.sw * row.C), a16(row.dw * row.C * elem(row))
    return Layout(frames, sst, row.sh * sst, dst, norm_dst_rows(row) * dst, 0, row.dh, *window(row))


def src_top(row):
    t = tight(row)
    st = top_stride(t.srows, row_bytes(row)[0], row.limits[0], row.limits[2])
    return t._replace(src_st=st, src_fst=a16(row_bytes(row)[0]))


def dst_top(row):
    t = tight(row)
    st = top_stride(norm_dst_rows(row), row_bytes(row)[1], row.limits[1], row.limits[3])
    return t._replace(dst_st=st, dst_fst=a16(row_bytes(row)[1]))


def far(row):
    return tight(row, 3)._replace(src_fst=FAR_SRC, dst_fst=FAR_DST)


def fits(row, lay):
    """Whether every byte the layout names lies inside buffers of BUF bytes."""
    sb, db = row_bytes(row)
    s = (lay.frames - 1) * lay.src_fst + lay.s0 * lay.src_st + span(lay.srows, lay.src_st, sb)
    rows = 3 * lay.rows if row.norm else lay.rows
    d = (lay.frames - 1) * lay.dst_fst + lay.r0 * lay.dst_st + span(rows, lay.dst_st, db)
    return s <= BUF and d <= BUF


def over(row):
    """{which: layout} of the smallest rejected layouts that fit the buffers; {} for an unlimited family.
    Span cases are whole frames; stride cases a band of one output row (normalised rows have no band entry, and
    in a whole frame a stride over its limit is a span over its limit: span cases only)."""
    smax, dmax, sst_max, dst_max = row.limits
    if not smax:
        return {}
    out = {}
    t = tight(row, 1)
    sb, db = row_bytes(row)
    st = (smax - sb) // (t.srows - 1) // 16 * 16 + 16
    if st <= sst_max:
        out["src_span"] = t._replace(src_st=st)
    st = (dmax - db) // (norm_dst_rows(row) - 1) // 16 * 16 + 16
    if st <= dst_max:
        out["dst_span"] = t._replace(dst_st=st)
    if not row.norm:
        one = t._replace(r0=0, rows=1, **dict(zip(("s0", "srows"), window(row, 0, 1))))
        # (only where the stride alone is over: with a stride limit as high as the span limit, a window of two
        # rows is over its span first, and the span cases have that)
        if accepted(row, one._replace(src_st=sst_max // 16 * 16)):
            out["src_stride"] = one._replace(src_st=sst_max // 16 * 16 + 16)
        out["dst_stride"] = one._replace(dst_st=dst_max // 16 * 16 + 16)
    return {k: v for k, v in out.items() if fits(row, v)}


def band(row):
    """(frame row strides over the limit, the band's layout): output rows [r0, r0 + 16) in the middle of a frame whose
    whole spans are one step over both limits."""
    o = over(row)
    sst, dst = o["src_span"].src_st, o["dst_span"].dst_st
    r0 = row.dh // 2 // 9 * 9  # (a multiple of every row group the exact-ratio rows use)
    s0, n = window(row, r0, BAND_ROWS)
    return Layout(1, sst, 0, dst, 0, r0, BAND_ROWS, s0, n)


def accepted(row, lay):
    """The limits' arithmetic on a layout, as csrc/kernels.hpp layout_ok does it."""
    smax, dmax, sst_max, dst_max = row.limits
    if not smax:
        return True
    sb, db = row_bytes(row)
    rows = 3 * lay.rows if row.norm else lay.rows
    return (lay.src_st <= sst_max and lay.dst_st <= dst_max and span(lay.srows, lay.src_st, sb) <= smax and
            span(rows, lay.dst_st, db) <= dmax)


# ----------------------------------------------------------------------------- frames and answers

@functools.lru_cache(maxsize=None)
def planes(method, d, sw, sh, dw, dh, px, n, seed=77):
    """(frames [n, sh, sw], expected [n, dh, dw]), read-only: a noise frame, then for Lanczos the tap-sign frames of
    tests/extreme_cases.py in their order, for Area / Linear more noise."""
    if method == "lanczos":
        fr = ec.plane_frames(d, sw, sh, dw, dh, px, False, seed)[1][:n]
    else:
        fr = np.stack([ol.gen("noise", sw, sh, seed + 13 * i) for i in range(n)])
    assert fr.shape[0] == n
    exp = np.stack([ol.run_oracle(method, d, sw, sh, dw, dh, px, f) for f in fr])
    fr.setflags(write=False)
    exp.setflags(write=False)
    return fr, exp


@functools.lru_cache(maxsize=None)
def far_planes(method, d, sw, sh, dw, dh, px, n):
    """n noise frames of different seeds and their answers."""
    fr = np.stack([ol.gen("noise", sw, sh, 1000 + 7 * i) for i in range(n)])
    exp = np.stack([ol.run_oracle(method, d, sw, sh, dw, dh, px, f) for f in fr])
    fr.setflags(write=False)
    exp.setflags(write=False)
    return fr, exp


def frames_of(row, n, is_far=False):
    """(source [n, sh, sw] or [n, sh, sw, C], expected bytes of the same form): a packed pixel's channels carry
    different planes."""
    shape = (row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px)
    fr, exp = (far_planes if is_far else planes)(*shape, n + row.C - 1)
    if row.C == 1:
        return fr, exp
    idx = [[f + c for c in range(row.C)] for f in range(n)]
    return (np.stack([np.stack([fr[i] for i in r], axis=2) for r in idx]),
            np.stack([np.stack([exp[i] for i in r], axis=2) for r in idx]))
