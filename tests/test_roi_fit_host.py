"""Boxes into destination rectangles (iqo_hip_resize_rois_fit_*_device, iqo_hip_resize_rois_yuv_fit_*_device), the
part that needs no GPU: the CPU twins, which build the fit arenas as the device calls do and walk them with the
kernels' formulas, against the oracle canvas of tests/roi_fit_cases.py; the pinned rectangle rule; every rejection;
strides; the arena statistics; and a sanitizer build of the arena code in a stand-alone program.
"""
import os
import shutil
import subprocess

import numpy as np
import pytest

import libiqo_amd
import norm_cases as nc
import roi_cases as rc
import roi_fit_cases as fc
import roi_yuv_cases as ryc
import yuvrgb_cases as yr

EINVAL, EUNSUP = ryc.EINVAL, ryc.EUNSUP
METHOD_IDS = ["%s%d" % m for m in fc.METHODS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H = fc.CW, fc.CH


def _host(method, degree, C, **kw):
    boxes, rects = fc.cases(method, degree)
    kw.setdefault("rects", rects)
    kw.setdefault("pad", fc.PAD)
    return libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(C), boxes, **kw)


def _host_yuv(method, degree, layout, **kw):
    boxes, rects = fc.cases(method, degree, True)
    kw.setdefault("rects", rects)
    kw.setdefault("pad", fc.PAD[:3])
    kw.setdefault("standard", ryc.STANDARD[(method, degree)])
    return libiqo_amd.host_resize_rois_yuv(method, degree, W, H, ryc.frames(layout), boxes, ryc.FW, ryc.FH, layout=layout, **kw)


def test_case_lists():
    """Every rectangle of the list is in some method's list: all twelve packed cases for every method; of the YUV cases
    Area takes all, Lanczos all but the two single-row rectangles, Linear all but the three above 2x in chroma."""
    for m in fc.METHODS:
        assert len(fc.cases(*m)[0]) == len(fc.CASES)
        assert len(fc.cases(*m, True)[0]) == len(fc.YUV_CASES) - {"area": 0, "lanczos": 2, "linear": 3}[m[0]]
    for (b, r), (yb, yr_) in zip(fc.CASES, fc.YUV_CASES):
        assert r == yr_ and not any(v & 1 for v in yb[1:5])
        assert b[1] + b[3] <= rc.FW and b[2] + b[4] <= rc.FH and yb[1] + yb[3] <= rc.FW and yb[2] + yb[4] <= rc.FH
        assert r[0] + r[2] <= W and r[1] + r[3] <= H
    # and the library lays every list out: one fit record per box, bands and pad workgroups
    for m in fc.METHODS:
        boxes, rects = fc.cases(*m)
        st = libiqo_amd.host_roi_arena_stats(m[0], m[1], W, H, 3, boxes, rc.FRAMES, rc.FW, rc.FH, rects=rects)
        none = libiqo_amd.host_roi_arena_stats(m[0], m[1], W, H, 3, [], rc.FRAMES, rc.FW, rc.FH, rects=[])
        assert st["record_bytes"] == 96 and none["workgroups"] == 0
        assert st["arena_bytes"] > none["arena_bytes"] + len(boxes) * 96
        lays = [libiqo_amd.host_roi_fit_box_layout(m[0], m[1], 3, W, H, b[3], b[4], r) for b, r in zip(boxes, rects)]
        assert st["workgroups"] == sum(l["pad_above"] + l["workgroups"] + l["pad_below"] for l in lays)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("method,degree", fc.METHODS, ids=METHOD_IDS)
def test_host_equals_oracle(method, degree, C):
    fc.same(_host(method, degree, C), fc.expected(method, degree, C), "%s-%d C=%d" % (method, degree, C))


@pytest.mark.parametrize("layout", ryc.LAYOUTS)
@pytest.mark.parametrize("method,degree", fc.METHODS, ids=METHOD_IDS)
def test_host_yuv_equals_oracle(method, degree, layout):
    exp = fc.expected_yuv(method, degree, ryc.STANDARD[(method, degree)])
    for order, o4 in yr.ORDERS.items():
        fc.same(_host_yuv(method, degree, layout, order=order), yr.reorder(exp, o4), "%s-%d %s %s" % (method, degree, layout, order))


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_host_norm_equals_numpy(dtype):
    """byte * scale + bias of the padded U8 canvas, pad included."""
    method, degree = "lanczos", 3
    for C, order in ((3, (2, 0, 1)), (1, (0, 0, 0)), (4, (3, 1))):
        scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
        got = _host(method, degree, C, scale=scale, bias=bias, dtype=dtype, order=order)
        u8 = fc.expected(method, degree, C)
        exp = nc.expected_bits(u8[..., None] if C == 1 else u8, order, scale, bias, dtype)
        fc.same(got.view(exp.dtype), exp, "norm C=%d %s" % (C, dtype))
    for layout in ryc.LAYOUTS:
        planes, scale, bias = (2, 0, 1), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
        got = _host_yuv(method, degree, layout, scale=scale, bias=bias, dtype=dtype, planes=planes)
        exp = nc.expected_bits(fc.expected_yuv(method, degree, ryc.STANDARD[(method, degree)]), planes, scale, bias, dtype)
        fc.same(got.view(exp.dtype), exp, "norm %s %s" % (layout, dtype))


@pytest.mark.parametrize("method,degree", fc.METHODS, ids=METHOD_IDS)
def test_no_rects_equals_stretch(method, degree):
    """rects=None: every rectangle is the whole output, byte for byte the stretch twin's (the pad is written nowhere)."""
    boxes = rc.boxes(method, degree)
    for C in rc.CHANNELS:
        src = rc.frames(C)
        fit = libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, src, boxes, pad=9)  # (pad != 0: the fit twin)
        fc.same(fit, libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, src, boxes), "packed C=%d" % C)
    yb = ryc.boxes(method, degree)
    for layout in ryc.LAYOUTS:
        args = (method, degree, ryc.DW, ryc.DH, ryc.frames(layout), yb, ryc.FW, ryc.FH)
        fc.same(libiqo_amd.host_resize_rois_yuv(*args, layout=layout, pad=(1, 2, 3)),
                libiqo_amd.host_resize_rois_yuv(*args, layout=layout), "yuv " + layout)
        fc.same(libiqo_amd.host_resize_rois_yuv(*args, layout=layout, pad=(0, 0, 9), scale=(1, 1, 1), bias=(0, 0, 0)),
                libiqo_amd.host_resize_rois_yuv(*args, layout=layout, scale=(1, 1, 1), bias=(0, 0, 0)), "yuv norm " + layout)


def _rule(w, h, dw, dh, centred):
    if w * dh >= h * dw:
        iw, ih = dw, max(1, (h * dw + w // 2) // w)
    else:
        iw, ih = max(1, (w * dh + h // 2) // h), dh
    return ((dw - iw) // 2, (dh - ih) // 2, iw, ih) if centred else (0, 0, iw, ih)


@pytest.mark.parametrize("dw,dh", [(48, 40), (40, 48)])
def test_fit_rects_rule(dw, dh):
    boxes = [(0, 0, 0, w, h) for w in range(1, 65) for h in range(1, 65)]
    for mode, centred in (("letterbox", True), ("letterbox-topleft", False)):
        got = libiqo_amd.fit_rects(boxes, dw, dh, mode)
        assert got == [_rule(b[3], b[4], dw, dh, centred) for b in boxes]
        for x, y, iw, ih in got:
            assert x >= 0 and y >= 0 and iw >= 1 and ih >= 1 and x + iw <= dw and y + ih <= dh
            assert iw == dw or ih == dh     # touches two opposite sides
    assert libiqo_amd.fit_rects(boxes[:3], dw, dh, "stretch") == [(0, 0, dw, dh)] * 3
    big = [(0, 0, 0, 1 << 24, 1), (0, 0, 0, 1, 1 << 24), (0, 0, 0, 1 << 24, (1 << 24) - 1)]
    assert libiqo_amd.fit_rects(big, 1 << 20, 1 << 20) == [_rule(b[3], b[4], 1 << 20, 1 << 20, True) for b in big]
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.fit_rects([(0, 0, 0, 0, 5)], dw, dh)
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.fit_rects(boxes[:1], dw, dh, "cover")


def test_fit_keyword_is_fit_rects():
    method, degree = "area", 0
    boxes = [(0, 2, 4, 64, 36), (1, 0, 0, 30, 90, 1), (2, 10, 10, 48, 40)]
    for mode in ("letterbox", "letterbox-topleft"):
        rects = libiqo_amd.fit_rects(boxes, W, H, mode)
        a = libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, fit=mode, pad=(1, 2, 3))
        b = libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, rects=rects, pad=(1, 2, 3))
        fc.same(a, b, mode)
        assert (a[0, 0, 0] == (1, 2, 3)).all() or rects[0][1] == 0
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, fit="letterbox", rects=rects)
    for kw in ({"fit": "stretch"}, {"fit": "cover"}, {"pad": 256}, {"pad": (1, 2, 3, 4, 5)}, {"pad": 1.5}, {"pad": (1, "x")}):
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, **kw)
    c = libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, fit="letterbox", pad=np.uint8(7))
    d = libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(3), boxes, fit="letterbox", pad=np.array([7, 7, 7]))
    fc.same(c, d, "numpy pads")


GOOD, GOODR = (0, 0, 0, 64, 48), (0, 0, 48, 40)
# (method, degree, boxes, rects, status, bad box)
REJECTED = (
    ("area", 0, [GOOD, GOOD], [GOODR, (1, 0, 48, 40)], EINVAL, 1),         # past the right edge
    ("area", 0, [GOOD, GOOD], [GOODR, (0, 1, 48, 40)], EINVAL, 1),         # past the bottom
    ("area", 0, [GOOD], [(-1, 0, 10, 10)], EINVAL, 0),
    ("area", 0, [GOOD], [(0, -1, 10, 10)], EINVAL, 0),
    ("area", 0, [GOOD, GOOD, GOOD], [GOODR, GOODR, (0, 0, 0, 10)], EINVAL, 2),  # iw < 1
    ("area", 0, [GOOD], [(0, 0, 10, 0)], EINVAL, 0),                       # ih < 1
    ("lanczos", 3, [GOOD, (0, 4, 4, 10, 1)], [GOODR, (0, 0, 10, 24)], EINVAL, 1),   # Lanczos rows undefined for 1 -> 24
    ("area", 0, [GOOD, (0, 0, 0, 160, 120)], [GOODR, (0, 0, 1, 40)], EUNSUP, 1),    # 160 taps > IQO_HIP_ROI_MAX_TAPS
)


@pytest.mark.parametrize("row", REJECTED, ids=[str(i) for i in range(len(REJECTED))])
def test_rejections(row):
    method, degree, boxes, rects, status, bad = row
    for kw in ({}, {"scale": (1.0,), "bias": (0.0,)}):
        with pytest.raises(libiqo_amd.IqoError) as e:
            libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(1), boxes, rects=rects, **kw)
        assert (e.value.status, e.value.bad_roi) == (status, bad)
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.host_roi_arena_stats(method, degree, W, H, 1, boxes, rc.FRAMES, rc.FW, rc.FH, rects=rects)
    assert (e.value.status, e.value.bad_roi) == (status, bad)


def test_rejections_yuv_and_lds():
    # (packed Linear above 2x: the stretch call accepts it unpinned, tests/test_roi_host.py, and so does the fit call)
    libiqo_amd.host_resize_rois("linear", 0, W, H, rc.frames(1), [(0, 0, 0, 20, 13)], rects=[(0, 0, 41, 27)])
    frames = ryc.frames("nv12")
    good = (0, 0, 0, 64, 48)

    def call(method, degree, boxes, rects, **kw):
        return libiqo_amd.host_resize_rois_yuv(method, degree, W, H, frames, boxes, ryc.FW, ryc.FH, rects=rects, **kw)
    for method, degree, boxes, rects, status, bad in (
            ("area", 0, [good, good], [GOODR, (40, 0, 9, 40)], EINVAL, 1),
            ("area", 0, [good], [(0, 0, 48, 0)], EINVAL, 0),
            ("linear", 0, [good, (0, 0, 0, 20, 14)], [GOODR, (0, 0, 21, 14)], EUNSUP, 1),   # chroma above 2x
            ("lanczos", 3, [good, (0, 0, 0, 16, 2)], [GOODR, (0, 0, 16, 24)], EINVAL, 1),   # chroma rows 1 -> 24
            ("area", 0, [good, (0, 0, 0, 160, 120)], [GOODR, (0, 0, 1, 40)], EUNSUP, 1)):   # 160 taps
        for kw in ({}, {"scale": (1, 1, 1), "bias": (0, 0, 0)}):
            with pytest.raises(libiqo_amd.IqoError) as e:
                call(method, degree, boxes, rects, **kw)
            assert (e.value.status, e.value.bad_roi) == (status, bad), (method, rects)
    # a band row over IQO_HIP_ROI_LDS_BYTES: a box 9000 wide at 4 channels (the stretch call's limit, by (iw, ih))
    wide = [(0, 0, 0, 16, 16), (0, 0, 0, 9000, 2)]
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.host_roi_arena_stats("area", 0, 9000, 8, 4, wide, 1, 9000, 16, rects=[(0, 0, 16, 8), (0, 2, 9000, 2)])
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, 1)
    with pytest.raises(libiqo_amd.IqoError) as e:  # and one rectangle per box
        libiqo_amd.host_roi_arena_stats("area", 0, W, H, 1, [GOOD, GOOD], 3, rc.FW, rc.FH, rects=[GOODR])
    assert not hasattr(e.value, "status")


def test_strides_and_sentinels():
    """Canvases inside a larger buffer: the twin writes the canvas and nothing else."""
    method, degree = "area", 0
    boxes, rects = fc.cases(method, degree)
    N = len(boxes)
    for C in (3, 4):
        big = np.full((N, H + 3, W + 5, C), 0xA5, np.uint8)
        out = big[:, :H, :W]
        res = libiqo_amd.host_resize_rois(method, degree, W, H, rc.frames(C), boxes, rects=rects, pad=fc.PAD, out=out)
        assert res is out
        fc.same(np.ascontiguousarray(out), fc.expected(method, degree, C), "strided C=%d" % C)
        mask = np.ones(big.shape, bool)
        mask[:, :H, :W] = False
        assert (big[mask] == 0xA5).all()
    yb, yrects = fc.cases(method, degree, True)
    bigf = np.full((len(yb), 3, H + 2, W + 3), np.float32(-7.5), np.float32)
    outf = bigf[:, :, :H, :W]
    libiqo_amd.host_resize_rois_yuv(method, degree, W, H, ryc.frames("i420"), yb, ryc.FW, ryc.FH, layout="i420",
                                    standard=ryc.STANDARD[(method, degree)], scale=nc.NORM_SCALE[:3],
                                    bias=nc.NORM_BIAS[:3], out=outf, rects=yrects, pad=fc.PAD[:3])
    exp = nc.expected_bits(fc.expected_yuv(method, degree, ryc.STANDARD[(method, degree)]), (0, 1, 2), nc.NORM_SCALE[:3],
                           nc.NORM_BIAS[:3], "float32")
    fc.same(np.ascontiguousarray(outf).view(np.int32), exp, "norm strided")
    maskf = np.ones(bigf.shape, bool)
    maskf[:, :, :H, :W] = False
    assert (bigf[maskf] == np.float32(-7.5)).all()


def test_arena_stats_show_table_sharing():
    """Tables are keyed by (source length, output length): two boxes of one width to two iw have two X tables, to one
    iw one; the fit records have sizes of their own, and the stretch arenas keep theirs."""
    def st(boxes, rects, **kw):
        return libiqo_amd.host_roi_arena_stats("lanczos", 3, W, H, 3, boxes, rc.FRAMES, rc.FW, rc.FH, rects=rects, **kw)
    a, b, c = (1, 2, 5, 45, 31), (0, 40, 2, 45, 50), (0, 9, 60, 45, 40)
    one = st([a], [(5, 7, 31, 19)])
    assert (one["x_tables"], one["y_tables"], one["record_bytes"]) == (1, 1, 96)
    two_iw = st([a, b], [(5, 7, 31, 19), (2, 3, 20, 30)])
    assert (two_iw["x_tables"], two_iw["y_tables"]) == (2, 2)
    same_iw = st([a, c], [(5, 7, 31, 19), (10, 0, 31, 33)])
    assert (same_iw["x_tables"], same_iw["y_tables"]) == (1, 2)
    assert same_iw["arena_bytes"] < two_iw["arena_bytes"]
    twice = st([a, a], [(5, 7, 31, 19), (9, 7, 31, 19)])
    assert (twice["x_tables"], twice["y_tables"]) == (1, 1)
    assert twice["arena_bytes"] == one["arena_bytes"] + 96 and twice["workgroups"] == 2 * one["workgroups"]
    # workgroups: pad above, bands, pad below, as the layout query says
    lay = libiqo_amd.host_roi_fit_box_layout("lanczos", 3, 3, W, H, 45, 31, (5, 7, 31, 19))
    assert one["workgroups"] == lay["pad_above"] + lay["workgroups"] + lay["pad_below"]
    assert (lay["pad_above"], lay["pad_below"]) == (1, 1) and lay["workgroups"] == -(-19 // lay["rows"])
    stretch = libiqo_amd.host_roi_box_layout("lanczos", 3, 3, 31, 19, 45, 31)
    assert {k: lay[k] for k in stretch} == stretch
    # YUV: 128 bytes a record; luma and chroma tables by (length, output length)
    y = libiqo_amd.host_roi_yuv_arena_stats("area", 0, W, H, "nv12", [(0, 0, 0, 64, 48), (0, 0, 0, 64, 48)], 3, ryc.FW, ryc.FH,
                                            rects=[(0, 0, 48, 40), (0, 0, 24, 20)])
    assert (y["record_bytes"], y["x_tables"], y["y_tables"]) == (128, 4, 4)
    ylay = libiqo_amd.host_roi_yuv_fit_box_layout("area", 0, "nv12", W, H, 64, 48, (0, 0, 24, 20))
    assert ylay == dict(libiqo_amd.host_roi_yuv_box_layout("area", 0, "nv12", 24, 20, 64, 48), pad_above=0, pad_below=1,
                        pad_rows=ylay["pad_rows"])
    # the stretch arenas are what they were
    s = libiqo_amd.host_roi_arena_stats("lanczos", 3, W, H, 3, [a], rc.FRAMES, rc.FW, rc.FH)
    assert s["record_bytes"] == 64
    assert libiqo_amd.host_roi_yuv_arena_stats("area", 0, W, H, "nv12", [(0, 0, 0, 64, 48)], 3, ryc.FW, ryc.FH)["record_bytes"] == 96


def test_pad_workgroups_have_a_bounded_share():
    """No workgroup writes a whole border: 140 rows above a rectangle of a 640 x 640 canvas are several workgroups'."""
    lay = libiqo_amd.host_roi_yuv_fit_box_layout("area", 0, "nv12", 640, 640, 1920, 1080, (0, 140, 640, 360))
    assert 1 <= lay["pad_rows"] < 140
    assert lay["pad_above"] == -(-140 // lay["pad_rows"]) >= 2 and lay["pad_below"] == -(-140 // lay["pad_rows"])
    tall = libiqo_amd.host_roi_fit_box_layout("area", 0, 1, 8, 600, 16, 40, (0, 290, 8, 20))
    assert tall["pad_above"] >= 3 and tall["pad_above"] == -(-290 // tall["pad_rows"]) == tall["pad_below"]


def test_arena_walk_under_sanitizers(tmp_path):
    """tests/native/roi_fit_walk.cpp: the layout, fill and twin of the case list and of 4097 tiny boxes, both formats, in
    a stand-alone program built with -fsanitize=address,undefined and run directly."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "roi_fit_walk")
    csrc = os.path.join(ROOT, "libiqo_amd", "csrc")
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *static, "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "roi_fit_walk.cpp"), os.path.join(csrc, "roi.cpp"),
                           os.path.join(csrc, "plan.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "roi_fit_walk ok" in r.stdout
