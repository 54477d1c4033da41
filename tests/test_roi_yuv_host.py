"""Crop-and-resize of NV12 / I420 boxes straight to RGB (iqo_hip_resize_rois_yuv_*_device), the part that needs no
GPU: the CPU twin (iqo_host_resize_rois_yuv_rgb / _norm), which builds the call's arena as the device call does and
walks it with the kernel's formulas, against the Generic oracle per component and the integer matrix; strides; the
arena statistics; every rejection; and a sanitizer build of the arena code in a stand-alone program.
"""
import ctypes
import os
import shutil
import subprocess

import numpy as np
import pytest

import libiqo_amd
import norm_cases as nc
import roi_yuv_cases as rc
import yuvrgb_cases as yr

EINVAL, EUNSUP = rc.EINVAL, rc.EUNSUP
METHOD_IDS = ["%s%d" % m for m in rc.METHODS]
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host(method, degree, layout, boxes, **kw):
    kw.setdefault("standard", rc.STANDARD[(method, degree)])
    return libiqo_amd.host_resize_rois_yuv(method, degree, rc.DW, rc.DH, rc.frames(layout), boxes, rc.FW, rc.FH,
                                           layout=layout, **kw)


def test_case_lists():
    """All 13 boxes for Lanczos-2, -3 and Area; Lanczos-5 without the 4 x 4 box; Linear without the last three; and
    the library lays every list out: one record per box, at least one workgroup each."""
    for m in (("lanczos", 2), ("lanczos", 3), ("area", 0)):
        assert rc.boxes(*m) == rc.BOXES
    assert len(rc.BOXES) == 13
    assert set(rc.BOXES) - set(rc.boxes("lanczos", 5)) <= {rc.BOXES[10]}
    assert set(rc.BOXES) - set(rc.boxes("linear", 0)) <= set(rc.BOXES[10:])
    for b in rc.BOXES:
        assert not any(v & 1 for v in b[1:5]) and b[1] + b[3] <= rc.FW and b[2] + b[4] <= rc.FH
    assert sorted(set(rc.STANDARD.values())) == yr.STANDARDS
    for method, degree in rc.METHODS:
        boxes = list(rc.boxes(method, degree))
        for layout in rc.LAYOUTS:
            st = libiqo_amd.host_roi_yuv_arena_stats(method, degree, rc.DW, rc.DH, layout, boxes, rc.FRAMES, rc.FW, rc.FH)
            none = libiqo_amd.host_roi_yuv_arena_stats(method, degree, rc.DW, rc.DH, layout, [], rc.FRAMES, rc.FW, rc.FH)
            assert st["workgroups"] >= len(boxes) and none["workgroups"] == 0
            assert st["arena_bytes"] > none["arena_bytes"] + len(boxes) * st["record_bytes"]  # (and its tables)


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_host_equals_oracle(method, degree, layout):
    boxes = rc.boxes(method, degree)
    exp = rc.expected(method, degree)
    for order, o4 in yr.ORDERS.items():
        got = _host(method, degree, layout, boxes, order=order)
        rc.same(got, yr.reorder(exp, o4), "%s-%d %s %s" % (method, degree, layout, order))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_host_norm_equals_numpy(layout, dtype):
    method, degree, planes = "lanczos", 3, (2, 0, 1)
    scale, bias = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
    got = _host(method, degree, layout, rc.boxes(method, degree), scale=scale, bias=bias, dtype=dtype, planes=planes)
    exp = nc.expected_bits(rc.expected(method, degree), planes, scale, bias, dtype)
    rc.same(got.view(exp.dtype), exp, "norm %s %s" % (layout, dtype))


@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_nv12_equals_i420(method, degree):
    boxes = rc.boxes(method, degree)
    rc.same(_host(method, degree, "nv12", boxes), _host(method, degree, "i420", boxes), "nv12 vs i420")


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_strides_and_sentinels(layout):
    """Frames a stride apart with sentinel bytes between them, and padded rows and outputs that keep theirs."""
    method, degree = "area", 0
    boxes = rc.boxes(method, degree)
    N, n = len(boxes), rc.FW * rc.FH * 3 // 2
    wide = np.full((rc.FRAMES, n + 37), 0x3C, np.uint8)
    src = wide[:, 5:5 + n]
    src[...] = rc.frames(layout)
    for order in ("rgb", "bgra"):
        C = len(yr.ORDERS[order])
        big = np.full((N, rc.DH + 3, rc.DW + 5, C), 0xA5, np.uint8)
        out = big[:, :rc.DH, :rc.DW]
        res = libiqo_amd.host_resize_rois_yuv(method, degree, rc.DW, rc.DH, src, boxes, rc.FW, rc.FH, layout=layout,
                                              standard=rc.STANDARD[(method, degree)], order=order, out=out)
        assert res is out
        rc.same(np.ascontiguousarray(out), yr.reorder(rc.expected(method, degree), yr.ORDERS[order]), "strided " + order)
        mask = np.ones(big.shape, bool)
        mask[:, :rc.DH, :rc.DW] = False
        assert (big[mask] == 0xA5).all()
    bigf = np.full((N, 3, rc.DH + 2, rc.DW + 3), np.float32(-7.5), np.float32)
    outf = bigf[:, :, :rc.DH, :rc.DW]
    libiqo_amd.host_resize_rois_yuv(method, degree, rc.DW, rc.DH, src, boxes, rc.FW, rc.FH, layout=layout,
                                    standard=rc.STANDARD[(method, degree)], scale=nc.NORM_SCALE[:3],
                                    bias=nc.NORM_BIAS[:3], out=outf)
    exp = nc.expected_bits(rc.expected(method, degree), (0, 1, 2), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "float32")
    rc.same(np.ascontiguousarray(outf).view(np.int32), exp, "norm strided")
    maskf = np.ones(bigf.shape, bool)
    maskf[:, :, :rc.DH, :rc.DW] = False
    assert (bigf[maskf] == np.float32(-7.5)).all()


def test_padded_rows():
    """Row strides larger than the rows (Y and chroma on their own, sentinels between the rows) and a frame stride."""
    method, degree = "lanczos", 2
    boxes = rc.boxes(method, degree)
    y, u, v = rc.planes()
    L = libiqo_amd.lib()
    for layout in rc.LAYOUTS:
        stY, stC = rc.FW + 3, (rc.FW if layout == "nv12" else rc.FW // 2) + 5
        hC = rc.FH // 2
        nU = stC * hC
        buf = np.full((rc.FRAMES, stY * rc.FH + 2 * nU + 11), 0x3C, np.uint8)
        for f in range(rc.FRAMES):
            buf[f, :stY * rc.FH].reshape(rc.FH, stY)[:, :rc.FW] = y[f]
            c = buf[f, stY * rc.FH:]
            if layout == "nv12":
                c[:nU].reshape(hC, stC)[:, :rc.FW] = np.stack([u[f], v[f]], axis=2).reshape(hC, rc.FW)
            else:
                c[:nU].reshape(hC, stC)[:, :rc.FW // 2] = u[f]
                c[nU:2 * nU].reshape(hC, stC)[:, :rc.FW // 2] = v[f]
        base = buf.ctypes.data
        out = np.zeros((len(boxes), rc.DH, rc.DW, 3), np.uint8)
        bad = ctypes.c_int(-1)
        order = (ctypes.c_int * 4)(0, 1, 2, 0)
        st = L.iqo_host_resize_rois_yuv_rgb(0, degree, libiqo_amd.ROI_LAYOUTS[layout], rc.DW, rc.DH, len(boxes),
                                            libiqo_amd._roi_array(list(boxes)), rc.FRAMES, rc.FW, rc.FH, stY, stC,
                                            buf.strides[0], base, base + stY * rc.FH,
                                            None if layout == "nv12" else base + stY * rc.FH + nU,
                                            rc.STANDARD[(method, degree)], 3, order, rc.DW * 3, rc.DW * rc.DH * 3,
                                            out.ctypes.data, ctypes.byref(bad))
        assert st == 0 and bad.value == -1
        rc.same(out, np.array(rc.expected(method, degree)), "padded rows " + layout)


def _rejected(method, degree, layout, boxes, status, bad, src=None, fw=rc.FW, fh=rc.FH, **kw):
    src = rc.frames(layout) if src is None else src
    for norm in (False, True):
        if norm:
            out = np.full((len(boxes), 3, rc.DH, rc.DW), np.float32(-7.5), np.float32)
            kw2 = dict(kw, scale=nc.NORM_SCALE[:3], bias=nc.NORM_BIAS[:3])
        else:
            out = np.full((len(boxes), rc.DH, rc.DW, 3), 0xA5, np.uint8)
            kw2 = kw
        with pytest.raises(libiqo_amd.IqoError) as e:
            libiqo_amd.host_resize_rois_yuv(method, degree, rc.DW, rc.DH, src, boxes, fw, fh, layout=layout, out=out, **kw2)
        assert (e.value.status, e.value.bad_roi) == (status, bad), (str(e.value), boxes)
        assert (out == (np.float32(-7.5) if norm else 0xA5)).all()  # the destination is untouched
        if bad >= 0:
            assert "box %d" % bad in str(e.value)


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_rejections(layout):
    for method, degree, boxes, status, bad in rc.REJECTED:
        _rejected(method, degree, layout, boxes, status, bad)
    for box in ((0, 0, 0, 0, 16), (0, 0, 0, 16, 0), (0, 150, 0, 12, 16), (0, 0, 112, 16, 10), (0, -2, 0, 16, 16),
                (3, 0, 0, 16, 16), (-1, 0, 0, 16, 16), (0, 0, 0, 16, 16, 2), (0, 0, 0, 16, 16, -1)):
        _rejected("area", 0, layout, [rc.GOOD, rc.GOOD, box], EINVAL, 2)
        _rejected("lanczos", 3, layout, [box], EINVAL, 0)
    # an odd frame width: the call itself
    odd = np.zeros((1, 15 * 16 * 3 // 2), np.uint8)
    _rejected("area", 0, layout, [(0, 0, 0, 8, 8)], EINVAL, -1, src=odd, fw=15, fh=16)
    odd = np.zeros((1, 16 * 15 * 3 // 2), np.uint8)
    _rejected("area", 0, layout, [(0, 0, 0, 8, 8)], EINVAL, -1, src=odd, fw=16, fh=15)
    _rejected("area", 0, layout, [rc.GOOD], EINVAL, -1, standard=4)
    # the boxes Lanczos rejects are fine for Area
    _host("area", 0, layout, [b for _, _, bl, st, _ in rc.REJECTED[:3] for b in bl])


def test_call_arguments():
    L = libiqo_amd.lib()
    src = np.array(rc.frames("i420"))
    dst = np.full((rc.DH, rc.DW, 3), 0xA5, np.uint8)
    roi = libiqo_amd._roi_array([rc.GOOD])
    bad = ctypes.c_int(7)
    base = src.ctypes.data
    n = rc.FW * rc.FH

    def call(layout=1, **k):
        order = k.get("order", (0, 1, 2, 3))
        order = None if order is None else (ctypes.c_int * 4)(*order)
        bad.value = 7
        return L.iqo_host_resize_rois_yuv_rgb(
            k.get("m", 1), 0, layout, rc.DW, rc.DH, 1, roi, rc.FRAMES, rc.FW, rc.FH, k.get("stY", rc.FW),
            k.get("stUV", rc.FW // 2 if layout else rc.FW), src.strides[0], k.get("y", base), k.get("u", base + n),
            k.get("v", base + n + n // 4), k.get("standard", 0), k.get("channels", 3),
            order, k.get("dstSt", rc.DW * 3), rc.DW * rc.DH * 3,
            k.get("dst", dst.ctypes.data), ctypes.byref(bad))

    assert call() == 0 and bad.value == -1
    assert call(layout=0, v=None) == 0 and bad.value == -1   # NV12 does not read dV
    dst[...] = 0xA5
    for k in ({"m": 3}, {"layout": 2}, {"stY": rc.FW - 1}, {"stUV": rc.FW // 2 - 1}, {"layout": 0, "stUV": rc.FW - 1},
              {"y": None}, {"u": None}, {"v": None}, {"dst": None}, {"standard": -1}, {"standard": 4}, {"channels": 2},
              {"channels": 5}, {"order": (0, 1, 4, 3)}, {"order": (-1, 1, 2, 3)}, {"order": None},
              {"dstSt": rc.DW * 3 - 1}):
        assert call(**k) == EINVAL and bad.value == -1, k
    assert (dst == 0xA5).all()
    # a plane of 2^31 bytes and more: unsupported, whatever the boxes
    assert call(stY=(1 << 31) // rc.FH + 1) == EUNSUP and bad.value == -1
    assert call(stUV=(1 << 31) // (rc.FH // 2) + 1) == EUNSUP and bad.value == -1


def test_empty_batch_and_python_surface():
    out = _host("area", 0, "nv12", [])
    assert out.shape == (0, rc.DH, rc.DW, 3)
    assert _host("area", 0, "i420", [], order="bgra").shape == (0, rc.DH, rc.DW, 4)
    for name in ("YuvRoiResizer", "host_resize_rois_yuv", "host_roi_yuv_arena_stats", "host_roi_yuv_box_layout",
                 "RoiYuvBoxLayout", "ROI_LAYOUTS"):
        assert name in libiqo_amd.__all__ and hasattr(libiqo_amd, name)
    L = libiqo_amd.lib()
    assert len(L.iqo_hip_resize_rois_yuv_rgb_device.argtypes) == 20
    assert len(L.iqo_hip_resize_rois_yuv_norm_device.argtypes) == 20
    bad = ctypes.c_int(3)
    order = (ctypes.c_int * 4)(0, 1, 2, 3)
    # null plan: rejected before anything is dereferenced
    assert L.iqo_hip_resize_rois_yuv_rgb_device(None, 0, None, 1, 8, 8, 8, 8, 96, 0x1000, 0x1040, None, 0, 3, order, 96,
                                                2304, 0x2000, None, ctypes.byref(bad)) == EINVAL


def _stats(method, degree, layout, boxes, frames=rc.FRAMES, fw=rc.FW, fh=rc.FH, dw=rc.DW, dh=rc.DH):
    return libiqo_amd.host_roi_yuv_arena_stats(method, degree, dw, dh, layout, boxes, frames, fw, fh)


@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_arena_stats_show_the_shared_tables(method, degree):
    boxes = list(rc.boxes(method, degree))
    assert len(boxes) == 13
    ws = {b[3] for b in boxes} | {b[3] // 2 for b in boxes}
    hs = {b[4] for b in boxes} | {b[4] // 2 for b in boxes}
    # 64 x 48 is both a luma size and the chroma size of 128 x 96; 90 and 62 occur three times each
    assert len(ws) == 19 and len(hs) == 15 and 64 in {b[3] for b in boxes} & {b[3] // 2 for b in boxes}
    for layout in rc.LAYOUTS:
        st = _stats(method, degree, layout, boxes)
        assert (st["x_tables"], st["y_tables"]) == (len(ws), len(hs))
        assert st["x_tables"] < 2 * 13 and st["y_tables"] < 2 * 13
        assert st["record_bytes"] == 96 and st["workgroups"] >= 13 and 0 < st["lds_bytes"] <= libiqo_amd.ROI_LDS_BYTES
        st2 = _stats(method, degree, layout, boxes + boxes)
        assert (st2["x_tables"], st2["y_tables"]) == (st["x_tables"], st["y_tables"])
        assert st2["arena_bytes"] - st["arena_bytes"] == 13 * st["record_bytes"]
        assert st2["workgroups"] == 2 * st["workgroups"]
    assert _stats(method, degree, "nv12", boxes) == _stats(method, degree, "i420", boxes)
    # the existing call's arena format is another one
    assert libiqo_amd.host_roi_arena_stats(method, degree, rc.DW, rc.DH, 1, boxes, rc.FRAMES, rc.FW, rc.FH)["record_bytes"] == 64


def test_box_layout_and_lds_cap():
    bl = libiqo_amd.host_roi_yuv_box_layout("lanczos", 3, "nv12", rc.DW, rc.DH, 90, 62)
    row = (bl["pitchDw"] + 2 * bl["pitchDwC"]) * 4 + (bl["nYp"] + bl["nYpC"]) * 8
    assert bl["lds_bytes"] == bl["rows"] * row and bl["rows"] == min(8, 16384 // row)
    assert bl["workgroups"] == -(-rc.DH // bl["rows"])
    assert bl["pitchDw"] % 2 == 1 and bl["pitchDwC"] % 2 == 1 and bl["nYp"] % 2 == 0 and bl["nYpC"] % 2 == 0
    one = libiqo_amd.host_roi_arena_stats("lanczos", 3, rc.DW, rc.DH, 1, [(0, 0, 0, 45, 31)], 1, 45, 31)
    assert one["lds_bytes"] > 0  # (the chroma tables of 90 x 62 are the luma tables of 45 x 31)
    assert bl == libiqo_amd.host_roi_yuv_box_layout("lanczos", 3, "i420", rc.DW, rc.DH, 90, 62)
    # one band row over IQO_HIP_ROI_LDS_BYTES: (w + w) 16-bit values
    ok = libiqo_amd.host_roi_yuv_box_layout("area", 0, "nv12", 4000, 2, 8000, 4)
    assert ok["rows"] == 1 and ok["lds_bytes"] <= libiqo_amd.ROI_LDS_BYTES
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.host_roi_yuv_box_layout("area", 0, "nv12", 9000, 2, 18000, 4)
    assert e.value.status == EUNSUP and "18000 x 4" in str(e.value)
    with pytest.raises(libiqo_amd.IqoError) as e:
        _stats("area", 0, "nv12", [(0, 0, 0, 64, 4), (0, 0, 0, 18000, 4)], frames=1, fw=18000, fh=4, dw=9000, dh=2)
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, 1) and "box 1" in str(e.value)


def test_tap_cap_on_the_chroma_axes():
    """A box at IQO_HIP_ROI_MAX_TAPS luma taps on both axes is accepted (its chroma axes have half as many); one
    more luma column pair per output column is refused."""
    cap = libiqo_amd.ROI_MAX_TAPS
    assert _stats("area", 0, "nv12", [(0, 0, 0, cap, 2 * cap)], frames=1, fw=cap, fh=2 * cap, dw=1, dh=2)["workgroups"] == 1
    with pytest.raises(libiqo_amd.IqoError) as e:
        _stats("area", 0, "nv12", [(0, 0, 0, cap + 2, 4)], frames=1, fw=cap + 2, fh=4, dw=1, dh=2)
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, 0)


def test_more_workgroups_than_a_grid():
    dh = 1 << 20
    box = (0, 0, 0, 2, 2)
    per = _stats("area", 0, "nv12", [box], frames=1, fw=2, fh=2, dw=1, dh=dh)["workgroups"]
    n = -(-(1 << 31) // per)
    assert n <= 1 << 15
    with pytest.raises(libiqo_amd.IqoError) as e:
        _stats("area", 0, "nv12", [box] * n, frames=1, fw=2, fh=2, dw=1, dh=dh)
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, n - 1)


def test_arena_walk_under_sanitizers(tmp_path):
    """tests/native/roi_yuv_walk.cpp: the layout, fill and walk of the 13-box call and of 4097 tiny boxes, and of the
    packed arena's boxes and 4097 one-pixel boxes at 1, 3 and 4 channels, in a stand-alone program built with
    -fsanitize=address,undefined, every offset checked against the buffers' sizes."""
    cxx = shutil.which("g++") or shutil.which("clang++") or shutil.which("c++")
    assert cxx, "no host C++ compiler"
    exe = str(tmp_path / "roi_yuv_walk")
    csrc = os.path.join(ROOT, "libiqo_amd", "csrc")
    # g++ links the sanitizer runtimes as shared libraries unless told otherwise (clang links them statically): static,
    # the program runs in whatever environment the suite runs in
    static = ["-static-libasan", "-static-libubsan"] if "clang" not in os.path.basename(cxx) else []
    subprocess.check_call([cxx, "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *static, "-ffp-contract=off", "-I", csrc, "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "roi_yuv_walk.cpp"), os.path.join(csrc, "roi.cpp"),
                           os.path.join(csrc, "plan.cpp"), "-o", exe])
    r = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert r.returncode == 0, r.stdout[-4000:]
    assert "roi_yuv_walk ok" in r.stdout
