"""Batched crop-and-resize (iqo_hip_resize_rois_device), the part that needs no GPU: the CPU twin
(iqo_host_resize_rois / _norm), which builds the call's arena exactly as the device call does and walks it
with the kernel's integer formulas, against the Generic oracle on every cropped box; the arena statistics;
and every rejection of the call.
"""
import ctypes

import numpy as np
import pytest

import libiqo_amd
import norm_cases as nc
import oracle_lib as ol
import roi_cases as rc

EINVAL, EUNSUP = -1, -5
METHOD_IDS = ["%s%d" % m for m in rc.METHODS]


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_host_equals_oracle(method, degree, C):
    boxes = rc.boxes(method, degree)
    assert len(boxes) >= 9 and any(len(b) == 6 and b[5] for b in boxes)
    got = libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, rc.frames(C), boxes)
    _same(got, rc.expected(method, degree, C), "%s-%d C=%d" % (method, degree, C))
    if ol.ref_available():
        assert rc.check_reference(method, degree, C) >= 5


def test_case_list_is_what_the_issue_names():
    """All boxes are defined for Lanczos-2 and -3; the two rejection shapes are not."""
    for deg in (2, 3):
        assert rc.boxes("lanczos", deg) == list(rc.BOXES)
    for method, deg, b in rc.UNDEFINED:
        assert not ol.lanczos_rows_defined(deg, b[4], rc.DH)
    xs = {b[1] % 4 for b in rc.BOXES}
    assert xs == {0, 1, 2, 3} and {(3 * x) % 4 for x in xs} == {0, 1, 2, 3}
    assert any(b[0] == rc.FRAMES - 1 and b[1] + b[3] == rc.FW and b[2] + b[4] == rc.FH for b in rc.BOXES)


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("C,order", [(3, (2, 0, 1)), (4, (3, 1)), (1, (0, 0, 0))], ids=["rgb-perm", "rgba-pick", "grey3"])
def test_host_norm_equals_numpy(C, order, dtype):
    """float32(u8) * scale + bias, two rounded operations, then rounded to the half types."""
    method, degree = "lanczos", 3
    boxes = rc.boxes(method, degree)
    scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
    got = libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, rc.frames(C), boxes, scale=scale, bias=bias,
                                      dtype=dtype, order=order)
    u8 = rc.expected(method, degree, C)
    exp = nc.expected_bits(u8[..., None] if C == 1 else u8, order, scale, bias, dtype)
    _same(got.view(exp.dtype), exp, "norm C=%d %s" % (C, dtype))


def test_host_norm_rounding_extremes():
    """Scales that drive the half conversions through subnormals, ties and overflow."""
    boxes = [(0, 0, 0, 32, 24)]  # identity: the output bytes are the source's
    src = np.arange(rc.DW * rc.DH, dtype=np.uint32).astype(np.uint8).reshape(1, rc.DH, rc.DW)
    for dtype in nc.DTYPES:
        for scale, bias in ((2.0 ** -24, 0.0), (2.0 ** -25 * 3, -1e-6), (300.0, -5.0), (257.0, 65000.0), (1e38, 1e38),
                            (2.0 ** -17, 2.0 ** -15), (-1.0 / 3, 1.0 / 7)):
            got = libiqo_amd.host_resize_rois("area", 0, rc.DW, rc.DH, src, boxes, scale=(scale,), bias=(bias,),
                                              dtype=dtype, order=(0,))
            with np.errstate(over="ignore"):
                exp = nc.expected_bits(src[..., None], (0,), (scale,), (bias,), dtype)
            _same(got.view(exp.dtype), exp, "%s scale %g bias %g" % (dtype, scale, bias))


@pytest.mark.parametrize("C", (1, 3))
def test_pixels_outside_the_boxes_do_not_matter(C):
    method, degree = "lanczos", 3
    boxes = rc.boxes(method, degree)
    a = rc.frames(C)
    inside = np.zeros(a.shape[:3], bool)
    for b in boxes:
        inside[b[0], b[2]:b[2] + b[4], b[1]:b[1] + b[3]] = True
    assert not inside.all()
    other = ol.splitmix_bytes(a.size, 77).reshape(a.shape)
    b2 = np.where(inside if C == 1 else inside[..., None], a, other)
    assert (b2 != a).any()
    _same(libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, b2, boxes),
          libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, a, boxes), "outside pixels")
    # each box alone, as a frame of its own, gives the same bytes: the box is the whole image
    full = rc.expected(method, degree, C)
    for i, b in enumerate(boxes[:4]):
        crop = np.ascontiguousarray(a[b[0]:b[0] + 1, b[2]:b[2] + b[4], b[1]:b[1] + b[3]])
        _same(libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, crop, [(0, 0, 0, b[3], b[4])])[0], full[i], str(b))


@pytest.mark.parametrize("C", (1, 3, 4))
def test_strides_and_sentinels(C):
    """Bytes between dstW*C and dstSt, and between outputs, keep their sentinel; a strided source (a crop view of
    larger frames, rows no multiple of 4 bytes) is read where it lies."""
    method, degree = "area", 0
    boxes = rc.boxes(method, degree)
    N = len(boxes)
    big = np.full((N, rc.DH + 3, rc.DW + 5) + ((C,) if C > 1 else ()), 0xA5, np.uint8)
    out = big[:, :rc.DH, :rc.DW]
    wide = np.full((rc.FRAMES + 1, rc.FH + 2, rc.FW + 3) + ((C,) if C > 1 else ()), 0x3C, np.uint8)
    src = wide[1:, 1:rc.FH + 1, 2:rc.FW + 2]
    src[...] = rc.frames(C)
    assert not src.flags["C_CONTIGUOUS"]
    res = libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, src, boxes, out=out)
    assert res is out
    _same(np.ascontiguousarray(out), rc.expected(method, degree, C), "strided")
    mask = np.ones(big.shape, bool)
    mask[:, :rc.DH, :rc.DW] = False
    assert (big[mask] == 0xA5).all()


def test_norm_sentinels():
    method, degree, C, order = "linear", 0, 3, (0, 1, 2)
    boxes = rc.boxes(method, degree)
    big = np.full((len(boxes), 3, rc.DH + 2, rc.DW + 3), np.float32(-7.5), np.float32)
    out = big[:, :, :rc.DH, :rc.DW]
    libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, rc.frames(C), boxes, scale=nc.NORM_SCALE[:3],
                                bias=nc.NORM_BIAS[:3], order=order, out=out)
    exp = nc.expected_bits(rc.expected(method, degree, C), order, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "float32")
    _same(np.ascontiguousarray(out).view(np.int32), exp, "norm strided")
    mask = np.ones(big.shape, bool)
    mask[:, :, :rc.DH, :rc.DW] = False
    assert (big[mask] == np.float32(-7.5)).all()


def _stats(method, degree, C, boxes, frames=rc.FRAMES, fw=rc.FW, fh=rc.FH, dw=rc.DW, dh=rc.DH):
    return libiqo_amd.host_roi_arena_stats(method, degree, dw, dh, C, boxes, frames, fw, fh)


@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_arena_stats(method, degree):
    boxes = rc.boxes(method, degree)
    st = _stats(method, degree, 3, boxes)
    assert st["x_tables"] == len({b[3] for b in boxes}) and st["y_tables"] == len({b[4] for b in boxes})
    assert st["workgroups"] >= len(boxes) and 0 < st["lds_bytes"] <= libiqo_amd.ROI_LDS_BYTES
    # the batch twice in one call: no new table, the arena grows by the box records only
    st2 = _stats(method, degree, 3, boxes + boxes)
    assert (st2["x_tables"], st2["y_tables"]) == (st["x_tables"], st["y_tables"])
    assert st2["arena_bytes"] - st["arena_bytes"] == len(boxes) * st["record_bytes"]
    assert st2["workgroups"] == 2 * st["workgroups"]
    # the tables do not depend on the channel count, the work rows do
    assert _stats(method, degree, 1, boxes)["arena_bytes"] == st["arena_bytes"]


def _rejected(method, degree, C, boxes, status, bad, frames=None, dw=rc.DW, dh=rc.DH):
    src = rc.frames(C) if frames is None else frames
    out = np.full((len(boxes), dh, dw) + ((C,) if C > 1 else ()), 0xA5, np.uint8)
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.host_resize_rois(method, degree, dw, dh, src, boxes, out=out)
    assert (e.value.status, e.value.bad_roi) == (status, bad), (str(e.value), boxes)
    assert (out == 0xA5).all()  # the destination is untouched
    if bad >= 0:
        assert "box %d" % bad in str(e.value)


GOOD = (0, 1, 3, 64, 48)


@pytest.mark.parametrize("box", [
    (0, 4, 4, 0, 10), (0, 4, 4, 10, 0), (0, 4, 4, -3, 10),            # empty
    (0, 150, 4, 11, 10), (0, 4, 111, 10, 10), (0, -1, 4, 10, 10), (0, 4, -1, 10, 10), (0, 160, 0, 1, 1),  # outside
    (3, 4, 4, 10, 10), (-1, 4, 4, 10, 10),                           # frame index
    (0, 4, 4, 10, 10, 2), (0, 4, 4, 10, 10, 3), (0, 4, 4, 10, 10, -1),  # unknown flag bit
])
def test_invalid_boxes(box):
    for method, degree in (("lanczos", 3), ("area", 0)):
        _rejected(method, degree, 3, [GOOD, GOOD, box, (0, 0, 0, 0, 0)], EINVAL, 2)
        _rejected(method, degree, 1, [box], EINVAL, 0)


def test_undefined_lanczos_boxes():
    """The condition build_plan rejects: the top border band is taller than the output."""
    for method, degree, box in rc.UNDEFINED:
        _rejected(method, degree, 3, [GOOD, box, GOOD], EINVAL, 1)
        # (the plan constructors' own verdict on that shape, through the host-only query)
        assert libiqo_amd.lib().iqo_host_kernel_for(0, degree, box[3], box[4], rc.DW, rc.DH, 1) < 0
    # the same boxes are fine for Area, and Linear up-scales above 2x are accepted and unpinned
    for box in (b for _, _, b in rc.UNDEFINED):
        libiqo_amd.host_resize_rois("area", 0, rc.DW, rc.DH, rc.frames(1), [box])
        libiqo_amd.host_resize_rois("linear", 0, rc.DW, rc.DH, rc.frames(1), [box])


def test_unsupported_channels_and_arguments():
    two = np.zeros((1, 8, 8, 2), np.uint8)
    _rejected("area", 0, 2, [(0, 0, 0, 4, 4)], EUNSUP, -1, frames=two)
    L = libiqo_amd.lib()
    bad = ctypes.c_int(7)
    roi = (libiqo_amd.Roi * 1)(libiqo_amd.Roi(0, 0, 0, 4, 4, 0))
    src = np.zeros((8, 8), np.uint8)
    dst = np.full((24, 32), 0xA5, np.uint8)
    args = lambda **k: [k.get("m", 1), 0, 1, 32, 24, 1, roi, 1, 8, 8, k.get("srcSt", 8), 64,
                        k.get("src", src.ctypes.data), k.get("dstSt", 32), 32 * 24, k.get("dst", dst.ctypes.data),
                        ctypes.byref(bad)]
    assert L.iqo_host_resize_rois(*args()) == 0 and bad.value == -1
    dst[...] = 0xA5
    for k in ({"m": 3}, {"srcSt": 7}, {"src": None}, {"dst": None}, {"dstSt": 31}):
        bad.value = 7
        assert L.iqo_host_resize_rois(*args(**k)) == EINVAL and bad.value == -1, k
    assert (dst == 0xA5).all()
    # Lanczos degree 0
    a = args(m=0)
    assert L.iqo_host_resize_rois(*a) == EINVAL and bad.value == 0


def _taps(method, degree, src_len, dst_len):
    return len(libiqo_amd.host_tables(method, degree, src_len, 4, dst_len, 4, 1, 0)[0])


@pytest.mark.parametrize("method,degree", [("area", 0), ("lanczos", 3)])
def test_tap_cap(method, degree):
    """A box at IQO_HIP_ROI_MAX_TAPS taps is accepted, one tap (Area) / one tap pair (Lanczos) over it is refused,
    on either axis.  The cap admits Lanczos-3 at 8:1 and Area at 16:1."""
    cap = libiqo_amd.ROI_MAX_TAPS
    assert _taps("lanczos", 3, 8 * 32, 32) <= cap and _taps("area", 0, 16 * 32, 32) <= cap
    d = 1 if method == "area" else 3  # Lanczos-3 taps are 2 ceil(3 s / d): 128 needs d = 3
    taps = {s: _taps(method, degree, s, d) for s in range(d + 1, 200)}
    at = max(s for s, t in taps.items() if t == cap)
    over = min(s for s, t in taps.items() if t > cap)
    assert taps[over] == cap + (1 if method == "area" else 2)
    wide = np.zeros((1, 200, 200), np.uint8)
    wide[...] = ol.splitmix_bytes(200 * 200, 5).reshape(200, 200)
    for box_at, box_over in (((0, 0, 0, at, 8), (0, 0, 0, over, 8)), ((0, 0, 0, 8, at), (0, 0, 0, 8, over))):
        assert method != "lanczos" or ol.lanczos_rows_defined(degree, box_at[4], d)
        got = libiqo_amd.host_resize_rois(method, degree, d, d, wide, [box_at])
        w, h = box_at[3], box_at[4]
        exp = ol.run_oracle(method, degree, w, h, d, d, 1, np.ascontiguousarray(wide[0, :h, :w]))
        _same(got[0], np.array(exp), "at the cap %s" % (box_at,))
        _rejected(method, degree, 1, [box_at, box_over], EUNSUP, 1, frames=wide, dw=d, dh=d)


def test_lds_cap():
    """One work row must fit IQO_HIP_ROI_LDS_BYTES: boxes 4096 wide at Lanczos-3 8:1 and Area 16:1 fit with 4
    channels; 4 channels x 9000 columns do not."""
    for method, degree, w, h, dw, dh in (("lanczos", 3, 4096, 64, 512, 8), ("area", 0, 4096, 64, 256, 4)):
        st = _stats(method, degree, 4, [(0, 0, 0, w, h)], frames=1, fw=4096, fh=64, dw=dw, dh=dh)
        assert st["lds_bytes"] <= libiqo_amd.ROI_LDS_BYTES and st["workgroups"] == dh
    with pytest.raises(libiqo_amd.IqoError) as e:
        _stats("area", 0, 4, [(0, 0, 0, 64, 2), (0, 0, 0, 9000, 2)], frames=1, fw=9000, fh=2, dw=4500, dh=2)
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, 1)
    assert _stats("area", 0, 1, [(0, 0, 0, 9000, 2)], frames=1, fw=9000, fh=2, dw=4500, dh=2)["workgroups"] == 2


def test_more_workgroups_than_a_grid():
    """2^31 workgroups: 16384 boxes of 2^20 output rows, 8 rows per workgroup."""
    dh = 1 << 20
    box = (0, 0, 0, 1, 1)
    per = _stats("area", 0, 1, [box], frames=1, fw=1, fh=1, dw=1, dh=dh)["workgroups"]
    n = -(-(1 << 31) // per)
    assert n <= 1 << 15
    assert _stats("area", 0, 1, [box] * (n - 1), frames=1, fw=1, fh=1, dw=1, dh=dh)["workgroups"] == (n - 1) * per
    with pytest.raises(libiqo_amd.IqoError) as e:
        _stats("area", 0, 1, [box] * n, frames=1, fw=1, fh=1, dw=1, dh=dh)
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, n - 1)


def test_empty_batch_and_python_surface():
    out = libiqo_amd.host_resize_rois("area", 0, rc.DW, rc.DH, rc.frames(3), [])
    assert out.shape == (0, rc.DH, rc.DW, 3)
    for name in ("RoiResizer", "host_resize_rois", "host_roi_arena_stats", "Roi"):
        assert name in libiqo_amd.__all__
    assert ctypes.sizeof(libiqo_amd.Roi) == 24
    L = libiqo_amd.lib()
    assert len(L.iqo_hip_resize_rois_device.argtypes) == 14 and len(L.iqo_hip_resize_rois_norm_device.argtypes) == 16
    # null plan: rejected before anything is dereferenced
    bad = ctypes.c_int(3)
    assert L.iqo_hip_resize_rois_device(None, 0, None, 1, 8, 8, 8, 64, 0x1000, 32, 768, 0x2000, None,
                                        ctypes.byref(bad)) == EINVAL
