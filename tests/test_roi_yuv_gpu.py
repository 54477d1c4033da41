"""GPU parity of the NV12 / I420 crop-and-resize straight to RGB (iqo_hip_resize_rois_yuv_*_device / YuvRoiResizer):
every box of one launch equals the CPU twin (which tests/test_roi_yuv_host.py pins to the Generic oracle and the
integer matrix) byte for byte, and the existing YUV resizers with chroma="full" on the cropped frame -- over every
method, both layouts, every kernel instantiation, every rows-per-workgroup value, box counts up to two search rounds,
misaligned planes and destinations, extreme frames, plane offsets beyond 4 GiB, strided outputs, queued calls and the
rejections.  Frames are 160 x 120 (one is 4096 x 16), outputs at most 32 x 24: well under a second each."""
import os

import numpy as np
import pytest

import norm_cases as nc
import oracle_lib as ol
import roi_yuv_cases as rc
import yuvrgb_cases as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
os.environ["IQO_REQUIRE_HIP"] = "1"
SENTINEL = 0xA5
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, EUNSUP = rc.EINVAL, rc.EUNSUP
METHOD_IDS = ["%s%d" % m for m in rc.METHODS]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _twin(method, degree, layout, boxes, frames=None, fw=rc.FW, fh=rc.FH, dw=rc.DW, dh=rc.DH, **kw):
    kw.setdefault("standard", rc.STANDARD.get((method, degree), "bt709"))
    frames = rc.frames(layout) if frames is None else frames
    return libiqo_amd.host_resize_rois_yuv(method, degree, dw, dh, frames, boxes, fw, fh, layout=layout, **kw)


def _src(layout):
    return torch.from_numpy(np.array(rc.frames(layout))).to(DEV)


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_equals_host_twin(method, degree, layout):
    """The whole case list in one call, then reversed: the second call uses the other arena and a warm cache."""
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    src = _src(layout)
    exp = _twin(method, degree, layout, boxes)
    rc.same(exp, np.array(rc.expected(method, degree)), "twin vs oracle")
    got = r.resize_rois_rgb(src, boxes, rc.FW, rc.FH, standard=std)
    back = r.resize_rois_rgb(src, boxes[::-1], rc.FW, rc.FH, standard=std)
    rc.same(got.cpu().numpy(), exp, "%s-%d %s" % (method, degree, layout))
    rc.same(back.cpu().numpy(), exp[::-1], "%s-%d %s reversed" % (method, degree, layout))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("method,degree,layout", [("lanczos", 3, "nv12"), ("area", 0, "i420")], ids=["lz3-nv12", "area-i420"])
def test_normalized_equals_host_twin(method, degree, layout, dtype):
    boxes, std, order = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)], (2, 0, 1)
    scale, bias = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    got = r.resize_rois_normalized(_src(layout), boxes, rc.FW, rc.FH, scale, bias, standard=std, dtype=TORCH_DTYPE[dtype],
                                   order=order)
    assert tuple(got.shape) == (len(boxes), 3, rc.DH, rc.DW) and got.dtype == TORCH_DTYPE[dtype]
    bits = nc.expected_bits(np.array(rc.expected(method, degree)), order, scale, bias, dtype)
    exp = _twin(method, degree, layout, boxes, scale=scale, bias=bias, dtype=dtype, planes=order)
    rc.same(exp.view(bits.dtype), bits, "twin vs numpy")
    rc.same(_bits(got), bits, "%s %s %s" % (method, layout, dtype))


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_agrees_with_full_chroma_resizers(method, degree, layout):
    """Independently of the twin: each box by Nv12Resizer / Yuv420Resizer(chroma="full").resize_rgb on a copy of the
    cropped frame."""
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    got = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout).resize_rois_rgb(
        _src(layout), boxes, rc.FW, rc.FH, standard=std).cpu().numpy()
    y, u, v = rc.planes()
    cls = libiqo_amd.Nv12Resizer if layout == "nv12" else libiqo_amd.Yuv420Resizer
    for i, b in enumerate(boxes):
        f, x, yy, w, h = b[:5]
        crop = rc.frames_of(y[f:f + 1, yy:yy + h, x:x + w], u[f:f + 1, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2],
                            v[f:f + 1, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2], layout)
        p = cls(method, degree, w, h, rc.DW, rc.DH, chroma="full")
        exp = p.resize_rgb(torch.from_numpy(crop).to(DEV), standard=std).cpu().numpy()[0]
        rc.same(got[i], exp[:, ::-1] if len(b) == 6 and b[5] else exp, "box %d %s" % (i, b))


@pytest.mark.parametrize("norm", (False, True), ids=["bytes", "norm"])
@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("method,degree", [("lanczos", 2), ("linear", 0)], ids=["LZ", "AL"])
def test_every_instantiation(method, degree, layout, norm):
    """roi_yuv_kernel<LZ, UV2, NORM>, the byte forms with 3 and with 4 bytes per pixel."""
    boxes, std = list(rc.boxes(method, degree))[:4], rc.STANDARD[(method, degree)]
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    exp = np.array(rc.expected(method, degree))[:4]
    if norm:
        got = r.resize_rois_normalized(_src(layout), boxes, rc.FW, rc.FH, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], standard=std,
                                       dtype=torch.bfloat16)
        rc.same(_bits(got), nc.expected_bits(exp, (0, 1, 2), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "bfloat16"), "norm")
        return
    for order in ("bgr", "rgba", "bgra"):
        got = r.resize_rois_rgb(_src(layout), boxes, rc.FW, rc.FH, standard=std, order=order)
        rc.same(got.cpu().numpy(), yr.reorder(exp, yr.ORDERS[order]), order)


WIDE_W, WIDE_H = 4096, 16
# (method, degree, dstW, dstH, box widths over the wide frame).  Area reaches every rows value: its tap cap admits
# boxes wide enough for one row per workgroup; Lanczos-3 (at most 682 columns to 32) covers 5 .. 8 rows.
BAND_PLANS = (("area", 0, 20, 13, (2560, 1800, 1240, 940, 740, 620, 540, 64)),
              ("area", 0, 32, 24, (4096, 1800, 1240, 940, 740, 620, 540, 64)),
              ("lanczos", 3, 32, 24, (680, 540, 480, 64)))


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_bands_and_rows_per_workgroup(layout):
    y = ol.splitmix_bytes(WIDE_W * WIDE_H, 31).reshape(1, WIDE_H, WIDE_W)
    uv = ol.splitmix_bytes(WIDE_W * WIDE_H // 2, 32).reshape(1, WIDE_H // 2, WIDE_W // 2, 2)
    wide = rc.frames_of(y, np.ascontiguousarray(uv[..., 0]), np.ascontiguousarray(uv[..., 1]), layout)
    seen, whole = set(), set()
    calls = []
    for method, degree, dw, dh, widths in BAND_PLANS:
        boxes, mine = [], set()
        for i, w in enumerate(widths):
            h = WIDE_H if i % 2 == 0 else WIDE_H - 4
            bl = libiqo_amd.host_roi_yuv_box_layout(method, degree, layout, dw, dh, w, h)
            mine.add(bl["rows"])
            whole.add(dh % bl["rows"] == 0)
            assert bl["workgroups"] == -(-dh // bl["rows"])
            boxes.append((0, (WIDE_W - w) // 2 & ~1, (WIDE_H - h) & ~1, w, h, i & 1))
        assert method != "area" or mine == set(range(1, 9)), (method, dw, dh, mine)
        seen |= mine
        calls.append((method, degree, dw, dh, boxes))
    # the coverage, before anything is launched
    assert seen == set(range(1, 9)) and whole == {True, False}, (seen, whole)
    src = torch.from_numpy(wide).to(DEV)
    for method, degree, dw, dh, boxes in calls:
        r = libiqo_amd.YuvRoiResizer(method, degree, dw, dh, layout=layout)
        exp = _twin(method, degree, layout, boxes, frames=wide, fw=WIDE_W, fh=WIDE_H, dw=dw, dh=dh, order="rgba",
                    standard="bt601")
        got = r.resize_rois_rgb(src, boxes, WIDE_W, WIDE_H, order="rgba", standard="bt601")
        rc.same(got.cpu().numpy(), exp, "wide %s %dx%d" % (method, dw, dh))
        # the small frames through the same plan
        small = [b for b in rc.BOXES if rc.defined(method, degree, b[3], b[4], dh)]
        assert len(small) >= 12
        exp = _twin(method, degree, layout, small, dw=dw, dh=dh)
        got = r.resize_rois_rgb(_src(layout), small, rc.FW, rc.FH, standard=rc.STANDARD[(method, degree)])
        rc.same(got.cpu().numpy(), exp, "small %s %dx%d" % (method, dw, dh))


def _tiny_boxes(n):
    """n boxes of 4 x 4 .. 16 x 12 anywhere in the small frames, seeded."""
    v = ol.splitmix_bytes(6 * n, 4097).astype(np.int64).reshape(n, 6)
    out = []
    for a in v:
        w, h = 4 + 2 * int(a[0] % 7), 4 + 2 * int(a[1] % 5)
        out.append((int(a[2] % rc.FRAMES), 2 * int(a[3] % ((rc.FW - w) // 2 + 1)), 2 * int(a[4] % ((rc.FH - h) // 2 + 1)),
                    w, h, int(a[5] & 1)))
    return out


@pytest.mark.parametrize("n", (1, 2, 65, 4097))
def test_box_counts(n):
    """One box, two, more than one round's 64 lanes, and two search rounds."""
    method, degree, dw, dh = "area", 0, 8, 6
    boxes = _tiny_boxes(n)
    assert {b[3] for b in _tiny_boxes(4097)} == set(range(4, 17, 2)) and {b[4] for b in _tiny_boxes(4097)} == set(range(4, 13, 2))
    for layout in rc.LAYOUTS:
        r = libiqo_amd.YuvRoiResizer(method, degree, dw, dh, layout=layout)
        got = r.resize_rois_rgb(_src(layout), boxes, rc.FW, rc.FH)
        rc.same(got.cpu().numpy(), _twin(method, degree, layout, boxes, dw=dw, dh=dh, standard="bt709"), "%d boxes" % n)


def _plane_tensor(planes, off, st, frame_st):
    """planes [F, rows, n] at byte offset `off` of a device tensor that ends at the last plane's last byte, rows st
    and frames frame_st bytes apart; the rest holds a sentinel.  Returns (tensor, address of plane 0)."""
    F, rows, n = planes.shape
    t = torch.full((off + (F - 1) * frame_st + (rows - 1) * st + n,), 0x3C, dtype=torch.uint8, device=DEV)
    t.as_strided((F, rows, n), (frame_st, st, 1), off).copy_(torch.from_numpy(np.array(planes)))
    return t, t.data_ptr() + off


@pytest.mark.parametrize("layout", rc.LAYOUTS)
@pytest.mark.parametrize("offs,padY,padC", [((1, 2, 3), 1, 2), ((2, 3, 1), 2, 1), ((3, 1, 2), 0, 3)],
                         ids=["st1-2", "st2-1", "st0-3"])
def test_misaligned_planes_and_destinations(layout, offs, padY, padC):
    """Base pointers at byte offsets 1, 2, 3; row strides = 1 and 2 (mod 4) take the per-tap alignment path; RGBA
    outputs at offset 1 with an odd row stride; boxes that end at a plane's last byte, where the tensor ends."""
    method, degree = "lanczos", 3
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    assert any(b[0] == rc.FRAMES - 1 and b[1] + b[3] == rc.FW and b[2] + b[4] == rc.FH for b in boxes)
    y, u, v = rc.planes()
    stY = rc.FW + padY
    cw = rc.FW if layout == "nv12" else rc.FW // 2
    stC = cw + padC
    assert stY % 4 == padY % 4 and stC % 4 == padC % 4
    frame_st = stY * rc.FH + 7
    keep = []
    ty, dY = _plane_tensor(y, offs[0], stY, frame_st)
    if layout == "nv12":
        tu, dU = _plane_tensor(np.stack([u, v], axis=3).reshape(rc.FRAMES, rc.FH // 2, rc.FW), offs[1], stC, frame_st)
        dV = None
    else:
        tu, dU = _plane_tensor(u, offs[1], stC, frame_st)
        tv, dV = _plane_tensor(v, offs[2], stC, frame_st)
        keep.append(tv)
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    N = len(boxes)
    row_st = rc.DW * 4 + 1
    roi_st = rc.DH * row_st + 2
    flat = torch.full((1 + N * roi_st,), SENTINEL, dtype=torch.uint8, device=DEV)
    r.resize_rois_rgb_device(boxes, rc.FRAMES, rc.FW, rc.FH, stY, stC, frame_st, dY, dU, dV, row_st, roi_st,
                             flat.data_ptr() + 1, standard=std, order="rgba", stream=torch.cuda.current_stream(DEV))
    torch.cuda.synchronize(DEV)
    h = flat.cpu().numpy()
    view = np.lib.stride_tricks.as_strided(h[1:], (N, rc.DH, rc.DW, 4), (roi_st, row_st, 4, 1))
    rc.same(np.ascontiguousarray(view), yr.reorder(np.array(rc.expected(method, degree)), yr.ORDERS["rgba"]), "misaligned")
    mask = np.ones(h.shape, bool)
    np.lib.stride_tricks.as_strided(mask[1:], (N, rc.DH, rc.DW * 4), (roi_st, row_st, 1))[...] = False
    assert (h[mask] == SENTINEL).all()
    del ty, tu, keep


EXT_W, EXT_H = 64, 48
EXT_BOXES = ((0, 0, 0, 64, 48), (1, 0, 0, 64, 48), (2, 0, 0, 64, 48), (3, 0, 0, 64, 48), (2, 8, 4, 50, 40), (3, 6, 2, 52, 44, 1))


@pytest.mark.parametrize("degree", (3, 5))
def test_extreme_frames(degree):
    """All-0, all-255 and the two clamp frames of yuvrgb_cases: both colour clamps and both resize clamps are live."""
    method = "lanczos"
    cy, cu, cv = yr.clamp_frames((method, degree, EXT_W, EXT_H, rc.DW, rc.DH, "nv12"))
    flat = lambda val, a: np.full((1,) + a.shape[1:], val, np.uint8)
    y = np.concatenate([flat(0, cy), flat(255, cy), cy])
    u = np.concatenate([flat(0, cu), flat(255, cu), cu])
    v = np.concatenate([flat(0, cv), flat(255, cv), cv])
    boxes = list(EXT_BOXES)
    lo = hi = neg = over = 0
    exp = np.zeros((len(boxes), rc.DH, rc.DW, 3), np.uint8)
    for i, b in enumerate(boxes):
        f, x, yy, w, h = b[:5]
        assert rc.defined(method, degree, w, h)
        py, pu, pv = rc.oracle_box(method, degree, y, u, v, b)
        raw = yr.raw_rgb(yr.BT709_LIMITED, py, pu, pv)
        lo, hi = lo + int((raw < 0).sum()), hi + int((raw > 255).sum())
        _, st = ol.run_oracle_stats(method, degree, w, h, rc.DW, rc.DH, 1, np.ascontiguousarray(y[f, yy:yy + h, x:x + w]))
        neg, over = neg + st["xm_neg"], over + st["xm_hi"]
        rgb = yr.yuv_to_rgb(yr.BT709_LIMITED, py, pu, pv)
        exp[i] = rgb[:, ::-1] if len(b) == 6 else rgb
    assert lo > 0 and hi > 0 and neg > 0 and over > 0, (lo, hi, neg, over)
    for layout in rc.LAYOUTS:
        frames = rc.frames_of(y, u, v, layout)
        rc.same(_twin(method, degree, layout, boxes, frames=frames, fw=EXT_W, fh=EXT_H, standard="bt709"), exp, "twin")
        r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
        got = r.resize_rois_rgb(torch.from_numpy(frames).to(DEV), boxes, EXT_W, EXT_H, standard="bt709")
        rc.same(got.cpu().numpy(), exp, "extreme %s" % layout)


def test_plane_offsets_beyond_4gib():
    """Frames 2^32 - 10000 bytes apart with chroma rows 1024 bytes apart: in frame 1 a box at y = 100 has its Y offset
    beyond 2^32, and a box at y = 40 its UV offset only."""
    if torch.cuda.mem_get_info()[0] < 6 * 2 ** 30:
        pytest.skip("less than 6 GiB of free device memory")
    method, degree, layout = "lanczos", 3, "nv12"
    frame_st, stY, stC, uv_base = 2 ** 32 - 10000, rc.FW, 1024, 32768
    boxes = [(1, 20, 100, 64, 20), (1, 8, 40, 90, 62), (0, 4, 10, 90, 62, 1), (1, 0, 0, 32, 24)]
    off_y = [b[0] * frame_st + b[2] * stY + b[1] for b in boxes]
    off_c = [b[0] * frame_st + (b[2] // 2) * stC + b[1] for b in boxes]
    assert off_y[0] >= 2 ** 32 and off_y[1] < 2 ** 32 <= off_c[1] and off_c[3] < 2 ** 32 and off_y[2] < 2 ** 32
    assert all(rc.defined(method, degree, b[3], b[4]) for b in boxes)
    y, u, v = rc.planes()
    buf = torch.empty(frame_st + uv_base + stC * rc.FH // 2 + 4096, dtype=torch.uint8, device=DEV)  # left unfilled
    buf.as_strided((2, rc.FH, rc.FW), (frame_st, stY, 1)).copy_(torch.from_numpy(np.array(y[:2])))
    uv = np.stack([u[:2], v[:2]], axis=3).reshape(2, rc.FH // 2, rc.FW)
    buf.as_strided((2, rc.FH // 2, rc.FW), (frame_st, stC, 1), uv_base).copy_(torch.from_numpy(np.ascontiguousarray(uv)))
    exp = _twin(method, degree, layout, boxes)
    big = torch.full((len(boxes), rc.DH + 1, rc.DW + 2, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    out = big[:, :rc.DH, :rc.DW]
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    r.resize_rois_rgb_device(boxes, 2, rc.FW, rc.FH, stY, stC, frame_st, buf.data_ptr(), buf.data_ptr() + uv_base, None,
                             out.stride(1), out.stride(0), out, standard=rc.STANDARD[(method, degree)],
                             stream=torch.cuda.current_stream(DEV))
    torch.cuda.synchronize(DEV)
    rc.same(out.cpu().numpy(), exp, "frames 2^32 - 10000 bytes apart")
    h = big.cpu().numpy()
    assert (h[:, rc.DH:] == SENTINEL).all() and (h[:, :, rc.DW:] == SENTINEL).all()
    del buf
    torch.cuda.empty_cache()


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_strided_out_views(layout):
    method, degree = "lanczos", 2
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    N = len(boxes)
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    exp = np.array(rc.expected(method, degree))
    for order in ("rgb", "rgba"):
        C = len(yr.ORDERS[order])
        big = torch.full((N, rc.DH + 3, rc.DW + 5, C), SENTINEL, dtype=torch.uint8, device=DEV)
        out = big[:, :rc.DH, :rc.DW]
        assert r.resize_rois_rgb(_src(layout), boxes, rc.FW, rc.FH, standard=std, order=order, out=out) is out
        rc.same(out.cpu().numpy(), yr.reorder(exp, yr.ORDERS[order]), "strided " + order)
        h = big.cpu().numpy()
        assert (h[:, rc.DH:] == SENTINEL).all() and (h[:, :, rc.DW:] == SENTINEL).all()
    bigf = torch.full((N, 3, rc.DH + 1, rc.DW + 3), -7.5, dtype=torch.float16, device=DEV)
    outf = bigf[:, :, :rc.DH, :rc.DW]
    r.resize_rois_normalized(_src(layout), boxes, rc.FW, rc.FH, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], standard=std,
                             dtype=torch.float16, order=(2, 1, 0), out=outf)
    rc.same(_bits(outf), nc.expected_bits(exp, (2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "float16"), "strided norm")
    hf = bigf.cpu().numpy()
    assert (hf[:, :, rc.DH:] == np.float16(-7.5)).all() and (hf[:, :, :, rc.DW:] == np.float16(-7.5)).all()


def test_queued_calls_on_one_stream():
    """Two and three calls back to back with different boxes, no synchronisation between them: the third refills the
    first arena (after its event)."""
    method, degree, layout = "lanczos", 3, "nv12"
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    batches = [boxes[:5], boxes[5:], boxes[3:9][::-1]]
    src = _src(layout)
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    s = torch.cuda.Stream(DEV)
    outs = [torch.zeros((len(b), rc.DH, rc.DW, 3), dtype=torch.uint8, device=DEV) for b in batches]
    torch.cuda.synchronize(DEV)
    for n in (2, 3, 3):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize(DEV)
        for b, o in list(zip(batches, outs))[:n]:
            r.resize_rois_rgb(src, b, rc.FW, rc.FH, standard=std, out=o, stream=s)
        s.synchronize()
        for b, o in list(zip(batches, outs))[:n]:
            rc.same(o.cpu().numpy(), _twin(method, degree, layout, b), "queued %d" % n)


def test_capturing_stream_is_unsupported():
    method, degree, layout = "area", 0, "i420"
    boxes, std = list(rc.boxes(method, degree)), rc.STANDARD[(method, degree)]
    src = _src(layout)
    r = libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout)
    out = torch.full((len(boxes), rc.DH, rc.DW, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    dummy = torch.zeros(16, device=DEV)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    status = []
    with torch.cuda.graph(g):
        dummy.add_(1.0)
        try:
            r.resize_rois_rgb(src, boxes, rc.FW, rc.FH, standard=std, out=out, stream=torch.cuda.current_stream(DEV))
        except libiqo_amd.IqoError as e:
            status.append(e.status)
    torch.cuda.synchronize(DEV)
    assert status == [EUNSUP]
    assert (out.cpu().numpy() == SENTINEL).all()
    # the plan is usable afterwards
    rc.same(r.resize_rois_rgb(src, boxes, rc.FW, rc.FH, standard=std).cpu().numpy(), _twin(method, degree, layout, boxes),
            "after the capture")


@pytest.mark.parametrize("layout", rc.LAYOUTS)
def test_rejections_launch_nothing(layout):
    src = _src(layout)
    plans = {}
    for method, degree, boxes, status, bad in rc.REJECTED:
        r = plans.setdefault((method, degree), libiqo_amd.YuvRoiResizer(method, degree, rc.DW, rc.DH, layout=layout))
        out = torch.full((len(boxes), rc.DH, rc.DW, 3), SENTINEL, dtype=torch.uint8, device=DEV)
        outf = torch.full((len(boxes), 3, rc.DH, rc.DW), -7.5, dtype=torch.float32, device=DEV)
        for call in (lambda: r.resize_rois_rgb(src, boxes, rc.FW, rc.FH, out=out),
                     lambda: r.resize_rois_normalized(src, boxes, rc.FW, rc.FH, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], out=outf)):
            with pytest.raises(libiqo_amd.IqoError) as e:
                call()
            assert (e.value.status, e.value.bad_roi) == (status, bad), str(e.value)
            assert "box %d" % bad in str(e.value)
        torch.cuda.synchronize(DEV)
        assert (out.cpu().numpy() == SENTINEL).all() and (outf.cpu().numpy() == np.float32(-7.5)).all()
    # an odd frame width: the call itself
    r = plans[("area", 0)]
    odd = torch.zeros((1, 15 * 16 * 3 // 2), dtype=torch.uint8, device=DEV)
    out = torch.full((1, rc.DH, rc.DW, 3), SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(libiqo_amd.IqoError) as e:
        r.resize_rois_rgb(odd, [(0, 0, 0, 8, 8)], 15, 16, out=out)
    assert (e.value.status, e.value.bad_roi) == (EINVAL, -1)
    with pytest.raises(libiqo_amd.IqoError) as e:
        r.resize_rois_rgb(src, [rc.GOOD], rc.FW, rc.FH, standard=7, out=out)
    assert (e.value.status, e.value.bad_roi) == (EINVAL, -1)
    torch.cuda.synchronize(DEV)
    assert (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.YuvRoiResizer("area", 0, rc.DW, rc.DH, layout="yuy2")
    # an empty batch is fine
    assert tuple(r.resize_rois_rgb(src, [], rc.FW, rc.FH).shape) == (0, rc.DH, rc.DW, 3)
