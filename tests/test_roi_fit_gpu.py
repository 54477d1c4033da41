"""GPU parity of boxes into destination rectangles (iqo_hip_resize_rois_fit_*_device,
iqo_hip_resize_rois_yuv_fit_*_device): every canvas of one launch equals the CPU twin (which
tests/test_roi_fit_host.py pins to the oracle canvas) bit for bit, over all 12 packed and 8 YUV fit instantiations;
the rectangle equals the stretch call and the per-shape resizers; every byte of a canvas is written once and nothing
outside it (each strided case runs on a buffer filled with 0xA5 and again with 0x5A); the pad stores at every
misalignment; pad workgroups; batch sizes.  Canvases are 48 x 40 and smaller but for two pad-store shapes."""
import os

import numpy as np
import pytest

import norm_cases as nc
import roi_cases as rc
import roi_fit_cases as fc
import roi_yuv_cases as ryc
import yuvrgb_cases as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
os.environ["IQO_REQUIRE_HIP"] = "1"
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, EUNSUP = -1, -5
METHOD_IDS = ["%s%d" % m for m in fc.METHODS]
W, H = fc.CW, fc.CH
FILLS = (0xA5, 0x5A)
_same = fc.same


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _src(C):
    return torch.from_numpy(rc.frames(C)).to(DEV)


def _yuv_src(layout):
    return torch.from_numpy(ryc.frames(layout)).to(DEV)


def _host(method, degree, C, boxes, rects, dw=W, dh=H, **kw):
    return libiqo_amd.host_resize_rois(method, degree, dw, dh, rc.frames(C), boxes, rects=rects, **kw)


def _run_twice(shape, dtype, view, run, exp, what):
    """`run(out)` on view(buffer) of a buffer filled with 0xA5 bytes, then with 0x5A: both times the canvases equal exp
    and every byte outside them keeps the fill -- a byte nobody wrote fails one of the two runs."""
    for fill in FILLS:
        raw = torch.full((int(np.prod(shape)) * torch.empty((), dtype=dtype).element_size(),), fill, dtype=torch.uint8, device=DEV)
        big = raw.view(dtype).view(shape)
        out = view(big)
        run(out)
        torch.cuda.synchronize(DEV)
        got = out.cpu()
        _same(_bits(got) if dtype != torch.uint8 else got.contiguous().numpy(), exp, "%s fill %#x" % (what, fill))
        out.view(torch.uint8 if dtype == torch.uint8 else {4: torch.int32, 2: torch.int16}[out.element_size()]).fill_(0)
        rest = raw.cpu().numpy()
        assert ((rest == fill) | (rest == 0)).all() and int((rest == 0).sum()) == out.numel() * out.element_size(), what


def _filled_twice(shape, dtype, run, exp, what):
    """_run_twice on an `out` that is the whole buffer: no byte of the result is one that happened to be there."""
    _run_twice(shape, dtype, lambda big: big, run, exp, what)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("method,degree", fc.METHODS, ids=METHOD_IDS)
def test_equals_host_twin(method, degree, C):
    """roi_fit_kernel<LZ, C, false> and <LZ, C, true>: the whole case list in one call, then reversed (the other
    arena, a warm cache)."""
    boxes, rects = fc.cases(method, degree)
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    exp = _host(method, degree, C, boxes, rects, pad=fc.PAD)
    _same(exp, fc.expected(method, degree, C), "twin vs oracle")
    what = "%s-%d C=%d" % (method, degree, C)
    shape = exp.shape
    # (each on a buffer filled with 0xA5, then 0x5A: four calls, so both arenas twice and a warm cache)
    _filled_twice(shape, torch.uint8, lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp, what)
    _filled_twice(shape, torch.uint8, lambda out: r.resize_rois(src, boxes[::-1], out=out, rects=rects[::-1], pad=fc.PAD),
                  exp[::-1], what + " reversed")
    # the float epilogue, the dtype dealt over the cases
    dtype = nc.DTYPES[(C + degree) % 3]
    order = {1: (0, 0, 0), 3: (2, 0, 1), 4: (3, 1)}[C]
    scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
    u8 = fc.expected(method, degree, C)
    bits = nc.expected_bits(u8[..., None] if C == 1 else u8, order, scale, bias, dtype)
    _filled_twice(bits.shape, TORCH_DTYPE[dtype],
                  lambda out: r.resize_rois_normalized(src, boxes, scale, bias, dtype=TORCH_DTYPE[dtype], order=order, out=out,
                                                       rects=rects, pad=fc.PAD), bits, "norm %s %s" % (what, dtype))
    _filled_twice(bits.shape, TORCH_DTYPE[dtype],
                  lambda out: r.resize_rois_normalized(src, boxes[::-1], scale, bias, dtype=TORCH_DTYPE[dtype], order=order,
                                                       out=out, rects=rects[::-1], pad=fc.PAD), bits[::-1],
                  "norm reversed %s %s" % (what, dtype))


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_whole_output_equals_stretch_call(method, degree, C):
    """Rectangle (0, 0, 48, 40), and rects=None: bit for bit RoiResizer(..., 48, 40).resize_rois of the same plan."""
    boxes = [b for b in rc.boxes(method, degree) if method != "lanczos" or fc.accepted(method, degree, b, (0, 0, W, H))]
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    stretch = r.resize_rois(src, boxes).cpu().numpy()
    _same(r.resize_rois(src, boxes, rects=[(0, 0, W, H)] * len(boxes), pad=7).cpu().numpy(), stretch, "whole rectangle")
    _same(r.resize_rois(src, boxes, pad=7).cpu().numpy(), stretch, "no rectangles")
    _same(r.resize_rois(src, boxes).cpu().numpy(), stretch, "the stretch call after fit calls on its plan")


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_agrees_with_per_box_resizers(method, degree, C):
    """Each box by a per-shape resizer (w, h) -> (iw, ih) through offset pointers into a pre-filled canvas."""
    boxes, rects = fc.cases(method, degree)
    src = _src(C)
    got = libiqo_amd.RoiResizer(method, degree, W, H, channels=C).resize_rois(src, boxes, rects=rects, pad=fc.PAD).cpu().numpy()
    tail = (C,) if C > 1 else ()
    for i, (b, (ox, oy, iw, ih)) in enumerate(zip(boxes, rects)):
        f, x, y, w, h = b[:5]
        one = torch.empty((H, W) + tail, dtype=torch.uint8, device=DEV)
        one[...] = torch.tensor(fc.PAD[:C], dtype=torch.uint8, device=DEV) if C > 1 else fc.PAD[0]
        p = libiqo_amd.make_resizer(method, degree, w, h, iw, ih, 1, channels=C)
        p.resize_device(1, src.stride(1), src.stride(0), src.data_ptr() + f * src.stride(0) + y * src.stride(1) + x * C,
                        W * C, H * W * C, one.data_ptr() + (oy * W + ox) * C, torch.cuda.current_stream(DEV))
        exp = one.cpu().numpy()
        if len(b) == 6 and b[5]:
            exp[oy:oy + ih, ox:ox + iw] = exp[oy:oy + ih, ox:ox + iw][:, ::-1].copy()
        _same(got[i], exp, "box %d %s -> %s" % (i, b, rects[i]))


@pytest.mark.parametrize("layout", ryc.LAYOUTS)
@pytest.mark.parametrize("method,degree", fc.METHODS, ids=METHOD_IDS)
def test_yuv_equals_host_twin(method, degree, layout):
    """roi_yuv_fit_kernel<LZ, UV2, false> and <LZ, UV2, true>."""
    boxes, rects = fc.cases(method, degree, True)
    std = ryc.STANDARD[(method, degree)]
    exp = fc.expected_yuv(method, degree, std)
    r = libiqo_amd.YuvRoiResizer(method, degree, W, H, layout=layout)
    src = _yuv_src(layout)
    for order in ("rgb", "bgra"):
        host = libiqo_amd.host_resize_rois_yuv(method, degree, W, H, ryc.frames(layout), boxes, ryc.FW, ryc.FH, layout=layout,
                                               standard=std, order=order, rects=rects, pad=fc.PAD[:3])
        _same(host, yr.reorder(exp, yr.ORDERS[order]), "twin vs oracle " + order)
        got = r.resize_rois_rgb(src, boxes, ryc.FW, ryc.FH, standard=std, order=order, rects=rects, pad=fc.PAD[:3])
        _same(got.cpu().numpy(), host, "%s-%d %s %s" % (method, degree, layout, order))
    back = r.resize_rois_rgb(src, boxes[::-1], ryc.FW, ryc.FH, standard=std, rects=rects[::-1], pad=fc.PAD[:3])
    _same(back.cpu().numpy(), exp[::-1], "reversed")
    dtype = nc.DTYPES[(degree + len(layout)) % 3]
    planes, scale, bias = (2, 0, 1), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
    gotn = r.resize_rois_normalized(src, boxes, ryc.FW, ryc.FH, scale, bias, standard=std, dtype=TORCH_DTYPE[dtype],
                                    order=planes, rects=rects, pad=fc.PAD[:3])
    _same(_bits(gotn), nc.expected_bits(exp, planes, scale, bias, dtype), "norm %s-%d %s %s" % (method, degree, layout, dtype))


@pytest.mark.parametrize("layout", ryc.LAYOUTS)
@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_yuv_agrees_with_full_chroma_resizers(method, degree, layout):
    """Independently of the twin: a box by Nv12Resizer / Yuv420Resizer(chroma="full").resize_rgb of the cropped frame
    at (iw, ih)."""
    boxes, rects = fc.cases(method, degree, True)
    std = ryc.STANDARD[(method, degree)]
    got = libiqo_amd.YuvRoiResizer(method, degree, W, H, layout=layout).resize_rois_rgb(
        _yuv_src(layout), boxes, ryc.FW, ryc.FH, standard=std, rects=rects, pad=fc.PAD[:3]).cpu().numpy()
    y, u, v = ryc.planes()
    cls = libiqo_amd.Nv12Resizer if layout == "nv12" else libiqo_amd.Yuv420Resizer
    for i in (0, 1, 4, 5, len(boxes) - 2):
        b, (ox, oy, iw, ih) = boxes[i], rects[i]
        f, x, yy, w, h = b[:5]
        crop = ryc.frames_of(y[f:f + 1, yy:yy + h, x:x + w], u[f:f + 1, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2],
                             v[f:f + 1, yy // 2:(yy + h) // 2, x // 2:(x + w) // 2], layout)
        inner = cls(method, degree, w, h, iw, ih, chroma="full").resize_rgb(torch.from_numpy(crop).to(DEV),
                                                                            standard=std).cpu().numpy()[0]
        _same(got[i], fc.canvas(inner, rects[i], fc.PAD, len(b) == 6 and b[5]), "box %d %s -> %s" % (i, b, rects[i]))


@pytest.mark.parametrize("C", rc.CHANNELS)
def test_strided_destination_written_once(C):
    method, degree = "lanczos", 2
    boxes, rects = fc.cases(method, degree)
    N, tail = len(boxes), ((C,) if C > 1 else ())
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    exp = _host(method, degree, C, boxes, rects, pad=fc.PAD)
    _run_twice((N, H + 3, W + 5) + tail, torch.uint8, lambda big: big[:, :H, :W],
               lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp, "U8 C=%d" % C)
    order = {1: (0, 0, 0), 3: (2, 0, 1), 4: (3, 1)}[C]
    scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
    for dtype in nc.DTYPES:
        expn = _host(method, degree, C, boxes, rects, pad=fc.PAD, scale=scale, bias=bias, dtype=dtype, order=order)
        expn = expn.view(np.int32 if dtype == "float32" else np.int16)
        # fp16 / bf16: an odd element offset and an odd row pitch
        _run_twice((N, len(order), H + 2, W + 3), TORCH_DTYPE[dtype], lambda big: big[:, :, 1:H + 1, 1:W + 1],
                   lambda out: r.resize_rois_normalized(src, boxes, scale, bias, dtype=TORCH_DTYPE[dtype], order=order, out=out,
                                                        rects=rects, pad=fc.PAD), expn, "%s C=%d" % (dtype, C))


@pytest.mark.parametrize("layout", ryc.LAYOUTS)
def test_yuv_strided_destination_written_once(layout):
    method, degree = "area", 0
    boxes, rects = fc.cases(method, degree, True)
    std, N = ryc.STANDARD[(method, degree)], len(boxes)
    src = _yuv_src(layout)
    r = libiqo_amd.YuvRoiResizer(method, degree, W, H, layout=layout)
    exp = fc.expected_yuv(method, degree, std)
    for order in ("bgr", "rgba"):
        C = len(yr.ORDERS[order])
        _run_twice((N, H + 3, W + 5, C), torch.uint8, lambda big: big[:, :H, :W],
                   lambda out: r.resize_rois_rgb(src, boxes, ryc.FW, ryc.FH, standard=std, order=order, out=out, rects=rects,
                                                 pad=fc.PAD[:3]), yr.reorder(exp, yr.ORDERS[order]), "%s %s" % (layout, order))
    scale, bias = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
    for dtype in ("float16", "float32"):
        _run_twice((N, 3, H + 2, W + 3), TORCH_DTYPE[dtype], lambda big: big[:, :, 1:H + 1, 1:W + 1],
                   lambda out: r.resize_rois_normalized(src, boxes, ryc.FW, ryc.FH, scale, bias, standard=std,
                                                        dtype=TORCH_DTYPE[dtype], out=out, rects=rects, pad=fc.PAD[:3]),
                   nc.expected_bits(exp, (0, 1, 2), scale, bias, dtype), "%s %s" % (layout, dtype))


def test_pad_stores_at_every_destination_misalignment():
    """C = 3 U8: the destination's base and its row stride at every misalignment 0 .. 15 of the 16-byte stores."""
    method, degree, C = "area", 0, 3
    boxes, rects = fc.cases(method, degree)
    boxes, rects = boxes[1:5], rects[1:5]   # letterbox, pillarbox, four sides, flipped
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    exp = _host(method, degree, C, boxes, rects, pad=fc.PAD)
    N = len(boxes)
    for k in range(16):
        rowSt = W * C + k                     # (48 * 3 = 144 is a multiple of 16)
        roiSt = rowSt * H + 5
        _run_twice((64 + N * roiSt,), torch.uint8,
                   lambda flat: flat.as_strided((N, H, W, C), (roiSt, rowSt, C, 1), 16 + k),
                   lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp, "misalignment %d" % k)


@pytest.mark.parametrize("C", rc.CHANNELS)
def test_pad_stores_at_every_rectangle_offset(C):
    """ox * C mod 16 over 0 .. 15 (C = 3: ox = 0 .. 15; C = 1 and 4: every value they reach), the run right of the
    rectangle at as many."""
    method, degree = "lanczos", 3
    rects = [(ox, 3 + ox % 5, 17 + ox % 3, 19) for ox in range(17)]
    boxes = [(i % 3, 2 + i, 5, 45, 31, i & 1) for i in range(len(rects))]
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    src, exp = _src(C), _host(method, degree, C, boxes, rects, pad=fc.PAD)
    _filled_twice(exp.shape, torch.uint8, lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp,
                  "C=%d" % C)
    if C == 3:
        assert sorted({(ox * C) % 16 for ox, _, _, _ in rects}) == list(range(16))


def test_pad_workgroups_above_and_below():
    """An 8 x 600 canvas: rectangle (0, 290, 8, 20) has at least three pad workgroups above it (and, with 290 rows on
    either side, as many below); rectangle (0, 100, 8, 20) a different count below than above."""
    method, degree, C, dw, dh = "area", 0, 1, 8, 600
    rects = [(0, 290, 8, 20), (0, 100, 8, 20), (0, 0, 8, 20), (0, 580, 8, 20)]
    boxes = [(0, 3, 5, 16, 40), (1, 7, 9, 16, 40), (2, 0, 0, 8, 20), (0, 9, 9, 16, 40)]
    lay = [libiqo_amd.host_roi_fit_box_layout(method, degree, C, dw, dh, b[3], b[4], rt) for b, rt in zip(boxes, rects)]
    assert lay[0]["pad_above"] >= 3 and lay[0]["pad_below"] >= 3
    assert lay[1]["pad_above"] >= 3 and lay[1]["pad_below"] != lay[1]["pad_above"]
    assert (lay[2]["pad_above"], lay[3]["pad_below"]) == (0, 0)
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, dw, dh, channels=C)
    exp = _host(method, degree, C, boxes, rects, dw, dh, pad=fc.PAD)
    _run_twice((len(boxes), dh + 2, dw + 3), torch.uint8, lambda big: big[:, 1:dh + 1, 2:dw + 2],
               lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp, "8 x 600")
    scale, bias = nc.NORM_SCALE[:1], nc.NORM_BIAS[:1]
    expn = _host(method, degree, C, boxes, rects, dw, dh, pad=fc.PAD, scale=scale, bias=bias, dtype="bfloat16")
    _run_twice((len(boxes), 1, dh + 2, dw + 3), torch.bfloat16, lambda big: big[:, :, 1:dh + 1, 1:dw + 1],
               lambda out: r.resize_rois_normalized(src, boxes, scale, bias, dtype=torch.bfloat16, out=out, rects=rects,
                                                    pad=fc.PAD), expn.view(np.int16), "8 x 600 bf16")


@pytest.mark.parametrize("method,degree", [("lanczos", 2), ("area", 0)], ids=["lanczos2", "area"])
def test_long_pad_runs(method, degree):
    """A 2100 x 12 four-channel canvas with rectangle (700, 4, 700, 4): its pad runs (8400 bytes a row above and below,
    2800 beside) are longer than one 256-thread sweep of 16-byte stores."""
    C, dw, dh = 4, 2100, 12
    boxes, rects = [(1, 0, 30, 160, 4), (2, 0, 60, 160, 4, 1)], [(700, 4, 700, 4), (699, 3, 701, 4)]
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, dw, dh, channels=C)
    exp = _host(method, degree, C, boxes, rects, dw, dh, pad=fc.PAD)
    assert dw * C > 256 * 16
    _run_twice((2, dh + 1, dw + 1, C), torch.uint8, lambda big: big[:, :dh, :dw],
               lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp, "2100 x 12")


@pytest.mark.parametrize("n", (1, 2, 255, 256, 257, 4097))
def test_batch_sizes(n):
    """n boxes into one-pixel rectangles of an 8 x 6 canvas: the box search at every batch size that turns it."""
    method, degree, C, dw, dh = "area", 0, 3, 8, 6
    boxes = [(i % 3, i % 150, (i // 7) % 110, 1 + i % 5, 1 + i % 3, i & 1) for i in range(n)]
    rects = [(i % 8, (i // 8) % 6, 1, 1) for i in range(n)]
    r = libiqo_amd.RoiResizer(method, degree, dw, dh, channels=C)
    src, exp = _src(C), _host(method, degree, C, boxes, rects, dw, dh, pad=fc.PAD)
    _filled_twice(exp.shape, torch.uint8, lambda out: r.resize_rois(src, boxes, out=out, rects=rects, pad=fc.PAD), exp,
                  "n=%d" % n)
    yb = [(i % 3, 2 * (i % 75), 2 * ((i // 7) % 55), 2 + 2 * (i % 3), 2 + 2 * (i % 2), i & 1) for i in range(n)]
    ry = libiqo_amd.YuvRoiResizer(method, degree, dw, dh, layout="nv12")
    ysrc = _yuv_src("nv12")
    expy = libiqo_amd.host_resize_rois_yuv(method, degree, dw, dh, ryc.frames("nv12"), yb, ryc.FW, ryc.FH, rects=rects,
                                           pad=fc.PAD[:3])
    _filled_twice(expy.shape, torch.uint8,
                  lambda out: ry.resize_rois_rgb(ysrc, yb, ryc.FW, ryc.FH, out=out, rects=rects, pad=fc.PAD[:3]), expy,
                  "yuv n=%d" % n)


def test_rejections_launch_nothing():
    method, degree, C = "lanczos", 3, 3
    src = _src(C)
    r = libiqo_amd.RoiResizer(method, degree, W, H, channels=C)
    good, goodr = (0, 1, 3, 64, 48), (0, 0, W, H)
    out = torch.full((3, H, W, C), 0xA5, dtype=torch.uint8, device=DEV)
    for box, rect, status in ((good, (1, 0, W, H), EINVAL), (good, (0, 0, W, 0), EINVAL), (good, (0, -1, 4, 4), EINVAL),
                              ((0, 4, 4, 10, 1), (0, 0, 10, 24), EINVAL), ((0, 0, 0, 160, 120), (0, 0, 1, H), EUNSUP)):
        with pytest.raises(libiqo_amd.IqoError) as e:
            r.resize_rois(src, [good, good, box], out=out, rects=[goodr, goodr, rect], pad=1)
        assert (e.value.status, e.value.bad_roi) == (status, 2)
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_rois(src, [good], rects=[goodr], fit="letterbox")
    ry = libiqo_amd.YuvRoiResizer("linear", 0, W, H)
    with pytest.raises(libiqo_amd.IqoError) as e:   # chroma above 2x, by the rectangle's size
        ry.resize_rois_rgb(_yuv_src("nv12"), [(0, 0, 0, 64, 48), (0, 0, 0, 20, 14)], ryc.FW, ryc.FH,
                           rects=[goodr, (0, 0, 21, 14)])
    assert (e.value.status, e.value.bad_roi) == (EUNSUP, 1)
    # a capturing stream
    dummy = torch.zeros(16, device=DEV)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    status = []
    with torch.cuda.graph(g):
        dummy.add_(1.0)
        try:
            r.resize_rois(src, [good] * 3, out=out, stream=torch.cuda.current_stream(DEV), rects=[goodr] * 3, pad=1)
        except libiqo_amd.IqoError as e:
            status.append(e.status)
    torch.cuda.synchronize(DEV)
    assert status == [EUNSUP]
    assert (out.cpu().numpy() == 0xA5).all()
    # the plan is usable afterwards, and fit="letterbox" is fit_rects
    boxes = [(0, 2, 4, 64, 36), (1, 0, 0, 30, 90, 1)]
    _same(r.resize_rois(src, boxes, fit="letterbox", pad=fc.PAD).cpu().numpy(),
          _host(method, degree, C, boxes, libiqo_amd.fit_rects(boxes, W, H), pad=fc.PAD), "letterbox")
