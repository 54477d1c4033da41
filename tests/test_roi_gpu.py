"""GPU parity of the batched crop-and-resize (iqo_hip_resize_rois_device / RoiResizer): every box of one launch
equals the CPU twin (which tests/test_roi_host.py pins to the Generic oracle) byte for byte, and the existing
per-shape resizers through an offset pointer -- over every method and channel count, the float epilogue, strided
sources and destinations, calls queued back to back on one stream (both arenas, then the first again) and the
rejections.  The frames are 3 x (160 x 120), the output 32 x 24: well under a second each."""
import ctypes
import os

import numpy as np
import pytest

import norm_cases as nc
import roi_cases as rc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
os.environ["IQO_REQUIRE_HIP"] = "1"
SENTINEL = 0xA5
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, EUNSUP = -1, -5
METHOD_IDS = ["%s%d" % m for m in rc.METHODS]


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _host(method, degree, C, boxes, **kw):
    return libiqo_amd.host_resize_rois(method, degree, rc.DW, rc.DH, rc.frames(C), boxes, **kw)


@pytest.mark.parametrize("C", rc.CHANNELS)
@pytest.mark.parametrize("method,degree", rc.METHODS, ids=METHOD_IDS)
def test_equals_host_twin(method, degree, C):
    """The whole case list in one call, then reversed: the second call uses the other arena and a warm cache."""
    boxes = rc.boxes(method, degree)
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    exp = _host(method, degree, C, boxes)
    _same(exp, rc.expected(method, degree, C), "twin vs oracle")
    got = r.resize_rois(src, boxes)
    back = r.resize_rois(src, boxes[::-1])
    _same(got.cpu().numpy(), exp, "%s-%d C=%d" % (method, degree, C))
    _same(back.cpu().numpy(), exp[::-1], "%s-%d C=%d reversed" % (method, degree, C))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("method,degree,C,order", [("lanczos", 3, 3, (2, 0, 1)), ("area", 0, 1, (0, 0, 0)),
                                                   ("linear", 0, 4, (3, 1))], ids=["lz3-rgb-perm", "area-grey3", "lin-rgba"])
def test_normalized_equals_host_twin(method, degree, C, order, dtype):
    boxes = rc.boxes(method, degree)
    scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    got = r.resize_rois_normalized(src, boxes, scale, bias, dtype=TORCH_DTYPE[dtype], order=order)
    assert tuple(got.shape) == (len(boxes), len(order), rc.DH, rc.DW) and got.dtype == TORCH_DTYPE[dtype]
    exp = _host(method, degree, C, boxes, scale=scale, bias=bias, dtype=dtype, order=order)
    u8 = rc.expected(method, degree, C)
    bits = nc.expected_bits(u8[..., None] if C == 1 else u8, order, scale, bias, dtype)
    _same(exp.view(bits.dtype), bits, "twin vs numpy")
    _same(_bits(got), bits, "%s C=%d %s" % (method, C, dtype))


@pytest.mark.parametrize("C", (1, 3))
@pytest.mark.parametrize("method,degree", [("lanczos", 3), ("area", 0)], ids=["lanczos3", "area"])
def test_agrees_with_per_box_resizers(method, degree, C):
    """Each box by an existing resizer of that shape through an offset pointer."""
    boxes = rc.boxes(method, degree)
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    got = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C).resize_rois(src, boxes).cpu().numpy()
    one = torch.empty((rc.DH, rc.DW) + ((C,) if C > 1 else ()), dtype=torch.uint8, device=DEV)
    for i, b in enumerate(boxes):
        f, x, y, w, h = b[:5]
        p = libiqo_amd.make_resizer(method, degree, w, h, rc.DW, rc.DH, 1, channels=C)
        p.resize_device(1, src.stride(1), src.stride(0), src.data_ptr() + f * src.stride(0) + y * src.stride(1) + x * C,
                        rc.DW * C, rc.DH * rc.DW * C, one, torch.cuda.current_stream(DEV))
        exp = one.cpu().numpy()
        _same(got[i], exp[:, ::-1] if len(b) == 6 and b[5] else exp, "box %d %s" % (i, b))


@pytest.mark.parametrize("C", rc.CHANNELS)
def test_strided_source_and_destination(C):
    """A crop view of larger frames (rows no multiple of 4 bytes) is read where it lies; a strided out keeps
    its sentinels."""
    method, degree = "lanczos", 2
    boxes = rc.boxes(method, degree)
    N, tail = len(boxes), ((C,) if C > 1 else ())
    wide = torch.full((rc.FRAMES + 1, rc.FH + 2, rc.FW + 3) + tail, 0x3C, dtype=torch.uint8, device=DEV)
    src = wide[1:, 1:rc.FH + 1, 2:rc.FW + 2]
    src.copy_(torch.from_numpy(rc.frames(C)))
    assert not src.is_contiguous()
    big = torch.full((N, rc.DH + 3, rc.DW + 5) + tail, SENTINEL, dtype=torch.uint8, device=DEV)
    out = big[:, :rc.DH, :rc.DW]
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    assert r.resize_rois(src, boxes, out=out) is out
    exp = _host(method, degree, C, boxes)
    _same(out.cpu().numpy(), exp, "strided C=%d" % C)
    h = big.cpu().numpy()
    mask = np.ones(h.shape, bool)
    mask[:, :rc.DH, :rc.DW] = False
    assert (h[mask] == SENTINEL).all()
    # the float form into a strided view
    order = (0,) * 3 if C == 1 else (2, 1, 0)
    bigf = torch.full((N, 3, rc.DH + 1, rc.DW + 3), -7.5, dtype=torch.float16, device=DEV)
    outf = bigf[:, :, :rc.DH, :rc.DW]
    r.resize_rois_normalized(src, boxes, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], dtype=torch.float16, order=order, out=outf)
    bits = nc.expected_bits(exp[..., None] if C == 1 else exp, order, nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "float16")
    _same(_bits(outf), bits, "strided norm C=%d" % C)
    hf = bigf.cpu().numpy()
    maskf = np.ones(hf.shape, bool)
    maskf[:, :, :rc.DH, :rc.DW] = False
    assert (hf[maskf] == np.float16(-7.5)).all()


def test_queued_calls_on_one_stream():
    """Two and three calls back to back with different boxes, no synchronisation between them: the third refills
    the first arena (after its event)."""
    method, degree, C = "lanczos", 3, 3
    boxes = rc.boxes(method, degree)
    batches = [boxes[:5], boxes[5:], boxes[3:9][::-1]]
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    s = torch.cuda.Stream(DEV)
    s.wait_stream(torch.cuda.current_stream(DEV))
    outs = [torch.zeros((len(b), rc.DH, rc.DW, C), dtype=torch.uint8, device=DEV) for b in batches]
    torch.cuda.synchronize(DEV)
    for n in (2, 3, 3):
        for o in outs:
            o.zero_()
        torch.cuda.synchronize(DEV)
        for b, o in list(zip(batches, outs))[:n]:
            r.resize_rois(src, b, out=o, stream=s)
        s.synchronize()
        for b, o in list(zip(batches, outs))[:n]:
            _same(o.cpu().numpy(), _host(method, degree, C, b), "queued %d" % n)


def test_capturing_stream_is_unsupported():
    method, degree, C = "area", 0, 3
    boxes = rc.boxes(method, degree)
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    out = torch.full((len(boxes), rc.DH, rc.DW, C), SENTINEL, dtype=torch.uint8, device=DEV)
    dummy = torch.zeros(16, device=DEV)
    torch.cuda.synchronize(DEV)
    g = torch.cuda.CUDAGraph()
    status = []
    with torch.cuda.graph(g):
        dummy.add_(1.0)
        try:
            r.resize_rois(src, boxes, out=out, stream=torch.cuda.current_stream(DEV))
        except libiqo_amd.IqoError as e:
            status.append(e.status)
    torch.cuda.synchronize(DEV)
    assert status == [EUNSUP]
    assert (out.cpu().numpy() == SENTINEL).all()
    # the plan is usable afterwards
    _same(r.resize_rois(src, boxes).cpu().numpy(), _host(method, degree, C, boxes), "after the capture")


def test_rejections_launch_nothing():
    method, degree, C = "lanczos", 3, 3
    src = torch.from_numpy(rc.frames(C)).to(DEV)
    r = libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=C)
    good = (0, 1, 3, 64, 48)
    for box, status in (((0, 4, 4, 0, 10), EINVAL), ((0, 150, 4, 11, 10), EINVAL), ((3, 4, 4, 10, 10), EINVAL),
                        ((0, 4, 4, 10, 10, 2), EINVAL), (rc.UNDEFINED[0][2], EINVAL)):
        out = torch.full((3, rc.DH, rc.DW, C), SENTINEL, dtype=torch.uint8, device=DEV)
        with pytest.raises(libiqo_amd.IqoError) as e:
            r.resize_rois(src, [good, good, box], out=out)
        torch.cuda.synchronize(DEV)
        assert (e.value.status, e.value.bad_roi) == (status, 2), str(e.value)
        assert "box 2" in str(e.value)
        assert (out.cpu().numpy() == SENTINEL).all()
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.RoiResizer(method, degree, rc.DW, rc.DH, channels=2)
    assert "(-5)" in str(e.value)
    # an empty batch is fine
    assert tuple(r.resize_rois(src, []).shape) == (0, rc.DH, rc.DW, C)
