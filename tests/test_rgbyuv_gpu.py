"""Packed RGB(A) resize straight to NV12 / I420 on the GPU (_Resizer.resize_nv12 / resize_i420 over
iqo_hip_resize_rgb_nv12_device / iqo_hip_resize_rgb_yuv420_device): the result is, bit for bit, the integer
RGB -> YUV 4:2:0 definition of tests/rgbyuv_cases.py applied to the per-channel oracle's bytes.  Every
rgb_yuv_kernel<C, UV2> instantiation on every shape of rgbyuv_cases.GPU_SHAPES (every method up and down,
the packed_general shape, rows narrower than a thread's 8 pixels, tail stores, odd sizes, a last row
without chroma), both source orders and the four standards; strided and misaligned destinations behind
sentinels; every rejected call; the tight layout handed on to Nv12Resizer / Yuv420Resizer.  Everything is
equality.  Small shapes, 3 frames (noise, pure blue, pure red): well under a second each."""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import packed_cases as pc
import rgbyuv_cases as ry

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENT = 0xA5
EINVAL, EUNSUP = -1, -5  # IQO_HIP_EINVAL, IQO_HIP_EUNSUP
N = ry.N_FRAMES


def _resizer(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    return libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _clamp_occurs(shape, C, order, standard):
    """From the expected value: a full-range row's chroma reaches 256 before the min."""
    _, u, v = ry.expected_planes(shape, C, order, standard, raw=True)
    return u.max() == 256 and v.max() == 256


# ---- 1. every instantiation on every shape, bit-exact

@pytest.mark.parametrize("row", ry.GPU_CASES, ids=ry.gid)
def test_bit_exact(row):
    shape, C, layout, order, standard = row
    exp = ry.expected_frames(row)  # (the oracle runs before anything is launched)
    if standard in ry.FULL_RANGE:
        assert _clamp_occurs(shape, C, order, standard), "the inputs do not reach the upper clamp"
        assert exp.max() == 255
    r = _resizer(shape, C)
    assert r.describe()["kernel"] == ry.first_pass_kernel(shape, C)
    src = torch.from_numpy(ry.frames_for(shape, C, order).copy()).to(DEV)
    fn = r.resize_nv12 if layout == "nv12" else r.resize_i420
    out = fn(src, standard=standard, order=order)
    assert out.dtype == torch.uint8 and tuple(out.shape) == exp.shape
    _same(out.cpu().numpy(), exp, ry.gid(row))
    # by name, one frame, into out=
    one = torch.full((exp.shape[1],), SENT, dtype=torch.uint8, device=DEV)
    got = fn(src[1], standard=ry.NAMES[standard], order=order, out=one)
    assert got is one
    _same(one.cpu().numpy(), exp[1], ry.gid(row) + " frame 1")


# ---- 2. strided destinations at odd byte offsets: nothing outside the planes is written

class Call:
    """The C entries with explicit pointers and strides on LAYOUT_SHAPE."""

    def __init__(self, C, layout, shape=ry.LAYOUT_SHAPE, order="bgr", standard=ry.BT601_FULL):
        self.C, self.layout, self.shape, self.order, self.standard = C, layout, shape, order, standard
        self.r = _resizer(shape, C)
        _, _, self.sw, self.sh, self.dw, self.dh, _ = shape
        self.cw, self.ch = self.dw // 2, self.dh // 2
        self.src = torch.from_numpy(ry.frames_for(shape, C, order).copy()).to(DEV)
        self.uvb = 2 * self.cw if layout == "nv12" else self.cw  # bytes of a chroma row
        self.wsb = libiqo_amd.rgb_yuv_workspace_bytes(self.dw, self.dh, C, N)
        self.ws = torch.empty((self.wsb,), dtype=torch.uint8, device=DEV)

    def __call__(self, st_y, st_uv, frame_st, y, u, v=None, n=N, plan="own", src="own", src_st=None, standard=None,
                 order="own", ws="own", wsb=None, stream=None):
        L = libiqo_amd.lib()
        o = (ctypes.c_int * 3)(*ry.ORDERS[self.order]) if order == "own" else (
            None if order is None else (ctypes.c_int * 3)(*order))
        head = (self.r._plan if plan == "own" else plan, n, self.sw * self.C if src_st is None else src_st,
                self.sw * self.sh * self.C, self.src.data_ptr() if src == "own" else src,
                self.standard if standard is None else standard, o, st_y, st_uv, frame_st)
        tail = (self.ws.data_ptr() if ws == "own" else ws, self.wsb if wsb is None else wsb, stream)
        if self.layout == "nv12":
            return L.iqo_hip_resize_rgb_nv12_device(*head, y, u, *tail)
        return L.iqo_hip_resize_rgb_yuv420_device(*head, y, u, v, *tail)

    def planes(self):
        return ry.expected_planes(self.shape, self.C, self.order, self.standard)


@pytest.mark.parametrize("C,layout", ry.COMBOS, ids=lambda v: str(v))
def test_strided_misaligned_destinations(C, layout):
    c = Call(C, layout)
    dw, dh, cw, ch = c.dw, c.dh, c.cw, c.ch
    st_y, st_uv = dw + 3, c.uvb + 5
    # one frame: Y at an odd offset, a gap, then the chroma plane(s), each at an odd offset
    off_y = 1
    off_u = off_y + dh * st_y + 6
    off_u += 1 - off_u % 2
    off_v = off_u + ch * st_uv + 8
    off_v += 1 - off_v % 2
    end = (off_v + ch * st_uv) if layout == "i420" else (off_u + ch * st_uv)
    frame_st = end + 11
    G = 64
    buf = torch.full((64 + G + N * frame_st + G,), SENT, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 64 + G  # a 64-byte boundary: the plane offsets above are odd
    p = buf.data_ptr() + base
    assert (p + off_y) % 2 == 1 and (p + off_u) % 2 == 1 and (p + off_v) % 2 == 1
    assert c(st_y, st_uv, frame_st, p + off_y, p + off_u, p + off_v if layout == "i420" else None) == 0
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    payload = np.zeros(full.shape, bool)
    y, u, v = c.planes()
    gy, gu, gv = np.empty_like(y), np.empty_like(u), np.empty_like(v)
    for f in range(N):
        fb = base + f * frame_st
        for r in range(dh):
            o = fb + off_y + r * st_y
            payload[o:o + dw] = True
            gy[f, r] = full[o:o + dw]
        for r in range(ch):
            o = fb + off_u + r * st_uv
            payload[o:o + c.uvb] = True
            if layout == "nv12":
                gu[f, r], gv[f, r] = full[o:o + 2 * cw:2], full[o + 1:o + 2 * cw:2]
            else:
                gu[f, r] = full[o:o + cw]
                o = fb + off_v + r * st_uv
                payload[o:o + cw] = True
                gv[f, r] = full[o:o + cw]
    what = "c%d-%s" % (C, layout)
    _same(gy, y, what + " Y")
    _same(gu, u, what + " U")
    _same(gv, v, what + " V")
    stray = np.flatnonzero(~payload & (full != SENT))
    assert stray.size == 0, (what, "wrote outside the planes at byte offsets (from the base)", (stray[:8] - base).tolist())


# ---- 3. rejected calls: the status, and nothing written

def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst == SENT).all())


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_rejected_calls(layout):
    c = Call(3, layout)
    dw, dh, cw, ch, uvb = c.dw, c.dh, c.cw, c.ch, c.uvb
    frame = dw * dh + 2 * cw * ch
    dst = torch.full((N * frame + 64,), SENT, dtype=torch.uint8, device=DEV)
    y = dst.data_ptr()
    u = y + dw * dh
    v = u + cw * ch if layout == "i420" else None
    good = (dw, uvb, frame, y, u, v)
    big = 1 << 31
    cases = {
        "null plan": c(*good, plan=None),
        "null source": c(*good, src=None),
        "null Y": c(dw, uvb, frame, None, u, v),
        "null chroma": c(dw, uvb, frame, y, None, v),
        "null workspace": c(*good, ws=None),
        "null order": c(*good, order=None),
        "standard -1": c(*good, standard=-1),
        "standard 4": c(*good, standard=4),
        "order 3 with 3 channels": c(*good, order=(0, 1, 3)),
        "order -1": c(*good, order=(-1, 1, 2)),
        "order with R = G": c(*good, order=(1, 1, 2)),
        "order with R = B": c(*good, order=(2, 1, 2)),
        "order with G = B": c(*good, order=(0, 2, 2)),
        "Y stride < dstW": c(dw - 1, uvb, frame, y, u, v),
        "chroma stride < its row": c(dw, uvb - 1, frame, y, u, v),
        "chroma begins inside Y": c(dw, uvb, frame, y, u - 1, v),
        "Y begins inside chroma": c(dw, uvb, frame, u + 1, u, v, n=1),
        "frame stride one byte short": c(dw, uvb, frame - 1, y, u, v),
        "frame stride 0": c(dw, uvb, 0, y, u, v),
        "Y stride of 2^31": c(big, uvb, 1 << 40, y, y + (1 << 36), None if v is None else y + (1 << 37), n=1),
        "chroma stride of 2^31": c(dw, big, 1 << 40, y, y + (1 << 36), None if v is None else y + (1 << 38), n=1),
        "Y plane of 2^31 bytes": c(big // (dh - 1) + 1, uvb, 1 << 40, y, y + (1 << 36),
                                   None if v is None else y + (1 << 37), n=1),
        "source stride < its row": c(*good, src_st=c.sw * 3 - 1),
        "source stride of 2^24": c(*good, src_st=1 << 24),
        "workspace one byte short": c(*good, wsb=c.wsb - 1),
        "workspace of two frames": c(*good, wsb=libiqo_amd.rgb_yuv_workspace_bytes(dw, dh, 3, N - 1)),
    }
    if layout == "i420":
        cases["null V"] = c(dw, uvb, frame, y, u, None)
        cases["V begins inside U"] = c(dw, uvb, frame, y, u, v - 1)
        cases["V = U"] = c(dw, uvb, frame, y, u, u)
    assert {k: s for k, s in cases.items() if s != EINVAL} == {}
    # plans without R, G, B: planar and 2 channels
    m, d, sw, sh, _, _, px = c.shape
    for C in (1, 2):
        other = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)
        assert c(*good, plan=other._plan) == EUNSUP, C
    assert _untouched(dst)
    # the same destination is accepted: one frame needs no frame stride, four channels take order 3
    assert c(dw, uvb, 0, y, u, v, n=1) == 0
    torch.cuda.synchronize()
    _same(dst[:frame].cpu().numpy(), ry.tight(layout, *c.planes())[0], layout + " after the errors")
    assert (dst[frame:] == SENT).all()
    c4 = Call(4, layout)
    assert c4(*good, order=(3, 1, 0)) == 0
    assert c4(*good, order=(4, 1, 0)) == EINVAL
    torch.cuda.synchronize()


@pytest.mark.parametrize("dims", [(1, 4), (4, 1)], ids=["dstW1", "dstH1"])
def test_rejects_outputs_below_two_pixels(dims):
    dw, dh = dims
    r = libiqo_amd.AreaResizer(16, 16, dw, dh, channels=3)
    src = torch.zeros((1, 16, 16, 3), dtype=torch.uint8, device=DEV)
    dst = torch.full((64,), SENT, dtype=torch.uint8, device=DEV)
    wsb = libiqo_amd.rgb_yuv_workspace_bytes(dw, dh, 3, 1)
    ws = torch.empty((wsb,), dtype=torch.uint8, device=DEV)
    L = libiqo_amd.lib()
    o = (ctypes.c_int * 3)(0, 1, 2)
    p = dst.data_ptr()
    head = (r._plan, 1, 48, 768, src.data_ptr(), 0, o, dw, 2, 0)
    assert L.iqo_hip_resize_rgb_nv12_device(*head, p, p + 16, ws.data_ptr(), wsb, None) == EINVAL
    assert L.iqo_hip_resize_rgb_yuv420_device(*head, p, p + 16, p + 32, ws.data_ptr(), wsb, None) == EINVAL
    assert _untouched(dst)


def test_python_errors():
    shape = ry.LAYOUT_SHAPE
    m, d, sw, sh, dw, dh, px = shape
    E = libiqo_amd.IqoError
    r = _resizer(shape, 3)
    src = torch.from_numpy(ry.frames_for(shape, 3, "rgb").copy()).to(DEV)
    nbytes = dw * dh + 2 * (dw // 2) * (dh // 2)
    out = torch.full((N, nbytes), SENT, dtype=torch.uint8, device=DEV)
    for fn in (r.resize_nv12, r.resize_i420):
        for kw in (dict(order="gbr"), dict(order="rgba"), dict(order=(0, 1, 2)), dict(standard="bt2020"),
                   dict(standard=7), dict(out=out[:2]), dict(out=out[:, :-1]), dict(out=out.to(torch.int8)),
                   dict(out=torch.full((N, 2 * nbytes), SENT, dtype=torch.uint8, device=DEV)[:, ::2])):
            with pytest.raises(E):
                fn(src, **{"out": out, **kw})
        with pytest.raises(E):
            fn(src[:, :-1], out=out)
        with pytest.raises(E):
            fn(src[..., :2], out=out)
    planar = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px)
    two = _resizer(shape, 2)
    for other, s in ((planar, src[..., 0].contiguous()), (two, src[..., :2].contiguous())):
        for name in ("resize_nv12", "resize_i420"):
            with pytest.raises(E):
                getattr(other, name)(s, out=out)
    assert _untouched(out)
    r.resize_nv12(src, standard=ry.BT709_LIMITED, out=out)
    _same(out.cpu().numpy(), ry.tight("nv12", *ry.expected_planes(shape, 3, "rgb", ry.BT709_LIMITED)), "after the errors")


# ---- 4. a side stream after prepare(), the workspace kept per stream

def test_side_stream():
    row = ry.GPU_CASES[2]  # C = 4, NV12
    shape, C, layout, order, standard = row
    assert (C, layout) == (4, "nv12")
    exp = ry.expected_frames(row)
    r = _resizer(shape, C)
    r.prepare()  # as before a graph capture: no upload inside the calls
    src = torch.from_numpy(ry.frames_for(shape, C, order).copy()).to(DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    with torch.cuda.stream(stream):
        a = r.resize_nv12(src, standard=standard, order=order, stream=stream)
        b = r.resize_nv12(src[:1], standard=standard, order=order, stream=stream)
    c = r.resize_nv12(src, standard=standard, order=order)
    stream.synchronize()
    torch.cuda.synchronize()
    _same(a.cpu().numpy(), exp, "side stream")
    _same(b.cpu().numpy(), exp[:1], "side stream, one frame")
    _same(c.cpu().numpy(), exp, "default stream")
    assert len(r._ws) == 2


# ---- 5. layout: the tight output is what Nv12Resizer / Yuv420Resizer.resize_frames take

@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_output_feeds_the_yuv_resizers(layout):
    shape = ("area", 0, 80, 48, 48, 24, 1)
    m, d, sw, sh, dw, dh, px = shape
    dw2, dh2 = 24, 12
    order, standard, C = "rgb", ry.BT709_LIMITED, 3
    y, u, v = ry.expected_planes(shape, C, order, standard)
    r = _resizer(shape, C)
    src = torch.from_numpy(ry.frames_for(shape, C, order).copy()).to(DEV)
    if layout == "nv12":
        mid = r.resize_nv12(src, standard=standard, order=order)
        out = libiqo_amd.Nv12Resizer(m, d, dw, dh, dw2, dh2).resize_frames(mid)
    else:
        mid = r.resize_i420(src, standard=standard, order=order)
        out, _ = libiqo_amd.Yuv420Resizer(m, d, dw, dh, dw2, dh2).resize_frames(mid)
    _same(mid.cpu().numpy(), ry.tight(layout, y, u, v), layout + " handed on")

    def small(plane, w, h):
        return np.stack([ol.run_oracle(m, d, w, h, w // 2, h // 2, 1, np.ascontiguousarray(p)) for p in plane])

    exp = ry.tight(layout, small(y, dw, dh), small(u, dw // 2, dh // 2), small(v, dw // 2, dh // 2))
    _same(out.cpu().numpy(), exp, layout + " resized again")
