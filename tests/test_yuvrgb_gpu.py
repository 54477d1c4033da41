"""NV12 / I420 resize straight to RGB bytes or normalised RGB tensors on the GPU
(Nv12Resizer / Yuv420Resizer .resize_rgb and .resize_normalized over iqo_hip_resize_nv12_rgb_device and
its three siblings): the result is, bit for bit, the integer YUV -> RGB definition of
tests/yuvrgb_cases.py applied to the per-plane oracle's bytes, and norm_cases.expected_bits of those for
the float forms.  Every fused I420 instantiation, both UV kernels of NV12, the shapes at which
yuv_rgb_kernel can go wrong (rows narrower than a thread's 8 pixels, tail stores, odd sizes), padded
and misaligned destinations, byte orders and plane picks, the error returns, a side stream with a
strided out=, and the untouched plane resizes.  Bit patterns are compared, never allclose.  Small
shapes, 5 frames (two of them flat patches that reach every clamp): well under a second each."""
import ctypes

import numpy as np
import pytest

import norm_cases as nc
import yuv_cases as yc
import yuvrgb_cases as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENT = 0xA5
EINVAL = -1
N = yr.N_FRAMES
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SCALE, BIAS = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
RGB = (0, 1, 2)

# the single shapes of the layout, order, stream, error and tie tests
LAYOUT_NV12 = yr.NV12_CASES[0]                                         # Lanczos-3 64x32 -> 33x17: odd x odd
LAYOUT_I420 = next(r for r in yr.I420_CASES if r[0][6] == "lin_d2")    # Linear 128x16 -> 64x8, fused
TIE_I420 = next(r for r in yr.I420_CASES if r[0][6] == "lz_sym10")


class Setup:
    """A resizer, its source frames on the device and the expected RGB bytes [5, dh, dw, 3] (the plan is
    built and the oracle run before anything is launched)."""

    def __init__(self, kind, row):
        self.kind = kind
        if kind == "nv12":
            shape, self.standard = row
            self.case = yr.nv12_case(shape)
            frames = yr.nv12_frames(self.case)
        else:
            self.case, self.standard = row
            frames = yr.i420_frames(self.case)
        m, d, sw, sh, dw, dh, self.label = self.case
        self.dw, self.dh = dw, dh
        cls = libiqo_amd.Nv12Resizer if kind == "nv12" else libiqo_amd.Yuv420Resizer
        self.r = cls(m, d, sw, sh, dw, dh)
        self.rgb = yr.expected_rgb(self.case, self.standard)
        self.src = torch.from_numpy(frames).to(DEV)
        self.what = (kind, yc.cid(self.case), yr.NAMES[self.standard])

    def bits(self, dtype, order=RGB, scale=SCALE, bias=BIAS):
        return nc.expected_bits(self.rgb, order, scale, bias, dtype)

    def check_fused(self):
        if self.kind == "i420":
            assert self.r.last_fused == (self.label != "none"), self.what

    # the C ABI with explicit strides and pointers
    def call_rgb(self, C, order, row_st, frame_st, dst, ws, ws_bytes, n=N, stream=None, standard=None, src_args=None):
        o = None if order is None else (ctypes.c_int * 4)(*(tuple(order) + (0,) * (4 - len(order))))
        L = libiqo_amd.lib()
        a = list(src_args or self.r._src_args(self.src))
        a[1] = n
        cs = self.standard if standard is None else standard
        if self.kind == "nv12":
            return L.iqo_hip_resize_nv12_rgb_device(*a, cs, C, o, row_st, frame_st, dst, ws, ws_bytes, stream)
        return L.iqo_hip_resize_yuv420_rgb_device(*a, cs, C, o, row_st, frame_st, dst, ws, ws_bytes, stream, None)

    def call_norm(self, norm, row_st, plane_st, frame_st, dst, ws, ws_bytes, n=N, stream=None, standard=None,
                  src_args=None):
        L = libiqo_amd.lib()
        a = list(src_args or self.r._src_args(self.src))
        a[1] = n
        cs = self.standard if standard is None else standard
        nm = None if norm is None else ctypes.byref(norm)
        if self.kind == "nv12":
            return L.iqo_hip_resize_nv12_norm_device(*a, cs, nm, row_st, plane_st, frame_st, dst, ws, ws_bytes, stream)
        return L.iqo_hip_resize_yuv420_norm_device(*a, cs, nm, row_st, plane_st, frame_st, dst, ws, ws_bytes, stream,
                                                   None)

    def workspace(self, n=N):
        nbytes = libiqo_amd.yuv_rgb_workspace_bytes(self.dw, self.dh, n)
        return torch.empty((nbytes,), dtype=torch.uint8, device=DEV), nbytes


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _norm_struct(dtype, order, scale, bias):
    n = libiqo_amd.Norm(nc.CODE[dtype], len(order))
    for i, (c, s, b) in enumerate(zip(order, scale, bias)):
        n.order[i], n.scale[i], n.bias[i] = c, s, b
    return n


# ---- 1. I420: every fused instantiation and "none", bytes and fp32

@pytest.mark.parametrize("row", yr.I420_CASES, ids=yr.iid)
def test_i420_every_label(row):
    s = Setup("i420", row)
    out = s.r.resize_rgb(s.src, standard=s.standard)
    s.check_fused()
    assert out.dtype == torch.uint8 and tuple(out.shape) == (N, s.dh, s.dw, 3)
    _same(out.cpu().numpy(), s.rgb, s.what + ("rgb",))
    out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=yr.NAMES[s.standard])
    s.check_fused()
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, 3, s.dh, s.dw)
    _same(_bits(out), s.bits("float32"), s.what + ("float32",))


# ---- 2. NV12: the kernel's edge shapes through both UV kernels

@pytest.mark.parametrize("row", yr.NV12_CASES, ids=yr.nid)
def test_nv12_shapes_both_uv_kernels(row):
    s = Setup("nv12", row)
    shape = row[0]
    m, d, sw, sh, dw, dh = shape
    default = libiqo_amd.host_packed_kernel_for(m, d, 2, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1)
    half = "float16" if yr.NV12_CASES.index(row) % 2 == 0 else "bfloat16"
    for force, name in ((0, default), (1, "packed_general")):
        s.r.set_option("force_general", force, plane=1)
        assert s.r.describe()[1] == name
        out = s.r.resize_rgb(s.src, standard=s.standard)
        _same(out.cpu().numpy(), s.rgb, s.what + (name, "rgb"))
        for dtype in ("float32", half):
            out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=TORCH_DTYPE[dtype])
            assert out.dtype == TORCH_DTYPE[dtype] and tuple(out.shape) == (N, 3, dh, dw)
            _same(_bits(out), s.bits(dtype), s.what + (name, dtype))


# ---- 3. layouts: base one element past a 64-byte boundary, padded rows, planes and frames, guards

LAYOUT_ROWS = [("nv12", LAYOUT_NV12), ("i420", LAYOUT_I420)]
G = 64


def _buffer(nbytes, e):
    buf = torch.full((64 + G + e + nbytes + G,), SENT, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 64 + G + e  # one element past a 64-byte boundary
    assert (buf.data_ptr() + base - e) % 64 == 0
    return buf, base


def _check_outside(full, payload, base, e, nbytes, what):
    stray = np.flatnonzero(~payload & (full != SENT))
    assert stray.size == 0, (what, "wrote outside the payload at byte offsets (from the base)", (stray[:8] - base).tolist())
    assert payload[:base].sum() == 0 and (full[base - e - G:base] == SENT).all()
    assert (full[base + nbytes:base + nbytes + G] == SENT).all()


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_rgb_padded_misaligned_layout(kind, row, C):
    s = Setup(kind, row)
    dw, dh = s.dw, s.dh
    order = yr.ORDERS["rgb" if C == 3 else "bgra"]
    row_st = dw * C + 1
    frame_st = dh * row_st + 5
    buf, base = _buffer(N * frame_st, 1)
    ws, wsb = s.workspace()
    assert s.call_rgb(C, order, row_st, frame_st, buf.data_ptr() + base, ws.data_ptr(), wsb) == 0
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    payload = np.zeros(full.shape, bool)
    got = np.empty((N, dh, dw, C), np.uint8)
    for f in range(N):
        for y in range(dh):
            o = base + f * frame_st + y * row_st
            payload[o:o + dw * C] = True
            got[f, y] = full[o:o + dw * C].reshape(dw, C)
    _same(got, yr.reorder(s.rgb, order), s.what + (C,))
    _check_outside(full, payload, base, 1, N * frame_st, s.what + (C,))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_norm_padded_misaligned_layout(kind, row, dtype):
    s = Setup(kind, row)
    dw, dh, e, P = s.dw, s.dh, nc.ELEM[dtype], 3
    row_st = (dw + 1) * e
    plane_st = dh * row_st + 3 * e
    frame_st = P * plane_st + 5 * e
    buf, base = _buffer(N * frame_st, e)
    ws, wsb = s.workspace()
    rc = s.call_norm(_norm_struct(dtype, RGB, SCALE, BIAS), row_st, plane_st, frame_st, buf.data_ptr() + base,
                     ws.data_ptr(), wsb)
    assert rc == 0
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    payload = np.zeros(full.shape, bool)
    got = np.empty((N, P, dh, dw), np.int32 if e == 4 else np.int16)
    for f in range(N):
        for p in range(P):
            for y in range(dh):
                o = base + f * frame_st + p * plane_st + y * row_st
                payload[o:o + dw * e] = True
                got[f, p, y] = full[o:o + dw * e].view(got.dtype)
    _same(got, s.bits(dtype), s.what + (dtype,))
    _check_outside(full, payload, base, e, N * frame_st, s.what + (dtype,))


# ---- 4. orders and planes (frame 2 is the constant frame (16, 128, 235), frames 3 and 4 are flat patches:
# a wrong pick shows as cross-talk)

@pytest.mark.parametrize("order", sorted(yr.ORDERS))
@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_rgb_orders(kind, row, order):
    s = Setup(kind, row)
    out = s.r.resize_rgb(s.src, standard=s.standard, order=order)
    C = len(yr.ORDERS[order])
    assert tuple(out.shape) == (N, s.dh, s.dw, C)
    got = out.cpu().numpy()
    _same(got, yr.reorder(s.rgb, yr.ORDERS[order]), s.what + (order,))
    if C == 4:
        assert (got[..., 3] == 255).all()


FLOAT_ORDERS = [
    ((2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]),
    ((1,), nc.NORM_SCALE[3:4], nc.NORM_BIAS[3:4]),
    ((0, 0, 0), nc.NORM_SCALE[:3], (nc.NORM_BIAS[2], nc.NORM_BIAS[0], nc.NORM_BIAS[3])),  # one channel, three maps
]


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("case", FLOAT_ORDERS, ids=lambda c: "order" + "".join(map(str, c[0])))
@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_norm_order_and_planes(kind, row, case, dtype):
    order, scale, bias = case
    assert len({(a, b) for a, b in zip(scale, bias)}) == len(order)
    s = Setup(kind, row)
    P = len(order)
    big = torch.empty((N, P + 1, s.dh, s.dw), dtype=TORCH_DTYPE[dtype], device=DEV)  # a sentinel plane behind
    big.view(torch.uint8).fill_(SENT)
    out = s.r.resize_normalized(s.src, scale, bias, standard=s.standard, dtype=TORCH_DTYPE[dtype], order=order,
                                out=big[:, :P])
    assert out.data_ptr() == big.data_ptr() and tuple(out.shape) == (N, P, s.dh, s.dw)
    torch.cuda.synchronize()
    _same(_bits(big[:, :P]), s.bits(dtype, order, scale, bias), s.what + (order, dtype))
    assert (big[:, P].contiguous().view(torch.uint8) == SENT).all(), s.what + (order, dtype, "sentinel plane")


# ---- 5. the two-rounding epilogue: the expected bits differ from a fused multiply-add's on these inputs

@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_norm_is_two_roundings_not_an_fma(kind, row):
    s = Setup(kind, row)
    two = s.bits("float32")
    one = np.stack([nc.fma_f32(s.rgb[..., c], SCALE[c], BIAS[c]) for c in range(3)], axis=1).view(np.int32)
    assert all((two[:, c] != one[:, c]).any() for c in range(3)), "the inputs do not tell the two forms apart"
    out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard)
    _same(_bits(out), two, s.what)


# ---- 6. errors: rejected on the host before any launch, the destination untouched

def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst == SENT).all())


@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_rgb_abi_errors(kind, row):
    s = Setup(kind, row)
    dw, dh, C = s.dw, s.dh, 3
    dst = torch.full((N * dh * dw * 4 + 64,), SENT, dtype=torch.uint8, device=DEV)
    ws, wsb = s.workspace()
    rs, fs, d, w = dw * C, dh * dw * C, dst.data_ptr(), ws.data_ptr()
    good = s.r._src_args(s.src)

    def src(i, v):
        a = list(good)
        a[i] = v
        return a

    cases = {
        "null plan": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(0, None)),
        "null Y": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(5, None)),
        "null chroma": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(6, None)),
        "null destination": s.call_rgb(C, RGB, rs, fs, None, w, wsb),
        "null workspace": s.call_rgb(C, RGB, rs, fs, d, None, wsb),
        "null order": s.call_rgb(C, None, rs, fs, d, w, wsb),
        "standard -1": s.call_rgb(C, RGB, rs, fs, d, w, wsb, standard=-1),
        "standard 4": s.call_rgb(C, RGB, rs, fs, d, w, wsb, standard=4),
        "channels 2": s.call_rgb(2, RGB, rs, fs, d, w, wsb),
        "channels 5": s.call_rgb(5, (0, 1, 2, 3), 5 * dw, 5 * dw * dh, d, w, wsb),
        "order 4": s.call_rgb(C, (0, 4, 2), rs, fs, d, w, wsb),
        "order -1": s.call_rgb(C, (0, 1, -1), rs, fs, d, w, wsb),
        "order[3] = 4 with 4 channels": s.call_rgb(4, (0, 1, 2, 4), 4 * dw, 4 * dw * dh, d, w, wsb),
        "row stride < dstW * channels": s.call_rgb(C, RGB, rs - 1, fs, d, w, wsb),
        "frame stride < dstH * row stride": s.call_rgb(C, RGB, rs, fs - 1, d, w, wsb),
        "Y stride < srcW": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(2, good[2] - 1)),
        "chroma stride < its row": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(3, good[3] - 1)),
        "Y stride of 2^24": s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(2, 1 << 24)),
        "row stride of 2^31": s.call_rgb(C, RGB, 1 << 31, 1 << 40, d, w, wsb, n=1),
        "destination frame of 2^31 bytes": s.call_rgb(C, RGB, (1 << 31) // (dh - 1), 1 << 40, d, w, wsb, n=1),
        "workspace one byte short": s.call_rgb(C, RGB, rs, fs, d, w, wsb - 1),
        "workspace of two frames": s.call_rgb(C, RGB, rs, fs, d, w, libiqo_amd.yuv_rgb_workspace_bytes(dw, dh, N - 1)),
    }
    if kind == "i420":
        cases["null V"] = s.call_rgb(C, RGB, rs, fs, d, w, wsb, src_args=src(7, None))
    assert {k: v for k, v in cases.items() if v != EINVAL} == {}
    assert _untouched(dst)
    # order entries from `channels` on are ignored; one frame: the frame stride is unused
    o = (ctypes.c_int * 4)(2, 1, 0, 99)
    a = list(good)
    a[1] = 1
    L = libiqo_amd.lib()
    tail = (s.standard, 3, o, rs, 0, d, w, wsb, None)
    rc = L.iqo_hip_resize_nv12_rgb_device(*a, *tail) if kind == "nv12" else L.iqo_hip_resize_yuv420_rgb_device(*a, *tail, None)
    assert rc == 0
    torch.cuda.synchronize()
    _same(dst[:fs].cpu().numpy().reshape(dh, dw, 3), yr.reorder(s.rgb[0], (2, 1, 0)), s.what + ("after the errors",))
    assert (dst[fs:] == SENT).all()


@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_norm_abi_errors(kind, row):
    s = Setup(kind, row)
    dw, dh, P = s.dw, s.dh, 3
    dst = torch.full((N * P * dh * dw * 4 + 64,), SENT, dtype=torch.uint8, device=DEV)
    ws, wsb = s.workspace()
    rs, ps, fs, d, w = dw * 4, dh * dw * 4, P * dh * dw * 4, dst.data_ptr(), ws.data_ptr()
    good = lambda: _norm_struct("float32", RGB, SCALE, BIAS)  # noqa: E731

    def variant(**kw):
        n = good()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(n, k)[v[0]] = v[1]
            else:
                setattr(n, k, v)
        return n

    def call(norm, rs=rs, ps=ps, fs=fs, d=d, w=w, wsb=wsb, **kw):
        return s.call_norm(norm, rs, ps, fs, d, w, wsb, **kw)

    a = list(s.r._src_args(s.src))
    cases = {
        "null plan": call(good(), src_args=[None] + a[1:]),
        "null Y": call(good(), src_args=a[:5] + [None] + a[6:]),
        "null destination": call(good(), d=None),
        "null workspace": call(good(), w=None),
        "null norm": call(None),
        "standard 4": call(good(), standard=4),
        "standard -1": call(good(), standard=-1),
        "dtype 0": call(variant(dtype=0)),
        "dtype 4": call(variant(dtype=4)),
        "planes 0": call(variant(planes=0)),
        "planes 5": call(variant(planes=5)),
        "order 3 (alpha is no float source)": call(variant(order=(1, 3))),
        "order < 0": call(variant(order=(2, -1))),
        "scale inf": call(variant(scale=(0, float("inf")))),
        "scale nan": call(variant(scale=(2, float("nan")))),
        "bias -inf": call(variant(bias=(1, float("-inf")))),
        "bias nan": call(variant(bias=(0, float("nan")))),
        "destination off by 2 bytes": call(good(), d=d + 2),
        "row stride no multiple of 4": call(good(), rs=rs + 2, ps=dh * (rs + 2) + 2, fs=4 * (dh * (rs + 2) + 2)),
        "plane stride no multiple of 4": call(good(), ps=ps + 2, fs=4 * (ps + 2)),
        "frame stride no multiple of 4": call(good(), fs=fs + 2),
        "row stride < dstW * elem": call(good(), rs=rs - 4),
        "plane stride < dstH * row stride": call(good(), ps=ps - 4),
        "frame stride < planes * plane stride": call(good(), fs=fs - 4),
        "chroma stride < its row": call(good(), src_args=a[:3] + [a[3] - 1] + a[4:]),
        "float frame of 2^31 bytes": call(good(), n=1, ps=1 << 30, fs=3 << 30),
        "plane stride of 2^31 bytes": call(variant(planes=1), n=1, ps=1 << 31, fs=1 << 31),
        "workspace one byte short": call(good(), wsb=wsb - 1),
    }
    assert {k: v for k, v in cases.items() if v != EINVAL} == {}
    assert _untouched(dst)
    # the half types: element size 2
    n16 = _norm_struct("float16", RGB, SCALE, BIAS)
    assert call(n16, rs=dw * 2, ps=dh * dw * 2, fs=P * dh * dw * 2, d=d + 1) == EINVAL
    assert call(n16, rs=dw * 2 + 1, ps=dh * (dw * 2 + 1) + 1, fs=4 * dh * (dw * 2 + 2)) == EINVAL
    assert call(n16, rs=dw * 2 - 2, ps=dh * dw * 2, fs=P * dh * dw * 2) == EINVAL
    assert _untouched(dst)
    assert call(good(), n=1, fs=0) == 0  # one frame: the frame stride is unused
    torch.cuda.synchronize()
    assert not _untouched(dst)


def test_python_errors():
    s = Setup("nv12", LAYOUT_NV12)
    dw, dh = s.dw, s.dh
    out = torch.full((N, dh, dw, 3), SENT, dtype=torch.uint8, device=DEV)
    fout = torch.empty((N, 3, dh, dw), dtype=torch.float32, device=DEV)
    fout.view(torch.uint8).fill_(SENT)
    E = libiqo_amd.IqoError
    for kw in (dict(order="gbr"), dict(standard="bt2020"), dict(standard=7), dict(order="rgba"),  # out has 3 channels
               dict(out=out[:2]), dict(out=out[:, :, ::2]), dict(out=out.as_strided((N, dh, dw, 3), (dh * dw * 3, dw * 3 - 1, 3, 1)))):
        with pytest.raises(E):
            s.r.resize_rgb(s.src, **{"out": out, **kw})
    with pytest.raises(E):
        s.r.resize_rgb(s.src[:, :-1], out=out)
    with pytest.raises(E):
        s.r.resize_rgb(s.src.to(torch.int8), out=out)
    for kw in (dict(order=(0, 1, 3)), dict(order=(0, 1, -1)), dict(scale=(float("inf"),) + tuple(SCALE[1:])),
               dict(bias=(0.0, float("nan"), 0.0)), dict(scale=SCALE[:2]), dict(order=(0, 1)),
               dict(scale=SCALE * 2, bias=BIAS * 2, order=(0, 1, 2, 0, 1, 2)), dict(dtype=torch.float64),
               dict(dtype=torch.float16), dict(standard="bt470"), dict(out=fout[:, :2]),
               dict(out=fout.as_strided((N, 3, dh, dw), (3 * dh * dw, dh * dw, dw - 1, 1)))):
        args = {"scale": SCALE, "bias": BIAS, "out": fout, **kw}
        with pytest.raises(E):
            s.r.resize_normalized(s.src, args.pop("scale"), args.pop("bias"), **args)
    torch.cuda.synchronize()
    assert (out == SENT).all() and (fout.view(torch.uint8) == SENT).all()
    s.r.resize_rgb(s.src, standard=s.standard, out=out)
    _same(out.cpu().numpy(), s.rgb, "after the errors")


# ---- 7. a non-default stream and a strided out=

@pytest.mark.parametrize("kind,row", LAYOUT_ROWS, ids=["nv12", "i420"])
def test_stream_and_strided_out(kind, row):
    s = Setup(kind, row)
    dw, dh = s.dw, s.dh
    for pl in (0, 1):  # as before a graph capture: no upload inside the calls
        libiqo_amd.lib().iqo_hip_plan_prepare((libiqo_amd.lib().iqo_hip_nv12_plane if kind == "nv12"
                                               else libiqo_amd.lib().iqo_hip_yuv_plane)(s.r._plan, pl))
    big = torch.full((N + 2, dh + 3, dw + 5, 4), SENT, dtype=torch.uint8, device=DEV)
    view = big[1:1 + N, 2:2 + dh, 3:3 + dw]
    fbig = torch.empty((N + 1, 5, dh + 3, dw + 5), dtype=torch.float16, device=DEV)
    fbig.view(torch.uint8).fill_(SENT)
    fview = fbig[1:, 1:4, 2:2 + dh, 3:3 + dw]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    assert stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
    with torch.cuda.stream(stream):
        out = s.r.resize_rgb(s.src, standard=s.standard, order="bgra", out=view, stream=stream)
        fo = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=torch.float16, order=(2, 1, 0),
                                   out=fview, stream=stream)
    assert out is view and fo is fview
    stream.synchronize()
    _same(view.cpu().numpy(), yr.reorder(s.rgb, yr.ORDERS["bgra"]), s.what + ("bgra view",))
    mask = torch.ones(big.shape, dtype=torch.bool, device=DEV)
    mask[1:1 + N, 2:2 + dh, 3:3 + dw] = False
    assert (big[mask] == SENT).all(), "wrote outside the strided byte view"
    _same(_bits(fview), s.bits("float16", (2, 1, 0)), s.what + ("float16 view",))
    fmask = torch.ones(fbig.shape, dtype=torch.bool, device=DEV)
    fmask[1:, 1:4, 2:2 + dh, 3:3 + dw] = False
    want = int(np.array([SENT] * 2, np.uint8).view(np.int16)[0])
    assert (fbig.view(torch.int16)[fmask] == want).all(), "wrote outside the strided float view"


# ---- 8. the plane resizes are undisturbed: resize_frames before and after the new calls

@pytest.mark.parametrize("kind,row", [("nv12", LAYOUT_NV12), ("i420", TIE_I420)], ids=["nv12", "i420"])
def test_resize_frames_before_and_after(kind, row):
    s = Setup(kind, row)

    def planes():
        out = s.r.resize_frames(s.src)
        return (out[0] if kind == "i420" else out).cpu().numpy()

    before = planes()
    y, u, v = yr.expected_planes(s.case)
    chroma = np.stack([u, v], axis=3) if kind == "nv12" else np.stack([u, v], axis=1)
    _same(before, np.concatenate([y.reshape(N, -1), chroma.reshape(N, -1)], axis=1), s.what + ("planes",))
    _same(s.r.resize_rgb(s.src, standard=s.standard).cpu().numpy(), s.rgb, s.what + ("rgb",))
    s.check_fused()
    _same(_bits(s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=torch.bfloat16)), s.bits("bfloat16"),
          s.what + ("bfloat16",))
    _same(planes(), before, s.what + ("planes after",))
    if kind == "i420":
        assert s.r.resize_frames(s.src)[1] == (s.label != "none")
