"""NV12 / I420 to RGB with chroma filtered to the full output grid on the GPU (Nv12Resizer / Yuv420Resizer
with chroma="full" over iqo_hip_*_plan_set_chroma and the 4:4:4 form of yuv_rgb_kernel): the result is, bit
for bit, tests/yuv444_cases.py -- the per-plane oracle of Y and of U, V resized srcW/2 x srcH/2 -> dstW x dstH
at pxScale 1, then the integer matrix per pixel -- and norm_cases.expected_bits of those bytes for the
float forms.  Both UV kernels of NV12, every planar family of the I420 chroma plan, padded and misaligned
destinations with the workspace at exactly its queried size between guards, switching the mode back and
forth, the error returns, a side stream with a strided out=, byte orders and plane picks.  Bit patterns
are compared, never allclose.  Small shapes, 5 frames: well under a second each."""
import ctypes

import numpy as np
import pytest

import norm_cases as nc
import yuv444_cases as y4
import yuvrgb_cases as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENT = 0xA5
N = yr.N_FRAMES
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SCALE, BIAS = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
RGB = (0, 1, 2)

# the single rows of the layout, switch, error, stream and order tests
LAYOUT_NV12 = y4.NV12_CASES[0]                                                         # Lanczos-3 64x32 -> 33x17
LAYOUT_I420 = next(r for r in y4.I420_CASES if r[0][:6] == ("area", 0, 96, 48, 64, 32))
SWITCH_I420 = next(r for r in y4.I420_CASES if r[0][:6] == ("lanczos", 3, 64, 32, 32, 16))  # fused lz_sym10 planes
LAYOUT_ROWS = [LAYOUT_NV12, LAYOUT_I420]
KIND_IDS = ["nv12", "i420"]


class Setup:
    """A resizer, its source frames on the device and the expected RGB bytes [5, dh, dw, 3] of chroma="full"
    (the plans are built and the oracle run before anything is launched)."""

    def __init__(self, row, chroma="full"):
        self.case, self.standard, self.family = row
        m, d, sw, sh, dw, dh, self.kind = self.case
        self.dw, self.dh = dw, dh
        cls = libiqo_amd.Nv12Resizer if self.kind == "nv12" else libiqo_amd.Yuv420Resizer
        self.r = cls(m, d, sw, sh, dw, dh, chroma=chroma)
        self.rgb = y4.expected_rgb(self.case, self.standard)
        self.src = torch.from_numpy(y4.frames(self.case)).to(DEV)
        self.what = (y4.cid(row),)

    def bits(self, dtype, order=RGB, scale=SCALE, bias=BIAS):
        return nc.expected_bits(self.rgb, order, scale, bias, dtype)

    def mode(self):
        L = libiqo_amd.lib()
        return (L.iqo_hip_nv12_plan_chroma if self.kind == "nv12" else L.iqo_hip_yuv_plan_chroma)(self.r._plan)

    def set_mode(self, mode):
        L = libiqo_amd.lib()
        return (L.iqo_hip_nv12_plan_set_chroma if self.kind == "nv12" else L.iqo_hip_yuv_plan_set_chroma)(self.r._plan, mode)

    def plane(self, i):
        L = libiqo_amd.lib()
        return (L.iqo_hip_nv12_plane if self.kind == "nv12" else L.iqo_hip_yuv_plane)(self.r._plan, i)

    # the C ABI with explicit strides and pointers
    def call_rgb(self, C, order, row_st, frame_st, dst, ws, ws_bytes):
        o = (ctypes.c_int * 4)(*(tuple(order) + (0,) * (4 - len(order))))
        L = libiqo_amd.lib()
        a = self.r._src_args(self.src)
        if self.kind == "nv12":
            return L.iqo_hip_resize_nv12_rgb_device(*a, self.standard, C, o, row_st, frame_st, dst, ws, ws_bytes, None)
        return L.iqo_hip_resize_yuv420_rgb_device(*a, self.standard, C, o, row_st, frame_st, dst, ws, ws_bytes, None, None)

    def call_norm(self, norm, row_st, plane_st, frame_st, dst, ws, ws_bytes):
        L = libiqo_amd.lib()
        a = self.r._src_args(self.src)
        if self.kind == "nv12":
            return L.iqo_hip_resize_nv12_norm_device(*a, self.standard, ctypes.byref(norm), row_st, plane_st, frame_st,
                                                     dst, ws, ws_bytes, None)
        return L.iqo_hip_resize_yuv420_norm_device(*a, self.standard, ctypes.byref(norm), row_st, plane_st, frame_st, dst,
                                                   ws, ws_bytes, None, None)


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


# ---- 1. NV12: every row through both UV kernels of the full-grid plan

@pytest.mark.parametrize("row", y4.NV12_CASES, ids=y4.cid)
def test_nv12_every_row_both_uv_kernels(row):
    s = Setup(row)
    m, d, sw, sh, dw, dh, _ = s.case
    assert s.r.chroma == "full" and s.mode() == libiqo_amd.CHROMA_FULL
    assert libiqo_amd.host_chroma_full_kernel(m, d, sw, sh, dw, dh, layout="nv12") == s.family
    half = "float16" if y4.NV12_CASES.index(row) % 2 == 0 else "bfloat16"
    before = s.r.describe()
    for force, name in ((0, s.family), (1, "packed_general")):
        s.r.set_option("force_general", force, plane=2)
        assert s.r.chroma_kernel() == name and s.r.describe() == before and len(before) == 2
        out = s.r.resize_rgb(s.src, standard=s.standard)
        assert out.dtype == torch.uint8 and tuple(out.shape) == (N, dh, dw, 3)
        _same(out.cpu().numpy(), s.rgb, s.what + (name, "rgb"))
        for dtype in ("float32", half):
            out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=TORCH_DTYPE[dtype])
            assert out.dtype == TORCH_DTYPE[dtype] and tuple(out.shape) == (N, 3, dh, dw)
            _same(_bits(out), s.bits(dtype), s.what + (name, dtype))


# ---- 2. I420: every planar family of the chroma plan, bytes and fp32

@pytest.mark.parametrize("row", y4.I420_CASES, ids=y4.cid)
def test_i420_every_row(row):
    s = Setup(row)
    m, d, sw, sh, dw, dh, _ = s.case
    assert libiqo_amd.host_chroma_full_kernel(m, d, sw, sh, dw, dh, layout="i420") == s.family == s.r.chroma_kernel()
    s.r.last_fused = True
    out = s.r.resize_rgb(s.src, standard=s.standard)
    assert s.r.last_fused is False
    assert out.dtype == torch.uint8 and tuple(out.shape) == (N, dh, dw, 3)
    _same(out.cpu().numpy(), s.rgb, s.what + ("rgb",))
    s.r.last_fused = True
    out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=yr.NAMES[s.standard])
    assert s.r.last_fused is False
    assert out.dtype == torch.float32 and tuple(out.shape) == (N, 3, dh, dw)
    _same(_bits(out), s.bits("float32"), s.what + ("float32",))


# ---- 3. layouts: destination one element past a 64-byte boundary with padded rows, planes and frames; the
# workspace at exactly its queried size, one byte past a 64-byte boundary, between guards

G = 64


def _buffer(nbytes, e):
    buf = torch.full((64 + G + e + nbytes + G,), SENT, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 64 + G + e  # one element past a 64-byte boundary
    assert (buf.data_ptr() + base - e) % 64 == 0
    return buf, base


def _workspace(s):
    nbytes = libiqo_amd.yuv_rgb_workspace_bytes(s.dw, s.dh, N, "full")
    assert nbytes > libiqo_amd.yuv_rgb_workspace_bytes(s.dw, s.dh, N)
    buf, base = _buffer(nbytes, 1)
    return buf, base, nbytes


def _check_workspace_guards(buf, base, nbytes, what):
    full = buf.cpu().numpy()
    assert (full[:base] == SENT).all() and (full[base + nbytes:] == SENT).all(), (what, "wrote outside the workspace")


def _check_outside(full, payload, base, e, nbytes, what):
    stray = np.flatnonzero(~payload & (full != SENT))
    assert stray.size == 0, (what, "wrote outside the payload at byte offsets (from the base)", (stray[:8] - base).tolist())
    assert payload[:base].sum() == 0 and (full[base - e - G:base] == SENT).all()
    assert (full[base + nbytes:base + nbytes + G] == SENT).all()


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_rgb_padded_misaligned_layout(row, C):
    s = Setup(row)
    dw, dh = s.dw, s.dh
    order = yr.ORDERS["rgb" if C == 3 else "bgra"]
    row_st = dw * C + 1
    frame_st = dh * row_st + 5
    buf, base = _buffer(N * frame_st, 1)
    wbuf, wbase, wsb = _workspace(s)
    assert s.call_rgb(C, order, row_st, frame_st, buf.data_ptr() + base, wbuf.data_ptr() + wbase, wsb) == 0
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
    _check_workspace_guards(wbuf, wbase, wsb, s.what + (C,))


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_norm_padded_misaligned_layout(row, dtype):
    s = Setup(row)
    dw, dh, e, P = s.dw, s.dh, nc.ELEM[dtype], 3
    row_st = (dw + 1) * e
    plane_st = dh * row_st + 3 * e
    frame_st = P * plane_st + 5 * e
    buf, base = _buffer(N * frame_st, e)
    wbuf, wbase, wsb = _workspace(s)
    rc = s.call_norm(_norm_struct(dtype, RGB, SCALE, BIAS), row_st, plane_st, frame_st, buf.data_ptr() + base,
                     wbuf.data_ptr() + wbase, wsb)
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
    _check_workspace_guards(wbuf, wbase, wsb, s.what + (dtype,))


# ---- 4. the mode is switched on one resizer; the plane resizes never see it

@pytest.mark.parametrize("row", [LAYOUT_NV12, SWITCH_I420], ids=KIND_IDS)
def test_mode_switching(row):
    s = Setup(row)
    m, d, sw, sh, dw, dh, kind = s.case
    replicated = yr.expected_rgb(s.case, s.standard)
    fused = kind == "i420" and libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) != "none"
    assert kind == "nv12" or fused, "the I420 row's plane resize is a fused launch"
    y, u, v = yr.expected_planes(s.case)
    chroma = np.stack([u, v], axis=3) if kind == "nv12" else np.stack([u, v], axis=1)
    planes = np.concatenate([y.reshape(N, -1), chroma.reshape(N, -1)], axis=1)

    def check_planes(when):
        out = s.r.resize_frames(s.src)
        if kind == "i420":
            assert out[1] == fused, when
            out = out[0]
        _same(out.cpu().numpy(), planes, s.what + ("planes", when))

    def check_rgb(exp, when):
        _same(s.r.resize_rgb(s.src, standard=s.standard).cpu().numpy(), exp, s.what + ("rgb", when))
        got = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=torch.float16)
        _same(_bits(got), nc.expected_bits(exp, RGB, SCALE, BIAS, "float16"), s.what + ("float16", when))
        if kind == "i420":
            assert s.r.last_fused == (fused and s.r.chroma == "replicate"), when

    extra = s.plane(2)
    assert extra
    check_planes("before")
    check_rgb(s.rgb, "full")
    s.r.set_chroma("replicate")
    assert s.r.chroma == "replicate" and s.mode() == libiqo_amd.CHROMA_REPLICATE
    assert s.plane(2) == extra  # the extra plan is kept
    check_rgb(replicated, "replicate")
    check_planes("between")
    s.r.set_chroma("full")
    assert s.r.chroma == "full" and s.mode() == libiqo_amd.CHROMA_FULL and s.plane(2) == extra
    check_rgb(s.rgb, "full again")
    check_planes("after")


# ---- 5. errors through the C ABI: rejected on the host before any launch, the destination untouched

def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst == SENT).all())


@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_workspace_errors(row):
    s = Setup(row)
    dw, dh, C = s.dw, s.dh, 3
    dst = torch.full((N * dh * dw * 4 + 64,), SENT, dtype=torch.uint8, device=DEV)
    need = libiqo_amd.yuv_rgb_workspace_bytes(dw, dh, N, "full")
    small = libiqo_amd.yuv_rgb_workspace_bytes(dw, dh, N)
    ws = torch.empty((need,), dtype=torch.uint8, device=DEV)
    rs, fs, d, w = dw * C, dh * dw * C, dst.data_ptr(), ws.data_ptr()
    n32 = _norm_struct("float32", RGB, SCALE, BIAS)
    cases = {
        "rgb, a replicate-sized workspace": s.call_rgb(C, RGB, rs, fs, d, w, small),
        "rgb, one byte short": s.call_rgb(C, RGB, rs, fs, d, w, need - 1),
        "norm, a replicate-sized workspace": s.call_norm(n32, dw * 4, dh * dw * 4, 3 * dh * dw * 4, d, w, small),
        "norm, one byte short": s.call_norm(n32, dw * 4, dh * dw * 4, 3 * dh * dw * 4, d, w, need - 1),
        "a mode that does not exist": s.set_mode(2),
        "a negative mode": s.set_mode(-1),
    }
    assert {k: v for k, v in cases.items() if v != y4.EINVAL} == {}
    assert _untouched(dst) and s.mode() == libiqo_amd.CHROMA_FULL
    # in replicate mode the smaller workspace is enough again, and the larger one is accepted in both
    assert s.set_mode(libiqo_amd.CHROMA_REPLICATE) == 0
    assert s.call_rgb(C, RGB, rs, fs, d, w, small - 1) == y4.EINVAL and _untouched(dst)
    assert s.call_rgb(C, RGB, rs, fs, d, w, small) == 0
    torch.cuda.synchronize()
    _same(dst[:N * fs].cpu().numpy().reshape(N, dh, dw, 3), yr.expected_rgb(s.case, s.standard), s.what + ("replicate",))
    assert s.set_mode(libiqo_amd.CHROMA_FULL) == 0
    assert s.call_rgb(C, RGB, rs, fs, d, w, need) == 0
    torch.cuda.synchronize()
    _same(dst[:N * fs].cpu().numpy().reshape(N, dh, dw, 3), s.rgb, s.what + ("full",))
    assert (dst[N * fs:] == SENT).all()


@pytest.mark.parametrize("kind", KIND_IDS)
@pytest.mark.parametrize("rejected", y4.REJECTED, ids=lambda r: "%s%d-%dx%d-%dx%d" % r[0])
def test_rejected_set_chroma_leaves_the_resizer_as_it_was(rejected, kind):
    shape, status = rejected
    row = (shape + (kind,), yr.BT709_LIMITED, None)
    case, standard, _ = row
    cls = libiqo_amd.Nv12Resizer if kind == "nv12" else libiqo_amd.Yuv420Resizer
    with pytest.raises(libiqo_amd.IqoError):
        cls(*shape, chroma="full")
    r = cls(*shape)
    L = libiqo_amd.lib()
    setter, getter, plane = ((L.iqo_hip_nv12_plan_set_chroma, L.iqo_hip_nv12_plan_chroma, L.iqo_hip_nv12_plane) if kind == "nv12"
                             else (L.iqo_hip_yuv_plan_set_chroma, L.iqo_hip_yuv_plan_chroma, L.iqo_hip_yuv_plane))
    exp = yr.expected_rgb(case, standard)
    src = torch.from_numpy(y4.frames(case)).to(DEV)
    _same(r.resize_rgb(src, standard=standard).cpu().numpy(), exp, (shape, kind, "before"))
    assert setter(r._plan, libiqo_amd.CHROMA_FULL) == status
    with pytest.raises(libiqo_amd.IqoError):
        r.set_chroma("full")
    assert getter(r._plan) == libiqo_amd.CHROMA_REPLICATE and r.chroma == "replicate"
    assert plane(r._plan, 2) is None and r.chroma_kernel() is None
    with pytest.raises(libiqo_amd.IqoError):
        r.set_option("force_general", 1, plane=2)
    _same(r.resize_rgb(src, standard=standard).cpu().numpy(), exp, (shape, kind, "after"))
    got = r.resize_normalized(src, SCALE, BIAS, standard=standard)
    _same(_bits(got), nc.expected_bits(exp, RGB, SCALE, BIAS, "float32"), (shape, kind, "float32 after"))


# ---- 6. a non-default stream and a strided out=, after iqo_hip_plan_prepare on the three sub-plans

@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_stream_and_strided_out(row):
    s = Setup(row)
    dw, dh = s.dw, s.dh
    for pl in (0, 1, 2):  # as before a graph capture: no upload inside the calls
        assert libiqo_amd.lib().iqo_hip_plan_prepare(s.plane(pl)) == 0
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


# ---- 7. byte orders and a plane pick

@pytest.mark.parametrize("order", ["bgr", "bgra"])
@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_rgb_orders(row, order):
    s = Setup(row)
    out = s.r.resize_rgb(s.src, standard=s.standard, order=order)
    C = len(yr.ORDERS[order])
    assert tuple(out.shape) == (N, s.dh, s.dw, C)
    got = out.cpu().numpy()
    _same(got, yr.reorder(s.rgb, yr.ORDERS[order]), s.what + (order,))
    if C == 4:
        assert (got[..., 3] == 255).all()


@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=KIND_IDS)
def test_norm_plane_pick(row):
    s = Setup(row)
    order = (2, 1, 0)
    out = s.r.resize_normalized(s.src, SCALE, BIAS, standard=s.standard, dtype=torch.bfloat16, order=order)
    _same(_bits(out), s.bits("bfloat16", order), s.what + (order,))
