"""GPU parity of planar U8 frames resized straight to normalised planar float tensors
(iqo_hip_resize_planes_norm_device / resize_planes_normalized / resize_luma_normalized): output plane p is,
bit for bit,

    cvt(fl32(fl32(float(u8[f, order[p]]) * scale[p]) + bias[p]))

of the per-plane oracle's bytes (planes_norm_cases) -- over one shape per first-pass kernel family, each the
smallest at which planes_norm_kernel meets another store path, the three dtypes, plane orders, strided
sources and destinations, the error paths, the Python surface and the luma-only form of the two YUV
resizers.  Bit patterns are compared, never allclose.  2 frames of 3 planes: well under a second each."""
import ctypes
import os

import numpy as np
import pytest

import norm_cases as nc
import planes_norm_cases as pn
import yuv_cases as yc
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
EINVAL, EUNSUP = -1, -5
SCALE, BIAS = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
ENTRY = "iqo_hip_resize_planes_norm_device"


def _make(shape, channels=1):
    m, d, sw, sh, dw, dh = shape
    return libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, 1, channels=channels)


def _bits(t):
    """Bit patterns of a float tensor as a numpy integer array."""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _check(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first [frame, plane, y, x] %s" % (what, len(bad), bad[:4].tolist())


def _norm_struct(dtype, order, scale, bias):
    n = libiqo_amd.Norm(nc.CODE[dtype], len(order))
    for i, (c, s, b) in enumerate(zip(order, scale, bias)):
        n.order[i], n.scale[i], n.bias[i] = c, s, b
    return n


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared inputs are read-only)


# ---- 1. every first-pass family x every dtype: P = 3, identity order, contiguous source (one launch)

@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("row", pn.SHAPES, ids=lambda r: "%s-%s" % (pn.sid(r[0]), r[1]))
def test_every_family(row, dtype):
    shape, family = row
    r = _make(shape)
    assert r.describe()["kernel"] == family
    exp = pn.expected_bits(pn.expected_u8(shape), (0, 1, 2), SCALE, BIAS, dtype)
    src = _dev(pn.frames_for(shape))
    out = r.resize_planes_normalized(src, SCALE, BIAS, dtype=TORCH_DTYPE[dtype])
    assert out.dtype == TORCH_DTYPE[dtype] and tuple(out.shape) == (2, 3, shape[5], shape[4])
    _check(_bits(out), exp, (shape, family, dtype))


# ---- 2. orders: repeats, a permutation with a dropped plane, one plane of two

ORDER_CASES = [
    # (source planes, order, scale, bias)
    (1, (0, 0, 0), nc.NORM_SCALE[:3], (nc.NORM_BIAS[2], nc.NORM_BIAS[0], nc.NORM_BIAS[3])),  # grey -> three maps
    (4, (2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]),                                     # BGRA planes -> RGB
    (2, (1,), nc.NORM_SCALE[3:4], nc.NORM_BIAS[3:4]),
]


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: "p%d-order%s" % (c[0], "".join(map(str, c[1]))))
def test_orders(case, dtype):
    P, order, scale, bias = case
    shape = pn.RYG
    assert len({(s, b) for s, b in zip(scale, bias)}) == len(order)
    exp = pn.expected_bits(pn.expected_u8(shape, P), order, scale, bias, dtype)
    frames = pn.frames_for(shape, P)
    r = _make(shape)
    out = r.resize_planes_normalized(_dev(frames), scale, bias, dtype=TORCH_DTYPE[dtype], order=order)
    assert tuple(out.shape) == (2, len(order), shape[5], shape[4])
    _check(_bits(out), exp, (case, dtype))
    dropped = sorted(set(range(P)) - set(order))
    if dropped:
        # a plane `order` does not name has no effect, whatever it holds
        other = frames.copy()
        for c in dropped:
            other[:, c] = 255 - other[:, c]
        again = r.resize_planes_normalized(_dev(other), scale, bias, dtype=TORCH_DTYPE[dtype], order=order)
        _check(_bits(again), exp, (case, dtype, "dropped plane changed"))


# ---- 3. source layouts: all equal to the contiguous result

def _spy(monkeypatch):
    """Records the arguments of the C entry while passing them on."""
    L = libiqo_amd.lib()
    real = getattr(L, ENTRY)
    calls = []

    def spy(*a):
        calls.append(a)
        return real(*a)

    monkeypatch.setattr(L, ENTRY, spy)
    return calls


@pytest.mark.parametrize("shape", [pn.STREAM, pn.RYG], ids=pn.sid)
def test_source_layouts(shape, monkeypatch):
    m, d, sw, sh, dw, dh = shape
    F, P = 2, 3
    frames = pn.frames_for(shape)
    exp = pn.expected_bits(pn.expected_u8(shape), (0, 1, 2), SCALE, BIAS, "float16")
    r = _make(shape)
    calls = _spy(monkeypatch)

    def run(view, what):
        assert view.shape == (F, P, sh, sw) and (view.cpu().numpy() == frames).all(), what
        del calls[:]
        out = r.resize_planes_normalized(view, SCALE, BIAS, dtype=torch.float16)
        # read where it lies: the view's own address and strides reach the C entry
        assert len(calls) == 1 and calls[0][6] == view.data_ptr(), what
        assert calls[0][3:6] == (view.stride(2), view.stride(1), view.stride(0)), what
        _check(_bits(out), exp, (shape, what))

    run(_dev(frames), "contiguous")
    # padding between frames: srcFrameSt != P * srcPlaneSt, one launch per plane
    pad = torch.full((F, P * sh * sw + 48), SENTINEL, dtype=torch.uint8, device=DEV)
    pad[:, :P * sh * sw] = _dev(frames).reshape(F, -1)
    run(pad[:, :P * sh * sw].view(F, P, sh, sw), "padded frames")
    # a padded row stride
    wide = torch.full((F, P, sh, sw + 16), SENTINEL, dtype=torch.uint8, device=DEV)
    wide[..., :sw] = _dev(frames)
    run(wide[..., :sw], "padded rows")
    # a base 1 byte off every alignment: the plan's fallback family, whatever it is
    flat = torch.full((F * P * sh * sw + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    off = (-flat.data_ptr()) % 16 + 1
    flat[off:off + F * P * sh * sw] = _dev(frames).reshape(-1)
    odd = flat[off:off + F * P * sh * sw].view(F, P, sh, sw)
    assert odd.data_ptr() % 16 == 1
    run(odd, "base 1 byte off")
    # a crop of a larger tensor, against the copied crop
    big = torch.full((F, P, sh + 5, sw + 9), SENTINEL, dtype=torch.uint8, device=DEV)
    big[:, :, 2:2 + sh, 3:3 + sw] = _dev(frames)
    crop = big[:, :, 2:2 + sh, 3:3 + sw]
    copied = crop.contiguous()
    assert not crop.is_contiguous() and copied.data_ptr() != crop.data_ptr()
    run(crop, "crop view")
    run(copied, "copied crop")
    # a channel slice: planes 1..3 of four
    four = torch.full((F, 4, sh, sw), SENTINEL, dtype=torch.uint8, device=DEV)
    four[:, 1:] = _dev(frames)
    run(four[:, 1:], "channel slice")
    # a column stride of 2 is the one layout that is copied
    two = torch.zeros((F, P, sh, 2 * sw), dtype=torch.uint8, device=DEV)
    two[..., ::2] = _dev(frames)
    del calls[:]
    out = r.resize_planes_normalized(two[..., ::2], SCALE, BIAS, dtype=torch.float16)
    assert len(calls) == 1 and calls[0][3:6] == (sw, sh * sw, P * sh * sw)
    _check(_bits(out), exp, (shape, "column stride 2"))


# ---- 4. destination layouts: misaligned bases, padded rows, planes and frames, guards

def _call(r, n, P, src, norm, row_st, plane_st, frame_st, dst_ptr, ws, ws_bytes=None, stream=None, src_st=None):
    sw, sh = r.srcW, r.srcH
    return getattr(libiqo_amd.lib(), ENTRY)(r._plan, n, P, sw if src_st is None else src_st, sh * sw, P * sh * sw,
                                            src.data_ptr(), ctypes.byref(norm), row_st, plane_st, frame_st, dst_ptr,
                                            ws.data_ptr(), ws.numel() if ws_bytes is None else ws_bytes, stream)


def _workspace(r, P, n):
    return torch.empty((libiqo_amd.planes_norm_workspace_bytes(r.dstW, r.dstH, P, n),), dtype=torch.uint8, device=DEV)


@pytest.mark.parametrize("base_off", ["element", "eight"])
@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("shape", [pn.RYG, pn.TILE], ids=pn.sid)
def test_padded_misaligned_destination(shape, dtype, base_off):
    m, d, sw, sh, dw, dh = shape
    n, P, e = 2, 3, nc.ELEM[dtype]
    row_st = (dw + 1) * e
    plane_st = dh * row_st + 3 * e
    frame_st = P * plane_st + 5 * e
    G = 64
    buf = torch.full((64 + G + 8 + n * frame_st + G,), SENTINEL, dtype=torch.uint8, device=DEV)
    # one element past a 64-byte boundary (single elements), or 8 bytes past one: 8- but not 16-byte aligned,
    # where whole groups go out as 8-byte stores
    shift = e if base_off == "element" else 8
    base = (-buf.data_ptr()) % 64 + G + shift
    assert (buf.data_ptr() + base - shift) % 64 == 0
    r = _make(shape)
    src = _dev(pn.frames_for(shape))
    ws = _workspace(r, P, n)
    rc = _call(r, n, P, src, _norm_struct(dtype, (0, 1, 2), SCALE, BIAS), row_st, plane_st, frame_st,
               buf.data_ptr() + base, ws)
    assert rc == 0
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    payload = np.zeros(full.shape, bool)
    got = np.empty((n, P, dh, dw), np.int32 if e == 4 else np.int16)
    for f in range(n):
        for p in range(P):
            for y in range(dh):
                o = base + f * frame_st + p * plane_st + y * row_st
                payload[o:o + dw * e] = True
                got[f, p, y] = full[o:o + dw * e].view(got.dtype)
    _check(got, pn.expected_bits(pn.expected_u8(shape), (0, 1, 2), SCALE, BIAS, dtype), (shape, dtype, base_off))
    # row padding, plane gaps, frame gaps and both guards
    stray = np.flatnonzero(~payload & (full != SENTINEL))
    assert stray.size == 0, (shape, dtype, base_off, "wrote outside the payload at byte offsets (from the base)",
                             (stray[:8] - base).tolist())
    assert payload[:base].sum() == 0 and (full[base - shift - G:base] == SENTINEL).all()
    assert (full[base + n * frame_st:base + n * frame_st + G] == SENTINEL).all()


# ---- 5. errors: rejected on the host before any launch, the destination untouched

def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst == SENTINEL).all())


def test_abi_errors():
    shape = pn.RYG
    m, d, sw, sh, dw, dh = shape
    P, n = 3, 2
    r = _make(shape)
    src = _dev(pn.frames_for(shape))
    row, plane, frame = dw * 4, dh * dw * 4, P * dh * dw * 4
    dst = torch.full((n * frame + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = _workspace(r, P, n)
    need = libiqo_amd.planes_norm_workspace_bytes(dw, dh, P, n)
    good = lambda: _norm_struct("float32", (0, 1, 2), SCALE, BIAS)  # noqa: E731
    fn = getattr(libiqo_amd.lib(), ENTRY)

    def call(plan=r._plan, n=n, P=P, s=src.data_ptr(), norm=None, rs=row, ps=plane, fs=frame, d=dst.data_ptr(), sst=sw,
             w=ws.data_ptr(), wb=need):
        nm = ctypes.byref(norm) if norm is not None else None
        return fn(plan, n, P, sst, sh * sw, P * sh * sw, s, nm, rs, ps, fs, d, w, wb, None)

    def variant(**kw):
        nm = good()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(nm, k)[v[0]] = v[1]
            else:
                setattr(nm, k, v)
        return nm

    assert call(norm=good(), wb=need) == 0  # the arguments every case below varies are good ones
    torch.cuda.synchronize()
    dst.fill_(SENTINEL)

    packed = _make(shape, channels=3)
    assert call(plan=packed._plan, norm=good()) == EUNSUP
    assert _untouched(dst)

    cases = {
        "null plan": call(plan=None, norm=good()),
        "null source": call(s=None, norm=good()),
        "null destination": call(d=None, norm=good()),
        "null norm": call(norm=None),
        "null workspace": call(w=None, norm=good()),
        "srcPlanes 0": call(P=0, norm=good()),
        "srcPlanes 5": call(P=5, norm=good()),
        "dtype 0": call(norm=variant(dtype=0)),
        "dtype 4": call(norm=variant(dtype=4)),
        "planes 0": call(norm=variant(planes=0)),
        "planes 5": call(norm=variant(planes=5)),
        "order = srcPlanes": call(norm=variant(order=(1, P))),
        "order = srcPlanes of 1": call(P=1, norm=variant(planes=1, order=(0, 1))),
        "order < 0": call(norm=variant(order=(2, -1))),
        "scale inf": call(norm=variant(scale=(0, float("inf")))),
        "scale nan": call(norm=variant(scale=(2, float("nan")))),
        "bias -inf": call(norm=variant(bias=(1, float("-inf")))),
        "bias nan": call(norm=variant(bias=(0, float("nan")))),
        "destination off by 2 bytes": call(norm=good(), d=dst.data_ptr() + 2),
        "row stride no multiple of 4": call(norm=good(), rs=row + 2, ps=dh * (row + 2) + 2, fs=4 * (dh * (row + 2) + 2)),
        "plane stride no multiple of 4": call(norm=good(), ps=plane + 2, fs=4 * (plane + 2)),
        "frame stride no multiple of 4": call(norm=good(), fs=frame + 2),
        "row stride < dstW * elem": call(norm=good(), rs=row - 4),
        "plane stride < dstH * row stride": call(norm=good(), ps=plane - 4),
        "frame stride < planes * plane stride": call(norm=good(), fs=frame - 4),
        "float frame of 2^31 bytes": call(norm=good(), n=1, ps=1 << 30, fs=3 << 30),
        "plane stride of 2^31 bytes": call(norm=variant(planes=1), n=1, ps=1 << 31, fs=1 << 31),
        "source stride < srcW": call(norm=good(), sst=sw - 1),
        "source stride of 2^24": call(norm=good(), sst=1 << 24),
        "workspace one byte short": call(norm=good(), wb=need - 1),
        "workspace of another frame count": call(norm=good(), wb=libiqo_amd.planes_norm_workspace_bytes(dw, dh, P, n - 1)),
    }
    assert {k: v for k, v in cases.items() if v != EINVAL} == {}
    assert _untouched(dst)
    # the half types: element size 2
    n16 = _norm_struct("float16", (0, 1, 2), SCALE, BIAS)
    assert call(norm=n16, rs=dw * 2, ps=dh * dw * 2, fs=P * dh * dw * 2, d=dst.data_ptr() + 1) == EINVAL
    assert call(norm=n16, rs=dw * 2 + 1, ps=dh * (dw * 2 + 1) + 1, fs=4 * dh * (dw * 2 + 2)) == EINVAL
    assert call(norm=n16, rs=dw * 2 - 2, ps=dh * dw * 2, fs=P * dh * dw * 2) == EINVAL
    assert _untouched(dst)
    # no frames: OK after the checks, nothing written
    assert call(norm=good(), n=0) == 0 and call(norm=good(), n=0, wb=15) == 0
    assert call(norm=variant(dtype=0), n=0) == EINVAL
    assert _untouched(dst)
    # frames = 1: the frame stride is not compared with the planes (it is unused)
    assert call(norm=good(), n=1, fs=0) == 0
    torch.cuda.synchronize()
    assert not _untouched(dst)


def test_source_plane_of_2_31_bytes_is_einval():
    """The walk shape has rows enough for a plane to reach 2^31 bytes below the 2^24 row stride limit."""
    shape = pn.BY_FAMILY["walk"]
    m, d, sw, sh, dw, dh = shape
    r = _make(shape)
    sst = 10000000
    assert sst < 1 << 24 and (sh - 1) * sst + sw >= 1 << 31 > (sh - 1) * (sst // 2) + sw
    src = _dev(pn.frames_for(shape)[:1, :1])
    dst = torch.full((dh * dw * 4,), SENTINEL, dtype=torch.uint8, device=DEV)
    ws = _workspace(r, 1, 1)
    nm = _norm_struct("float32", (0,), SCALE[:1], BIAS[:1])
    # (nothing is launched, so the stride may describe memory that is not there)
    assert _call(r, 1, 1, src, nm, dw * 4, dh * dw * 4, dh * dw * 4, dst.data_ptr(), ws, src_st=sst) == EINVAL
    assert _untouched(dst)


# ---- 6. the Python surface

def test_python_surface():
    shape = pn.RYG
    m, d, sw, sh, dw, dh = shape
    frames = pn.frames_for(shape)
    u8 = pn.expected_u8(shape)
    src = _dev(frames)
    r = _make(shape)
    # a 3-D source gives a 3-D result
    single = r.resize_planes_normalized(src[1], SCALE, BIAS)
    assert single.dtype == torch.float32 and tuple(single.shape) == (3, dh, dw)
    _check(_bits(single)[None], pn.expected_bits(u8[1:], (0, 1, 2), SCALE, BIAS, "float32"), "3-D source")
    # scale 1, bias 0 in fp32 is resize_tensor's result as floats
    unit = r.resize_planes_normalized(src, (1.0,) * 3, (0.0,) * 3)
    assert torch.equal(unit, r.resize_tensor(src.view(6, sh, sw)).view(2, 3, dh, dw).float())


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_stream_and_strided_out(dtype):
    shape = pn.RYG
    m, d, sw, sh, dw, dh = shape
    order = (2, 1, 0)
    r = _make(shape)
    r.prepare()
    src = _dev(pn.frames_for(shape))
    big = torch.empty((3, 5, dh + 3, dw + 5), dtype=TORCH_DTYPE[dtype], device=DEV)
    big.view(torch.uint8).fill_(SENTINEL)
    view = big[1:3, 1:4, 2:2 + dh, 3:3 + dw]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    assert stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
    with torch.cuda.stream(stream):
        out = r.resize_planes_normalized(src, SCALE, BIAS, dtype=TORCH_DTYPE[dtype], order=order, out=view, stream=stream)
    assert out is view
    stream.synchronize()
    _check(_bits(view), pn.expected_bits(pn.expected_u8(shape), order, SCALE, BIAS, dtype), (shape, dtype))
    mask = torch.ones(big.shape, dtype=torch.bool, device=DEV)
    mask[1:3, 1:4, 2:2 + dh, 3:3 + dw] = False
    outside = big.view(torch.int32 if dtype == "float32" else torch.int16)[mask]
    want = int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0]) if dtype == "float32" else int(
        np.array([SENTINEL] * 2, np.uint8).view(np.int16)[0])
    assert (outside == want).all(), "wrote outside the strided view"


def test_python_errors():
    shape = pn.RYG
    m, d, sw, sh, dw, dh = shape
    r = _make(shape)
    src = _dev(pn.frames_for(shape))
    out = torch.empty((2, 3, dh, dw), dtype=torch.float32, device=DEV)
    out.view(torch.uint8).fill_(SENTINEL)
    packed = _make(shape, channels=3)
    with pytest.raises(libiqo_amd.IqoError, match="resize_normalized"):
        packed.resize_planes_normalized(src, SCALE, BIAS, out=out)
    bad = [
        dict(scale=SCALE, bias=BIAS, order=(0, 1, 3)),                       # order out of range
        dict(scale=SCALE, bias=BIAS, order=(0, 1, -1)),
        dict(scale=(float("inf"),) + tuple(SCALE[1:]), bias=BIAS),           # ABI: non-finite
        dict(scale=SCALE, bias=(0.0, float("nan"), 0.0)),
        dict(scale=SCALE[:2], bias=BIAS),                                    # lengths
        dict(scale=SCALE, bias=BIAS, order=(0, 1)),
        dict(scale=SCALE * 2, bias=BIAS * 2, order=(0, 1, 2, 0, 1, 2)),      # planes > 4
        dict(scale=(), bias=(), order=()),
        dict(scale=SCALE, bias=BIAS, dtype=torch.float64),
        dict(scale=SCALE, bias=BIAS, dtype=torch.float16),                   # out is float32
    ]
    for kw in bad:
        with pytest.raises(libiqo_amd.IqoError):
            r.resize_planes_normalized(src, out=out, **kw)
    wrong_sources = [
        src[:, :, :-1],                                                      # a wrong height
        src.view(6, sh, sw),                                                 # [F, H, W] with F no plane count
        torch.cat([src, src[:, :2]], dim=1),                                 # 5 planes
        src.to(torch.int8),                                                  # a wrong dtype
        src.cpu(),                                                           # not on the device
    ]
    for s in wrong_sources:
        with pytest.raises(libiqo_amd.IqoError):
            r.resize_planes_normalized(s, SCALE, BIAS, out=out)
    with pytest.raises(libiqo_amd.IqoError):  # overlapping rows
        r.resize_planes_normalized(src, SCALE, BIAS, out=out.as_strided((2, 3, dh, dw), (3 * dh * dw, dh * dw, dw - 1, 1)))
    with pytest.raises(libiqo_amd.IqoError):  # column stride 2
        r.resize_planes_normalized(src, SCALE, BIAS, out=torch.empty((2, 3, dh, 2 * dw), dtype=torch.float32,
                                                                     device=DEV)[..., ::2])
    with pytest.raises(libiqo_amd.IqoError):  # wrong plane count
        r.resize_planes_normalized(src, SCALE, BIAS, out=out[:, :2])
    torch.cuda.synchronize()
    assert (out.view(torch.uint8) == SENTINEL).all()
    r.resize_planes_normalized(src, SCALE, BIAS, out=out)
    _check(_bits(out), pn.expected_bits(pn.expected_u8(shape), (0, 1, 2), SCALE, BIAS, "float32"), "after the errors")


# ---- 7. luma only, from the two YUV resizers

LUMA_CASES = [next(c for c in yc.CASES if c[:6] == ("lanczos", 3, 64, 32, 32, 16)),   # Y by lanczos_stream, fused I420
              next(c for c in yc.CASES if c[:6] == ("lanczos", 3, 3840, 50, 1920, 25))]  # "none": plane by plane


@pytest.mark.parametrize("kind", ["nv12", "i420"])
@pytest.mark.parametrize("case", LUMA_CASES, ids=yc.cid)
def test_luma(case, kind):
    m, d, sw, sh, dw, dh, label = case
    assert label == ("lz_sym10" if sw == 64 else "none")
    assert libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh) == "lanczos_stream"
    if kind == "nv12":
        r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
        frames = yr.nv12_frames(case)
    else:
        r = libiqo_amd.Yuv420Resizer(m, d, sw, sh, dw, dh)
        frames = yr.i420_frames(case)
    y, u, v = yr.expected_planes(case)  # the per-plane oracle of those frames
    n = y.shape[0]
    src = _dev(frames)
    scale3, bias3 = SCALE, (nc.NORM_BIAS[2], nc.NORM_BIAS[0], nc.NORM_BIAS[3])
    results = {}
    for dtype in nc.DTYPES:
        for scale, bias in ((scale3, bias3), (scale3[1:2], bias3[1:2])):
            planes = len(scale)
            out = r.resize_luma_normalized(src, scale, bias, dtype=TORCH_DTYPE[dtype])
            assert out.dtype == TORCH_DTYPE[dtype] and tuple(out.shape) == (n, planes, dh, dw)
            results[dtype, planes] = _bits(out)
            _check(results[dtype, planes], pn.expected_bits(y[:, None], (0,) * planes, scale, bias, dtype),
                   (kind, yc.cid(case), dtype, planes))
    # the chroma mode has no effect
    r.set_chroma("full")
    out = r.resize_luma_normalized(src, scale3, bias3, dtype=torch.float16)
    _check(_bits(out), results["float16", 3], (kind, yc.cid(case), "chroma full"))
    r.set_chroma("replicate")
    # the shared luma sub-plan is left in order: resize_frames still gives the oracle's planes
    res = r.resize_frames(src)
    got = (res if kind == "nv12" else res[0]).cpu().numpy()
    chroma = np.stack([u, v], axis=3).reshape(n, -1) if kind == "nv12" else np.concatenate(
        [u.reshape(n, -1), v.reshape(n, -1)], axis=1)
    want = np.concatenate([y.reshape(n, -1), chroma], axis=1)
    assert got.shape == want.shape and (got == want).all(), (kind, yc.cid(case), "resize_frames afterwards")
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_luma_normalized(src[:, :-1], scale3, bias3)
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_luma_normalized(src, scale3, bias3[:2])


# ---- 8. a batch across several blocks of partial groups only

@pytest.mark.parametrize("dtype", ["float32", "bfloat16"])
def test_many_frames_of_partial_groups(dtype):
    shape = pn.TILE
    F, P = 40, 3
    r = _make(shape)
    assert r.describe()["kernel"] == "tile"
    # fp32: 40 x 40 rows x 2 groups, bf16: x 1 group -- 13 and 7 blocks of 256 threads
    src = _dev(pn.frames_for(shape, P, F))
    out = r.resize_planes_normalized(src, SCALE, BIAS, dtype=TORCH_DTYPE[dtype])
    _check(_bits(out), pn.expected_bits(pn.expected_u8(shape, P, F), (0, 1, 2), SCALE, BIAS, dtype), (shape, dtype, F))
