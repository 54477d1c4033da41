"""GPU parity of the normalised planar float output of the packed resize
(iqo_hip_resize_device_norm / resize_normalized): plane p of the result is, bit for bit,

    cvt(fl32(fl32(float(u8[..., order[p]]) * scale[p]) + bias[p]))

of the per-channel oracle's bytes (packed_cases) -- through packed_tile_kernel's and
packed_general_kernel's float epilogues, over every tile instantiation, the tile geometries, padded and
misaligned destinations, channel orders, the error paths, streams and out=.  Bit patterns are compared,
never allclose.  Small shapes, 2 frames (3 with the constant-channel frame): well under a second each."""
import ctypes
import os

import numpy as np
import pytest

import norm_cases as nc
import packed_cases as pc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
os.environ["IQO_REQUIRE_HIP"] = "1"
SENTINEL = 0xA5
CHANNELS = [2, 3, 4]
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
EINVAL, EUNSUP = -1, -5


def _make(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    return libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)


def _bits(t):
    """Bit patterns of a float tensor as a numpy integer array."""
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _check(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first [frame, plane, y, x] %s" % (what, len(bad), bad[:4].tolist())


def _identity(C):
    return tuple(range(C)), nc.NORM_SCALE[:C], nc.NORM_BIAS[:C]


def _both_kernels(r, tile_expected=True):
    """The resizer set to packed_tile, then to packed_general; describe() is asserted each time."""
    for force, name in ((0, "packed_tile"), (1, "packed_general")):
        r.set_option("force_general", force)
        if force == 0 and not tile_expected:
            continue
        assert r.describe()["kernel"] == name
        yield name


# ---- 1. every packed_tile_kernel<C, NP, LZ, NORM = true> instantiation

@pytest.mark.parametrize("idx", range(len(pc.INSTANTIATIONS)), ids=lambda i: pc.cell_id(pc.INSTANTIATIONS[i]))
def test_norm_every_instantiation(idx):
    shape, C, CT, TH, NP = pc.INSTANTIATIONS[idx]
    order, scale, bias = _identity(C)
    u8 = pc.expected_for(shape, C)
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    r = _make(shape, C)
    assert r.describe()["tile_rows"] == TH
    # fp32 everywhere; fp16 on even rows and bf16 on odd rows: C cycles with period 3, so every
    # (C, LZ) sees both half types
    for dtype in ("float32", "float16" if idx % 2 == 0 else "bfloat16"):
        exp = nc.expected_bits(u8, order, scale, bias, dtype)
        for kernel in _both_kernels(r):
            out = r.resize_normalized(src, scale, bias, dtype=TORCH_DTYPE[dtype])
            assert out.dtype == TORCH_DTYPE[dtype] and tuple(out.shape) == (2, C) + u8.shape[1:3]
            _check(_bits(out), exp, (pc.cell_id(pc.INSTANTIATIONS[idx]), dtype, kernel))


# ---- 2. tile geometry: partial last tiles in both axes, dstW % 4 != 0 (per-element tail stores)

@pytest.mark.parametrize("row", pc.GEOMETRY + pc.LANCZOS_WIDE_UPSCALES, ids=pc.cell_id)
def test_norm_tile_geometries(row):
    shape, C, CT, TH, NP = row
    order, scale, bias = _identity(C)
    r = _make(shape, C)
    desc = r.describe()
    assert desc["kernel"] == "packed_tile" and desc["tile_rows"] == TH
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    out = r.resize_normalized(src, scale, bias)
    _check(_bits(out), nc.expected_bits(pc.expected_for(shape, C), order, scale, bias, "float32"), pc.cell_id(row))


# ---- 3. layouts: base one element off a 64-byte boundary, padded rows, planes and frames, guards

def _norm_struct(dtype, order, scale, bias):
    n = libiqo_amd.Norm(nc.CODE[dtype], len(order))
    for i, (c, s, b) in enumerate(zip(order, scale, bias)):
        n.order[i], n.scale[i], n.bias[i] = c, s, b
    return n


def _call(r, nframes, src, norm, row_st, plane_st, frame_st, dst_ptr, stream=None):
    sw, C = r.srcW, r.channels
    return libiqo_amd.lib().iqo_hip_resize_device_norm(r._plan, nframes, sw * C, r.srcH * sw * C, src.data_ptr(),
                                                       ctypes.byref(norm), row_st, plane_st, frame_st, dst_ptr, stream)


@pytest.mark.parametrize("kernel", ["packed_tile", "packed_general"])
@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", [pc.SHAPES[0], pc.SHAPES[9]], ids=pc.sid)
def test_norm_padded_misaligned_layout(shape, C, dtype, kernel):
    m, d, sw, sh, dw, dh, px = shape
    n, e = 2, nc.ELEM[dtype]
    order, scale, bias = _identity(C)
    row_st = (dw + 1) * e
    plane_st = dh * row_st + 3 * e
    frame_st = C * plane_st + 5 * e
    G = 64
    buf = torch.full((64 + G + e + n * frame_st + G,), SENTINEL, dtype=torch.uint8, device=DEV)
    base = (-buf.data_ptr()) % 64 + G + e  # one element past a 64-byte boundary
    assert (buf.data_ptr() + base - e) % 64 == 0
    r = _make(shape, C)
    r.set_option("force_general", int(kernel == "packed_general"))
    assert r.describe()["kernel"] == kernel
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    rc = _call(r, n, src, _norm_struct(dtype, order, scale, bias), row_st, plane_st, frame_st, buf.data_ptr() + base)
    assert rc == 0
    torch.cuda.synchronize()
    full = buf.cpu().numpy()
    payload = np.zeros(full.shape, bool)
    got = np.empty((n, C, dh, dw), np.int32 if e == 4 else np.int16)
    for f in range(n):
        for p in range(C):
            for y in range(dh):
                o = base + f * frame_st + p * plane_st + y * row_st
                payload[o:o + dw * e] = True
                got[f, p, y] = full[o:o + dw * e].view(got.dtype)
    _check(got, nc.expected_bits(pc.expected_for(shape, C), order, scale, bias, dtype), (shape, C, dtype, kernel))
    # row padding, plane gaps, frame gaps and both guards
    stray = np.flatnonzero(~payload & (full != SENTINEL))
    assert stray.size == 0, (shape, C, dtype, kernel, "wrote outside the payload at byte offsets (from the base)",
                             (stray[:8] - base).tolist())
    assert payload[:base].sum() == 0 and (full[base - e - G:base] == SENTINEL).all()
    assert (full[base + n * frame_st:base + n * frame_st + G] == SENTINEL).all()


# ---- 4. order and planes

def _three_frames(shape, C):
    """frames_for's two frames and the constant-channel frame, with the oracle's bytes."""
    const = pc.const_frame(shape, C)
    frames = np.concatenate([pc.frames_for(shape, C), const[None]])
    exp = np.concatenate([pc.expected_for(shape, C), pc.oracle_packed(shape, const)[None]])
    return frames, exp


ORDER_CASES = [
    # (C, order, scale, bias)
    (4, (2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]),                   # BGRA -> RGB, alpha dropped
    (3, (2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]),
    (2, (1,), nc.NORM_SCALE[3:4], nc.NORM_BIAS[3:4]),
    (3, (0, 0, 0), nc.NORM_SCALE[:3], (nc.NORM_BIAS[2], nc.NORM_BIAS[0], nc.NORM_BIAS[3])),  # one channel, three maps
]


@pytest.mark.parametrize("dtype", nc.DTYPES)
@pytest.mark.parametrize("case", ORDER_CASES, ids=lambda c: "c%d-order%s" % (c[0], "".join(map(str, c[1]))))
def test_norm_order_and_planes(case, dtype):
    C, order, scale, bias = case
    shape = pc.SHAPES[0]
    m, d, sw, sh, dw, dh, px = shape
    assert len({(s, b) for s, b in zip(scale, bias)}) == len(order)
    frames, u8 = _three_frames(shape, C)  # the constant frame shows a wrong channel pick as cross-talk
    exp = nc.expected_bits(u8, order, scale, bias, dtype)
    src = torch.from_numpy(frames).to(DEV)
    r = _make(shape, C)
    P = len(order)
    for kernel in _both_kernels(r):
        # one sentinel plane behind every frame's output planes
        big = torch.empty((3, P + 1, dh, dw), dtype=TORCH_DTYPE[dtype], device=DEV)
        big.view(torch.uint8).fill_(SENTINEL)
        out = r.resize_normalized(src, scale, bias, dtype=TORCH_DTYPE[dtype], order=order, out=big[:, :P])
        assert out.data_ptr() == big.data_ptr() and tuple(out.shape) == (3, P, dh, dw)
        torch.cuda.synchronize()
        _check(_bits(big[:, :P]), exp, (case, dtype, kernel))
        assert (big[:, P].contiguous().view(torch.uint8) == SENTINEL).all(), (case, dtype, kernel, "sentinel plane")


# ---- 5. ties to the U8 path: scale 1, bias 0, fp32 is the U8 result as floats

@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", pc.SHAPES + [pc.GENERAL_SHAPE], ids=pc.sid)
def test_norm_unit_map_equals_the_u8_path(shape, C):
    r = _make(shape, C)
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    u8 = r.resize_tensor(src)
    out = r.resize_normalized(src, (1.0,) * C, (0.0,) * C)
    assert out.dtype == torch.float32
    assert torch.equal(out, u8.permute(0, 3, 1, 2).float()), (shape, C, r.describe()["kernel"])
    single = r.resize_normalized(src[1], (1.0,) * C, (0.0,) * C)  # [H, W, C] -> [C, H, W]
    assert tuple(single.shape) == tuple(out.shape[1:]) and torch.equal(single, out[1])


# ---- 6. errors: rejected on the host before any launch, the destination untouched

def _error_setup(C=3, dtype="float32"):
    shape = pc.SHAPES[0]
    m, d, sw, sh, dw, dh, px = shape
    r = _make(shape, C)
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    e = nc.ELEM[dtype]
    dst = torch.full((2 * C * dh * dw * e + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    return r, src, dst, (dw * e, dh * dw * e, C * dh * dw * e)


def _untouched(dst):
    torch.cuda.synchronize()
    return bool((dst == SENTINEL).all())


def test_norm_abi_errors():
    C = 3
    r, src, dst, (row, plane, frame) = _error_setup(C)
    order, scale, bias = _identity(C)
    good = lambda: _norm_struct("float32", order, scale, bias)  # noqa: E731
    dw, dh = r.dstW, r.dstH
    L = libiqo_amd.lib()
    sst, sfst = r.srcW * C, r.srcH * r.srcW * C

    def call(plan=r._plan, n=2, s=src.data_ptr(), norm=None, rs=row, ps=plane, fs=frame, d=dst.data_ptr(), sst=sst):
        nm = ctypes.byref(norm) if norm is not None else None
        return L.iqo_hip_resize_device_norm(plan, n, sst, sfst, s, nm, rs, ps, fs, d, None)

    def variant(**kw):
        n = good()
        for k, v in kw.items():
            if isinstance(v, tuple):
                getattr(n, k)[v[0]] = v[1]
            else:
                setattr(n, k, v)
        return n

    cases = {
        "null plan": call(plan=None, norm=good()),
        "null source": call(s=None, norm=good()),
        "null destination": call(d=None, norm=good()),
        "null norm": call(norm=None),
        "dtype 0": call(norm=variant(dtype=0)),
        "dtype 4": call(norm=variant(dtype=4)),
        "planes 0": call(norm=variant(planes=0)),
        "planes 5": call(norm=variant(planes=5)),
        "order = channels": call(norm=variant(order=(1, C))),
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
        "source stride < srcW * channels": call(norm=good(), sst=sst - 1),
        "float frame of 2^31 bytes": call(norm=good(), n=1, ps=1 << 30, fs=3 << 30),
        "plane stride of 2^31 bytes": call(norm=variant(planes=1), n=1, ps=1 << 31, fs=1 << 31),
    }
    assert {k: v for k, v in cases.items() if v != EINVAL} == {}
    assert _untouched(dst)
    # the half types: element size 2
    n16 = _norm_struct("float16", order, scale, bias)
    assert call(norm=n16, rs=dw * 2, ps=dh * dw * 2, fs=C * dh * dw * 2, d=dst.data_ptr() + 1) == EINVAL
    assert call(norm=n16, rs=dw * 2 + 1, ps=dh * (dw * 2 + 1) + 1, fs=4 * dh * (dw * 2 + 2)) == EINVAL
    assert call(norm=n16, rs=dw * 2 - 2, ps=dh * dw * 2, fs=C * dh * dw * 2) == EINVAL
    assert _untouched(dst)
    # frames = 1: the frame stride is not compared with the planes (it is unused)
    assert call(norm=good(), n=1, fs=0) == 0
    torch.cuda.synchronize()
    assert not _untouched(dst)


def test_norm_one_channel_plan_is_unsupported():
    shape = pc.SHAPES[0]
    m, d, sw, sh, dw, dh, px = shape
    r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px)
    src = torch.zeros((1, sh, sw), dtype=torch.uint8, device=DEV)
    dst = torch.full((dh * dw * 4,), SENTINEL, dtype=torch.uint8, device=DEV)
    n = _norm_struct("float32", (0,), (1.0,), (0.0,))
    rc = libiqo_amd.lib().iqo_hip_resize_device_norm(r._plan, 1, sw, sh * sw, src.data_ptr(), ctypes.byref(n), dw * 4,
                                                     dh * dw * 4, dh * dw * 4, dst.data_ptr(), None)
    assert rc == EUNSUP
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_normalized(src, (1.0,), (0.0,))
    assert _untouched(dst)


def test_norm_python_errors():
    C = 3
    shape = pc.SHAPES[0]
    m, d, sw, sh, dw, dh, px = shape
    r = _make(shape, C)
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    order, scale, bias = _identity(C)
    out = torch.empty((2, C, dh, dw), dtype=torch.float32, device=DEV)
    out.view(torch.uint8).fill_(SENTINEL)
    bad = [
        dict(scale=scale, bias=bias, order=(0, 1, 3)),                       # ABI: order out of range
        dict(scale=scale, bias=bias, order=(0, 1, -1)),
        dict(scale=(float("inf"),) + tuple(scale[1:]), bias=bias),           # ABI: non-finite
        dict(scale=scale, bias=(0.0, float("nan"), 0.0)),
        dict(scale=scale[:2], bias=bias),                                    # lengths
        dict(scale=scale, bias=bias, order=(0, 1)),
        dict(scale=scale * 2, bias=bias * 2, order=(0, 1, 2, 0, 1, 2)),      # planes > 4
        dict(scale=(), bias=(), order=()),
        dict(scale=scale, bias=bias, dtype=torch.float64),
        dict(scale=scale, bias=bias, dtype=torch.float16),                   # out is float32
    ]
    for kw in bad:
        with pytest.raises(libiqo_amd.IqoError):
            r.resize_normalized(src, out=out, **kw)
    with pytest.raises(libiqo_amd.IqoError):  # a planar tensor
        r.resize_normalized(src[..., 0], scale, bias, out=out)
    with pytest.raises(libiqo_amd.IqoError):  # overlapping rows
        r.resize_normalized(src, scale, bias, out=out.as_strided((2, C, dh, dw), (C * dh * dw, dh * dw, dw - 1, 1)))
    with pytest.raises(libiqo_amd.IqoError):  # column stride 2
        r.resize_normalized(src, scale, bias, out=torch.empty((2, C, dh, 2 * dw), dtype=torch.float32,
                                                              device=DEV)[..., ::2])
    with pytest.raises(libiqo_amd.IqoError):  # wrong plane count
        r.resize_normalized(src, scale, bias, out=out[:, :2])
    torch.cuda.synchronize()
    assert (out.view(torch.uint8) == SENTINEL).all()
    r.resize_normalized(src, scale, bias, out=out)
    _check(_bits(out), nc.expected_bits(pc.expected_for(shape, C), order, scale, bias, "float32"), "after the errors")


# ---- 7. a non-default stream and a strided out=

@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_norm_stream_and_strided_out(dtype):
    C = 3
    shape = pc.SHAPES[7]  # several tiles in both axes
    m, d, sw, sh, dw, dh, px = shape
    order, scale, bias = (2, 1, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
    r = _make(shape, C)
    r.prepare()
    assert r.describe()["kernel"] == "packed_tile"
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    big = torch.empty((3, 5, dh + 3, dw + 5), dtype=TORCH_DTYPE[dtype], device=DEV)
    big.view(torch.uint8).fill_(SENTINEL)
    view = big[1:3, 1:4, 2:2 + dh, 3:3 + dw]
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    assert stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
    with torch.cuda.stream(stream):
        out = r.resize_normalized(src, scale, bias, dtype=TORCH_DTYPE[dtype], order=order, out=view, stream=stream)
    assert out is view
    stream.synchronize()
    _check(_bits(view), nc.expected_bits(pc.expected_for(shape, C), order, scale, bias, dtype), (shape, dtype))
    mask = torch.ones(big.shape, dtype=torch.bool, device=DEV)
    mask[1:3, 1:4, 2:2 + dh, 3:3 + dw] = False
    outside = big.view(torch.int32 if dtype == "float32" else torch.int16)[mask]
    want = int(np.array([SENTINEL] * 4, np.uint8).view(np.int32)[0]) if dtype == "float32" else int(
        np.array([SENTINEL] * 2, np.uint8).view(np.int16)[0])
    assert (outside == want).all(), "wrote outside the strided view"
