"""Batch sizes at which a kernel's grid map and grid loops turn, on the GPU, bit for bit against the CPU oracle.

1. Folded batches: every row of tests/batch_cases.py at every frame count of the row -- the whole rounds of the
   chunk map, the seam to its tail, two rounds, workgroups whose waves belong to two frames, a partial last
   workgroup, the XCD tail split and the stacked streamer's partial group (tests/test_batch_host.py shows on the CPU
   that the counts reach those regimes; here the live plan must say the same before anything is launched).  Every
   frame is noise of its own seed and one carries a flat band, so a workgroup that decodes the wrong frame, runs
   twice or never runs shows; the destination has padded rows, guard rows between the frames and a guard behind the
   batch, all of which must keep their sentinel.
2. Grid-stride trips: each of the 18 instantiations of the second-pass kernels (yuv_rgb_kernel 12, rgb_yuv_kernel 4,
   planes_norm_kernel 2) in one call of more than one and one of more than two times GRID_STRIDE_BLOCKS x 256 items,
   so that the stride loop takes its second and third trip, starting mid-frame and mid-row.
3. iqo_hip_resize_device_norm past 65535 frames per launch, and the byte output of the same packed plan.

Small shapes throughout: the batch sizes are the smallest at which these paths turn.
"""
import numpy as np
import pytest

import batch_cases as bc
import norm_cases as nc
import packed_cases as pc
import planes_norm_cases as pn
import rgbyuv_cases as ry
import yuv444_cases as y4
import yuvrgb_cases as yr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0xA5
GUARD_ROWS = 3
GUARD = 256
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}
SCALE, BIAS = nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]
CAP = libiqo_amd.GRID_STRIDE_BLOCKS


def _up(v, a):
    return (v + a - 1) // a * a


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


# ---- 1. folded batches

@pytest.mark.parametrize("row", bc.ROWS, ids=bc.rid)
def test_folded_batch_matches_oracle(row):
    body, method, degree, C, sw, sh, dw, dh, px, options, claims = row
    r = libiqo_amd.make_resizer(method, degree, sw, sh, dw, dh, px, channels=C)
    for k, v in options:
        r.set_option(k, v)
    # -- the live plan launches what the host query said, and reaches what the table claims: before any launch
    for n, want in sorted(claims.items()):
        g = r.launch_grid(n)
        assert g == libiqo_amd.host_launch_grid(*bc.query_args(row, n)), (n, g)
        assert bc.regimes(g) == want and g["family"] == bc.BODIES[body][0] == r.describe()["kernel"], (n, g)
    # -- layout: 16-byte aligned source rows; destination rows of dw C + pad bytes, guard rows between the frames, a
    # guard behind the batch, all sentinel
    s_st = _up(sw * C, 16)
    d_st = _up(dw * C + 3, 16) + 16
    f_st = d_st * (dh + GUARD_ROWS)
    for n in sorted(claims):
        frames, exp = bc.batch_for(row, n)
        src = torch.full((n, sh, s_st), 0x5A, dtype=torch.uint8, device=DEV)
        src[:, :, :sw * C] = torch.from_numpy(frames.reshape(n, sh, sw * C)).to(DEV)
        dst = torch.full((n * f_st + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
        r.resize_device(n, s_st, s_st * sh, src, d_st, f_st, dst)
        torch.cuda.synchronize()
        out = dst.cpu().numpy()
        img = out[:n * f_st].reshape(n, dh + GUARD_ROWS, d_st)
        got = img[:, :dh, :dw * C].copy()
        what = "%s x%d (%s)" % (bc.rid(row), n, claims[n])
        wrong = np.flatnonzero((got.reshape(n, -1) != exp.reshape(n, -1)).any(axis=1))
        assert wrong.size == 0, "%s: frames %s differ from the oracle" % (what, wrong[:16].tolist())
        img[:, :dh, :dw * C] = SENTINEL
        assert (out == SENTINEL).all(), "%s: wrote outside the images (padding, guard rows or past the batch)" % what


# ---- 2. grid-stride trips of the second-pass kernels

def _cycle(a, n):
    """Frames 0 .. n-1 of the cycle through a's frames."""
    return a[np.arange(n) % a.shape[0]]


def _guarded(nbytes):
    buf = torch.full((nbytes + GUARD,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert buf.numel() < bc.MAX_BUFFER
    return buf


def _guard_ok(buf, nbytes):
    return bool((buf[nbytes:] == SENTINEL).all())


YUV_FORMS = ("bytes", "px4", "px8")


@pytest.mark.parametrize("form", YUV_FORMS)
@pytest.mark.parametrize("chroma", ["replicate", "full"])
@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_yuv_rgb_grid_stride(layout, chroma, form):
    """yuv_rgb_kernel<UV2, NORM, PX, C444>: one instantiation per parameter set, two calls each."""
    for k, (shape, times) in enumerate(bc.STRIDE_YUV):
        m, d, sw, sh, dw, dh = shape
        case = shape + (layout,)
        standard = yr.STANDARDS[(k + YUV_FORMS.index(form)) % 4]
        rgb = (y4.expected_rgb if chroma == "full" else yr.expected_rgb)(case, standard)
        frames = y4.frames(case)
        n, period = bc.stride_plan("yuv_rgb", shape, 4 if form == "px4" else 8, times, CAP, (frames.shape[0],))
        cls = libiqo_amd.Nv12Resizer if layout == "nv12" else libiqo_amd.Yuv420Resizer
        r = cls(m, d, sw, sh, dw, dh, chroma=chroma)
        assert libiqo_amd.yuv_rgb_workspace_bytes(dw, dh, n, chroma) < bc.MAX_BUFFER
        src = torch.from_numpy(frames).to(DEV)[torch.arange(n, device=DEV) % period].contiguous()
        assert src.numel() < bc.MAX_BUFFER
        what = (layout, chroma, form, shape, n)
        if form == "bytes":
            order = ("bgr", "rgba")[k]
            C = len(yr.ORDERS[order])
            buf = _guarded(n * dh * dw * C)
            out = buf[:n * dh * dw * C].view(n, dh, dw, C)
            r.resize_rgb(src, standard=standard, order=order, out=out)
            torch.cuda.synchronize()
            _same(out.cpu().numpy(), _cycle(yr.reorder(rgb, yr.ORDERS[order]), n), what)
        else:
            dtype = "float32" if form == "px4" else ("float16", "bfloat16")[k]
            e = nc.ELEM[dtype]
            buf = _guarded(n * 3 * dh * dw * e)
            out = buf[:n * 3 * dh * dw * e].view(TORCH_DTYPE[dtype]).view(n, 3, dh, dw)
            r.resize_normalized(src, SCALE, BIAS, standard=standard, dtype=TORCH_DTYPE[dtype], out=out)
            torch.cuda.synchronize()
            _same(_bits(out), _cycle(nc.expected_bits(rgb, (0, 1, 2), SCALE, BIAS, dtype), n), what)
        assert _guard_ok(buf, buf.numel() - GUARD), what


@pytest.mark.parametrize("C,layout", ry.COMBOS, ids=["c%d-%s" % c for c in ry.COMBOS])
def test_rgb_yuv_grid_stride(C, layout):
    """rgb_yuv_kernel<C, UV2>: items are 8 pixels of a row pair."""
    for k, (shape, times) in enumerate(bc.STRIDE_RGB_YUV):
        m, d, sw, sh, dw, dh, _ = shape
        order = ("rgb", "bgr")[(k + C) % 2]
        standard = ry.STANDARDS[(k + C + (layout == "nv12")) % 4]
        n, period = bc.stride_plan("rgb_yuv", shape, 8, times, CAP)
        frames = pc.frames_for(shape, C, period)
        resized = np.stack([pc.oracle_packed(shape, f) for f in frames])
        exp = ry.tight(layout, *ry.rgb_to_yuv420(standard, resized[..., list(ry.ORDERS[order])]))
        assert libiqo_amd.rgb_yuv_workspace_bytes(dw, dh, C, n) < bc.MAX_BUFFER
        r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, 1, channels=C)
        src = torch.from_numpy(frames).to(DEV)[torch.arange(n, device=DEV) % period].contiguous()
        assert src.numel() < bc.MAX_BUFFER
        nbytes = n * exp.shape[1]
        buf = _guarded(nbytes)
        out = buf[:nbytes].view(n, exp.shape[1])
        (r.resize_nv12 if layout == "nv12" else r.resize_i420)(src, standard=standard, order=order, out=out)
        torch.cuda.synchronize()
        _same(out.cpu().numpy(), _cycle(exp, n), (C, layout, shape, n))
        assert _guard_ok(buf, nbytes), (C, layout, shape, n)


@pytest.mark.parametrize("dtype", nc.DTYPES)
def test_planes_norm_grid_stride(dtype):
    """planes_norm_kernel<4> (float32) and <8> (float16, bfloat16)."""
    px = 4 if dtype == "float32" else 8
    e = nc.ELEM[dtype]
    for shape, times in bc.STRIDE_PLANES:
        m, d, sw, sh, dw, dh = shape
        n, period = bc.stride_plan("planes_norm", shape, px, times, CAP)
        u8 = pn.expected_u8(shape, 3, period)
        exp = pn.expected_bits(u8, (2, 0, 1), SCALE, BIAS, dtype)
        r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, 1)
        src = torch.from_numpy(np.array(pn.frames_for(shape, 3, period))).to(DEV)[torch.arange(n, device=DEV) % period]
        src = src.contiguous()
        nbytes = n * 3 * dh * dw * e
        assert src.numel() < bc.MAX_BUFFER and libiqo_amd.planes_norm_workspace_bytes(dw, dh, 3, n) < bc.MAX_BUFFER
        buf = _guarded(nbytes)
        out = buf[:nbytes].view(TORCH_DTYPE[dtype]).view(n, 3, dh, dw)
        r.resize_planes_normalized(src, SCALE, BIAS, dtype=TORCH_DTYPE[dtype], order=(2, 0, 1), out=out)
        torch.cuda.synchronize()
        _same(_bits(out), _cycle(exp, n), (dtype, shape, n))
        assert _guard_ok(buf, nbytes), (dtype, shape, n)


# ---- 3. more frames than one launch takes, through the float entry of a packed plan

def test_norm_entry_past_65535_frames():
    """iqo_hip_resize_device_norm splits a batch into launches of 65535 frames (abi.hip run_norm), as
    iqo_hip_resize_device does (run_band): frames on both sides of the seam, the first and the last."""
    shape = ("lanczos", 2, 8, 4, 4, 2, 1)
    m, d, sw, sh, dw, dh, px = shape
    n, C = 70000, 3
    probe = (0, 65534, 65535, 65536, 69999)
    r = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)
    assert r.describe()["kernel"] in ("packed_tile", "packed_general")
    assert r.launch_grid(n)["frames"] == 65535
    g = torch.Generator(device=DEV)
    g.manual_seed(7)
    src = torch.randint(0, 256, (n, sh, sw, C), dtype=torch.uint8, device=DEV, generator=g)
    exp = np.stack([pc.oracle_packed(shape, src[f].cpu().numpy()) for f in probe])
    nbytes = n * C * dh * dw * 4
    buf = _guarded(nbytes)
    out = buf[:nbytes].view(torch.float32).view(n, C, dh, dw)
    r.resize_normalized(src, SCALE, BIAS, out=out)
    u8 = r.resize_tensor(src)
    torch.cuda.synchronize()
    idx = torch.tensor(probe, device=DEV)
    _same(u8[idx].cpu().numpy(), exp, "bytes")
    _same(_bits(out[idx]), nc.expected_bits(exp, (0, 1, 2), SCALE, BIAS, "float32"), "float32")
    assert _guard_ok(buf, nbytes)
    # every other frame too: the float output is norm_cases' map of the byte output, frame by frame
    _same(_bits(out), nc.expected_bits(u8.cpu().numpy(), (0, 1, 2), SCALE, BIAS, "float32"), "float32 of the bytes")
