"""Extreme inputs on the GPU: every Lanczos kernel family on the frames of tests/extreme_cases.py (tap-sign
and border-stress frames, one noise frame as the control), bit for bit against the CPU oracle.

tests/test_extreme_host.py shows, without a GPU, that these frames reach both clamps of both passes, the
analytic extreme of each pass, negative border numerators and denominators and wrapping border quotients,
that the host tables and the arithmetic model hold there, and that the oracle equals the reference.  What
is left for this file is the GPU code itself at those values: the intrinsics, the packing, the saturating
shifts and the neighbour exchange.  A case whose plan is not the kernel the table names fails.
"""
import numpy as np
import pytest

import extreme_cases as ec

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")


def _same(got, exp, what):
    """got / exp: arrays of one shape, frame first."""
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, first at %s: got %s want %s" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def _make(c, options=()):
    r = libiqo_amd.LanczosResizer(c.d, c.sw, c.sh, c.dw, c.dh, c.px)
    for k, v in options:
        r.set_option(k, v)
    return r


def _batches(c):
    """(frame indices of each call): the whole set at once, or -- the frame-stacked cases -- calls of c.batch
    frames, the set repeated until it fills them."""
    n = ec.frames_of(c)[1].shape[0]
    if not c.batch:
        return [list(range(n))]
    total = -(-n // c.batch) * c.batch
    idx = [i % n for i in range(total)]
    return [idx[i:i + c.batch] for i in range(0, total, c.batch)]


def _check(c, r, what):
    names, frames = ec.frames_of(c)
    exp = ec.expected_of(c)
    for idx in _batches(c):
        src = torch.from_numpy(np.array(frames[idx])).to(DEV)
        out = r.resize_tensor(src).cpu().numpy()
        for k, i in enumerate(idx):
            _same(out[k], exp[i], "%s %s frame %d (%s)" % (ec.cid(c), what, k, names[i]))


@pytest.mark.parametrize("c", ec.PLANAR, ids=ec.cid)
def test_planar_kernel_on_extreme_frames(c):
    r = _make(c)
    assert r.describe()["kernel"] == c.kernel
    _check(c, r, "default")
    for bands in (1, 3):  # border rows at band starts
        _check(c, _make(c, [("bands", bands)]), "bands %d" % bands)
    if c.batch:  # the frame-stacked streamer, as test_frame_stacked_streamer_matches_oracle sets it
        for stack, bands in ((2, 0), (2, 1), (2, 3), (1, 0), (0, 0)):
            r = _make(c, [("stack", stack), ("bands", bands)])
            assert r.describe()["kernel"] == c.kernel
            _check(c, r, "stack %d bands %d" % (stack, bands))
    if c.stream:  # every streamer test_stream_variants_agree_with_oracle selects by option
        for variant, pd, lanes, bands in ec.STREAM_OPTIONS:
            r = _make(c, [("stream_variant", variant), ("prefetch", pd), ("lanes", lanes), ("bands", bands)])
            assert r.describe()["kernel"] == c.kernel
            _check(c, r, "variant %d prefetch %d lanes %d bands %d" % (variant, pd, lanes, bands))


@pytest.mark.parametrize("c", ec.PLANAR, ids=ec.cid)
def test_planar_row_bands_through_source_windows(c):
    names, frames = ec.frames_of(c)
    exp = ec.expected_of(c)
    n = frames.shape[0]
    src = torch.from_numpy(frames.copy()).to(DEV)
    r = _make(c)
    assert r.describe()["kernel"] == c.kernel
    got = torch.zeros((n, c.dh, c.dw), dtype=torch.uint8, device=DEV)
    cuts = sorted({0, 1, c.dh // 2, c.dh})
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        s0, sn = r.band_src_rows(r0, r1 - r0)
        win = src[:, s0:s0 + sn].contiguous()
        r.resize_band(n, r0, r1 - r0, s0, c.sw, sn * c.sw, win.data_ptr(), c.dw, c.dh * c.dw, got[:, r0].data_ptr())
    torch.cuda.synchronize()
    _same(got.cpu().numpy(), exp, "%s row bands %s" % (ec.cid(c), cuts))


@pytest.mark.parametrize("c", [c for c in ec.PLANAR if c.kernel not in ("general", "lanczos_stream")], ids=ec.cid)
def test_tile_kernel_on_extreme_frames(c):
    """The exact-ratio kernels and the walker off: the separable tile kernel (general_kernel where the tile
    tables do not take the shape).  The 2:1 streamer has no switch: its shapes reach the tile tables only
    through their CPU emulation (tests/test_extreme_host.py)."""
    r = _make(c, [(k, 0) for k in ec.TILE_OPTIONS])
    assert r.describe()["kernel"] == ("tile" if c.tile else "general")
    _check(c, r, "tile")


@pytest.mark.parametrize("c", ec.PLANAR, ids=ec.cid)
def test_general_kernel_on_extreme_frames(c):
    r = _make(c, [("force_general", 1)])
    assert r.describe()["kernel"] == "general"
    _check(c, r, "force_general")


@pytest.mark.parametrize("row", ec.PACKED, ids=lambda r: "%s-L%d-%dx%d-C%d" % (r[0], r[1], r[2], r[3], r[6]))
def test_packed_kernels_on_extreme_frames(row):
    """Each channel of a pixel carries another frame of the set: a leak between channels shows."""
    kernel, d, sw, sh, dw, dh, C, norm = row
    frames, exp = ec.packed_frames(d, sw, sh, dw, dh, C)
    r = libiqo_amd.LanczosResizer(d, sw, sh, dw, dh, 1, channels=C)
    assert r.describe()["kernel"] == kernel and r.describe()["channels"] == C
    src = torch.from_numpy(frames).to(DEV)
    _same(r.resize_tensor(src).cpu().numpy(), exp, "%s C=%d" % (kernel, C))
    if norm:  # the normalising epilogue: scale 1, bias 0 in float32 is the byte itself
        out = r.resize_normalized(src, (1.0,) * C, (0.0,) * C).cpu().numpy()
        _same(out, exp.transpose(0, 3, 1, 2).astype(np.float32), "%s C=%d normalized" % (kernel, C))


def _tight(*planes):
    n = planes[0].shape[0]
    return np.concatenate([p.reshape(n, -1) for p in planes], axis=1)


@pytest.mark.parametrize("case", ec.FUSED, ids=lambda c: "%s-L%d-%dx%d" % (c[6], c[1], c[2], c[3]))
def test_fused_i420_on_extreme_frames(case):
    m, d, sw, sh, dw, dh, label = case
    y, u, v, ye, ue, ve = ec.yuv_planes(case)
    n = y.shape[0]
    assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == label
    r = libiqo_amd.Yuv420Resizer(m, d, sw, sh, dw, dh)
    out, fused = r.resize_frames(torch.from_numpy(_tight(y, u, v)).to(DEV))
    assert fused, label
    out = out.cpu().numpy()
    a, b = dw * dh, dw * dh + (dw // 2) * (dh // 2)
    _same(out[:, :a].reshape(n, dh, dw), ye, label + " Y")
    _same(out[:, a:b].reshape(n, dh // 2, dw // 2), ue, label + " U")
    _same(out[:, b:].reshape(n, dh // 2, dw // 2), ve, label + " V")


def test_nv12_on_extreme_frames():
    m, d, sw, sh, dw, dh = ec.NV12
    y, u, v, ye, ue, ve = ec.yuv_planes(ec.NV12)
    n = y.shape[0]
    r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
    assert r.describe() == (libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, 1), "packed_tile")
    uv = np.stack([u, v], axis=3)
    out = r.resize_frames(torch.from_numpy(_tight(y, uv)).to(DEV)).cpu().numpy()
    _same(out[:, :dw * dh].reshape(n, dh, dw), ye, "NV12 Y")
    ouv = out[:, dw * dh:].reshape(n, dh // 2, dw // 2, 2)
    _same(ouv[..., 0], ue, "NV12 U")
    _same(ouv[..., 1], ve, "NV12 V")
