"""Every template instantiation of the 1-channel ratio, tile and walker kernels, launched once at a small shape:
one test per row of tests/instance_cases.py, bit for bit against the CPU oracle.

tests/test_instance_host.py shows without a GPU that the table is complete and that every row's shape and options
select the row's instantiation in the host query.  Here the live plan must name the same instantiation before
anything is launched -- a test that silently ran another kernel fails there -- and then that instantiation runs:
on the tap-sign and border-stress frames (Lanczos) or noise, flat, checkerboard and half-flat frames (Area,
Linear); into a padded, sentinel-filled destination with guard rows; in 1, 3 and dstH bands and through row-band
source windows (trip and prefetch bookkeeping differs per instantiation); and from a misaligned source.
"""
import numpy as np
import pytest

import instance_cases as ic

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENTINEL = 0xA5
GUARD_ROWS = 3


def _same(got, exp, what, names=None):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d bytes differ, first at %s%s: got %s want %s" % (
        what, len(bad), tuple(bad[0]), " (%s)" % names[bad[0][0]] if names else "", got[tuple(bad[0])], exp[tuple(bad[0])])


def _make(row, more=()):
    _, _, method, degree, sw, sh, dw, dh, px, options = row
    r = libiqo_amd.make_resizer(method, degree, sw, sh, dw, dh, px)
    for k, v in tuple(options) + tuple(more):
        r.set_option(k, v)
    return r


def _up(v, a):
    return (v + a - 1) // a * a


def _source(frames, stride, offset=0):
    """The frames on the device with the given row stride, `offset` bytes into the allocation; (buffer, view)."""
    n, sh, sw = frames.shape
    buf = torch.full((offset + n * sh * stride,), 0x5A, dtype=torch.uint8, device=DEV)
    view = buf[offset:].view(n, sh, stride)
    view[:, :, :sw] = torch.from_numpy(np.array(frames)).to(DEV)
    return buf, view


@pytest.mark.parametrize("row", ic.ALL_ROWS, ids=ic.rid)
def test_instantiation_matches_oracle(row):
    kernel, params, method, degree, sw, sh, dw, dh, px, options = row
    want = ic.instance_of(row)
    names, frames = ic.frames_of(row)
    exp = ic.expected_of(row)
    n = frames.shape[0]
    sa, da = ic.align_of(kernel)

    # -- live query, before any launch
    r = _make(row)
    assert r.instance() == want and r.describe()["instance"] == want
    assert r.instance(sa, da) == want

    # -- layout: rows of dw + pad bytes, three guard rows between frames, a guard after the batch, all sentinel; base
    # and strides multiples of what the family needs and of nothing larger
    s_st = _up(sw, sa)
    _, src = _source(frames, s_st)
    d_st = _up(dw + 3, da)
    if d_st % (2 * da) == 0:
        d_st += da
    f_st = d_st * (dh + GUARD_ROWS)
    dst = torch.full((n * f_st + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    r.resize_device(n, s_st, s_st * sh, src, d_st, f_st, dst)
    torch.cuda.synchronize()
    out = dst.cpu().numpy()
    img = out[:n * f_st].reshape(n, dh + GUARD_ROWS, d_st)
    full = img[:, :dh, :dw].copy()
    _same(full, exp, "%s padded layout" % ic.rid(row), names)
    img[:, :dh, :dw] = SENTINEL
    assert (out == SENTINEL).all(), "%s: wrote outside the images (padding, guard rows or past the batch)" % ic.rid(row)

    # -- bands: the option, and row bands through their source windows
    for bands in (1, 3, dh):
        b = _make(row, [("bands", bands)])
        assert b.instance(sa, da) == want
        got = torch.full((n, dh, _up(dw, da)), SENTINEL, dtype=torch.uint8, device=DEV)
        b.resize_device(n, s_st, s_st * sh, src, got.shape[2], got.shape[2] * dh, got)
        torch.cuda.synchronize()
        _same(got.cpu().numpy()[:, :, :dw], full, "%s bands %d" % (ic.rid(row), bands), names)
    cuts = sorted({0, 1, dh // 3 + 1, dh - 2, dh})
    got = torch.full((n, dh, _up(dw, da)), SENTINEL, dtype=torch.uint8, device=DEV)
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        s0, sn = r.band_src_rows(r0, r1 - r0)
        assert 0 <= s0 and s0 + sn <= sh and sn >= 1
        r.resize_band(n, r0, r1 - r0, s0, s_st, s_st * sh, src[:, s0].data_ptr(), got.shape[2], got.shape[2] * dh,
                      got[:, r0].data_ptr())
    torch.cuda.synchronize()
    _same(got.cpu().numpy()[:, :, :dw], full, "%s row bands %s" % (ic.rid(row), cuts), names)

    # -- alignment: the kernels that take any source (byte offset 1, stride sw + 3); the walker's padded stride
    if kernel in ("ryx", "ryg", "ryu", "tile", "walk"):
        off, st = (0, _up(sw, 4) + 4) if kernel == "walk" else (1, sw + 3)
        assert r.instance(4 if kernel == "walk" else 1, 1) == want
        _, usrc = _source(frames, st, off)
        got = torch.full((n, dh, dw), SENTINEL, dtype=torch.uint8, device=DEV)
        r.resize_device(n, st, st * sh, usrc, dw, dw * dh, got)
        torch.cuda.synchronize()
        _same(got.cpu().numpy(), full, "%s source at offset %d, stride %d" % (ic.rid(row), off, st), names)


@pytest.mark.parametrize("case", ic.BAD_PREFETCH, ids=lambda c: "%s-pd%d" % (c[0], c[7]))
def test_uninstantiated_prefetch_depth_is_rejected(case):
    """A depth the family's kernel does not instantiate fails the resize call; it is never the default kernel."""
    kernel, method, degree, sw, sh, dw, dh, depth = case
    r = libiqo_amd.make_resizer(method, degree, sw, sh, dw, dh, 1)
    assert r.describe()["kernel"] == kernel
    r.set_option("ratio_prefetch", depth)
    assert r.describe()["instance"] is None
    with pytest.raises(libiqo_amd.IqoError):
        r.instance()
    src = torch.zeros((1, sh, sw), dtype=torch.uint8, device=DEV)
    dst = torch.full((1, dh, dw), SENTINEL, dtype=torch.uint8, device=DEV)
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_device(1, sw, sw * sh, src, dw, dw * dh, dst)
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == SENTINEL).all()
