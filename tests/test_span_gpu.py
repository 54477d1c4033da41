"""Every 1-channel kernel family, the two packed kernels and the I420 / NV12 entries at their address-range limits
(tests/span_cases.py): the largest layouts the launchers accept, the smallest they reject, and frames more than
2^31 and 2^32 bytes apart.

One source and one destination buffer of 2^32 + 2^25 bytes hold every layout, so each byte a layout names is
mapped.  An accepted call must give the CPU oracle's rows bit for bit and leave every other byte of the
destination buffer at 0xA5 -- a stray store anywhere in 4 GiB shows, in particular at byte 0x7ff00000, where the
buffer-addressed kernels send the accesses they drop.  A rejected call must raise IQO_HIP_EINVAL and leave the
whole buffer at 0xA5.  Kernel family and instantiation are asserted before each launch: a case that fell to
another family fails.
"""
import ctypes

import numpy as np
import pytest

import norm_cases as nc
import span_cases as sc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)
if torch.cuda.mem_get_info()[0] < 12 * 2 ** 30:  # pragma: no cover - an MI355X never does
    pytest.skip("needs 12 GiB of free device memory", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
A5 = 0xA5
A5_32 = int.from_bytes(b"\xa5" * 4, "little", signed=True)
A5_64 = int.from_bytes(b"\xa5" * 8, "little", signed=True)
CHUNK = 2 ** 27  # int64 elements per comparison: 1 GiB

ROWS = pytest.mark.parametrize("row", sc.ROWS, ids=sc.rid)


@pytest.fixture(scope="module")
def bufs():
    """(source, destination): torch.empty, only the rows a case names are ever written."""
    src = torch.empty(sc.BUF, dtype=torch.uint8, device=DEV)
    dst = torch.empty(sc.BUF, dtype=torch.uint8, device=DEV)
    yield src, dst
    del src, dst
    torch.cuda.empty_cache()


def _untouched(dst):
    """Every byte of the destination buffer is 0xA5 (compared on the device, 1 GiB at a time)."""
    v = dst.view(torch.int64)
    flags = [(v[i:i + CHUNK] != A5_64).any() for i in range(0, v.numel(), CHUNK)]
    if not bool(torch.stack(flags).any()):
        return
    for i in range(0, v.numel(), CHUNK):  # (failure only: where)
        bad = (v[i:i + CHUNK] != A5_64).nonzero()
        if bad.numel():
            at = 8 * (i + int(bad[0]))
            raise AssertionError("destination bytes outside the output rows were written: %d qwords in this GiB, first "
                                 "at byte 0x%x: %s" % (bad.shape[0], at, dst[at:at + 8].cpu().tolist()))


def _einval(exc):
    return str(exc.value).endswith("(-1)")  # IQO_HIP_EINVAL


def _same(got, exp, what):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d values differ, first at %s: got %s want %s" % (
        what, len(bad), tuple(bad[0]), got[tuple(bad[0])], exp[tuple(bad[0])])


def _make(row):
    r = libiqo_amd.make_resizer(row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px, channels=row.C)
    for k, v in row.options:
        r.set_option(k, v)
    d = r.describe()
    assert d["kernel"] == ("ryg" if row.kernel == "ryu" else row.kernel) and d["channels"] == row.C, d
    if isinstance(row.inst, dict):
        assert r.instance() == dict(row.inst, kernel=row.kernel)
    return r


def _src_view(buf, row, lay, rows0, rows):
    """Source rows [rows0, rows0 + rows) of every frame, where the layout puts them."""
    shape, st = (lay.frames, rows, row.sw), (lay.src_fst, lay.src_st, 1)
    if row.C > 1:
        shape, st = shape + (row.C,), (lay.src_fst, lay.src_st, row.C, 1)
    return torch.as_strided(buf, shape, st, rows0 * lay.src_st)


def _dst_view(buf, row, lay):
    """The output rows of every frame: bytes [F, rows, dw(, C)], or the int32 bit patterns [F, 3, dh, dw] of a
    normalised float frame (plane stride dh * row stride)."""
    if row.norm:
        assert lay.dst_st % 4 == 0 and lay.dst_fst % 4 == 0
        return torch.as_strided(buf.view(torch.int32), (lay.frames, 3, row.dh, row.dw),
                                (lay.dst_fst // 4, row.dh * lay.dst_st // 4, lay.dst_st // 4, 1))
    shape, st = (lay.frames, lay.rows, row.dw), (lay.dst_fst, lay.dst_st, 1)
    if row.C > 1:
        shape, st = shape + (row.C,), (lay.dst_fst, lay.dst_st, row.C, 1)
    return torch.as_strided(buf, shape, st, lay.r0 * lay.dst_st)


def _call(r, row, lay, src, dst):
    assert sc.fits(row, lay), "the buffers cover every byte the layout names"
    sp, dp = src.data_ptr() + lay.s0 * lay.src_st, dst.data_ptr() + lay.r0 * lay.dst_st
    if row.norm:
        n = libiqo_amd.Norm(nc.OUT_F32, 3)
        for i in range(3):
            n.order[i], n.scale[i], n.bias[i] = (2, 0, 1)[i], float(nc.NORM_SCALE[i]), float(nc.NORM_BIAS[i])
        libiqo_amd._check(libiqo_amd.lib().iqo_hip_resize_device_norm(
            r._plan, lay.frames, lay.src_st, lay.src_fst, sp, ctypes.byref(n), lay.dst_st, row.dh * lay.dst_st,
            lay.dst_fst, dp, None), "resize_normalized")
    elif (lay.r0, lay.rows) == (0, row.dh):
        r.resize_device(lay.frames, lay.src_st, lay.src_fst, sp, lay.dst_st, lay.dst_fst, dp)
    else:
        r.resize_band(lay.frames, lay.r0, lay.rows, lay.s0, lay.src_st, lay.src_fst, sp, lay.dst_st, lay.dst_fst, dp)


def _accepted(r, row, lay, bufs, what, is_far=False):
    """One launch in the layout: the oracle's rows bit for bit, and nothing else written."""
    src, dst = bufs
    frames, exp = sc.frames_of(row, lay.frames, is_far)
    dst.fill_(A5)
    _src_view(src, row, lay, lay.s0, lay.srows).copy_(torch.from_numpy(np.array(frames[:, lay.s0:lay.s0 + lay.srows])).to(DEV))
    _call(r, row, lay, src, dst)
    out = _dst_view(dst, row, lay)
    got = out.cpu().numpy()
    out.fill_(A5_32 if row.norm else A5)
    _untouched(dst)
    if row.norm:
        exp = nc.expected_bits(exp, (2, 0, 1), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3], "float32")
    else:
        exp = exp[:, lay.r0:lay.r0 + lay.rows]
    _same(got, exp, "%s %s" % (row.name, what))


@ROWS
def test_tight_layout(row, bufs):
    _accepted(_make(row), row, sc.tight(row), bufs, "tight")


@ROWS
def test_largest_accepted_source_layout(row, bufs):
    _accepted(_make(row), row, sc.src_top(row), bufs, "src_top")


@ROWS
def test_largest_accepted_destination_layout(row, bufs):
    _accepted(_make(row), row, sc.dst_top(row), bufs, "dst_top")


@ROWS
def test_frames_beyond_2g_and_4g(row, bufs):
    _accepted(_make(row), row, sc.far(row), bufs, "far", is_far=True)


@pytest.mark.parametrize("name", sc.BAND)
def test_band_of_a_frame_over_the_limit(name, bufs):
    row = sc.BY_NAME[name]
    _accepted(_make(row), row, sc.band(row), bufs, "band")


@pytest.mark.parametrize("row", [r for r in sc.ROWS if r.limits[0]], ids=sc.rid)
def test_smallest_rejected_layouts(row, bufs):
    src, dst = bufs
    r = _make(row)
    dst.fill_(A5)
    cases = sc.over(row)
    assert cases
    for which, lay in cases.items():
        assert not sc.accepted(row, lay)
        with pytest.raises(libiqo_amd.IqoError) as e:
            _call(r, row, lay, src, dst)
        assert _einval(e), (which, str(e.value))
    torch.cuda.synchronize()
    _untouched(dst)
    _accepted(r, row, sc.tight(row), bufs, "tight after the rejected calls")


# ----------------------------------------------------------------------------- I420 and NV12

# (entry, method, degree, sw, sh, dw, dh, fused label or None; the planes' kernels, Y and chroma)
YUV = [
    ("i420", "lanczos", 3, 64, 32, 32, 16, "lz_sym10", "lanczos_stream", "lanczos_stream"),
    ("i420", "area", 0, 64, 32, 32, 16, "area22", "area_int", "area_int"),
    ("i420", "lanczos", 3, 200, 140, 136, 132, "none", "ryg", "ryg"),     # plane by plane
    ("nv12", "lanczos", 3, 384, 216, 192, 108, None, "lanczos_stream", "packed_tile"),
]
LIMITS = {"lanczos_stream": sc.STREAM, "area_int": sc.UNLIMITED, "ryg": sc.RATIO, "packed_tile": sc.TILE}
YUV_CASES = pytest.mark.parametrize("case", YUV, ids=lambda c: "%s-%s%d-%dx%d" % c[:5])


def _yuv_planes(case, n, is_far):
    """[(source [n, h, w(, 2]), expected)] for the planes of the entry: Y, U, V or Y, UV."""
    entry, m, d, sw, sh, dw, dh = case[:7]
    get = sc.far_planes if is_far else sc.planes
    y = get(m, d, sw, sh, dw, dh, 1, n)
    c = get(m, d, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1, n + 1)
    u, v = (c[0][:n], c[1][:n]), (c[0][1:], c[1][1:])
    if entry == "nv12":
        return [y, (np.stack([u[0], v[0]], axis=3), np.stack([u[1], v[1]], axis=3))]
    return [y, u, v]


def _yuv_make(case):
    entry, m, d, sw, sh, dw, dh, label, ky, kc = case
    assert libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh) == ky
    if entry == "nv12":
        r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
        assert r.describe() == (ky, kc)
        return r
    assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == label
    assert libiqo_amd.host_kernel_for(m, d, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1) == kc
    return libiqo_amd.Yuv420Resizer(m, d, sw, sh, dw, dh)


def _yuv_call(r, case, n, sp, sst, sfst, dp, dstr, dfst, src, dst):
    """sp / dp: the planes' byte offsets in the buffers; sst / dstr: (Y stride, chroma stride)."""
    s, d = [src.data_ptr() + o for o in sp], [dst.data_ptr() + o for o in dp]
    if case[0] == "nv12":
        r.resize_device(n, sst[0], sst[1], sfst, s[0], s[1], dstr[0], dstr[1], dfst, d[0], d[1])
        return None
    return r.resize_device(n, sst[0], sst[1], sfst, s[0], s[1], s[2], dstr[0], dstr[1], dfst, d[0], d[1], d[2])


def _yuv_layout(case, which):
    """(frames, source plane offsets, (Y, chroma) source strides, source frame stride, the same for the destination).
    Source planes always lie tightly one after the other; so do the destination's, except where Y or chroma takes
    a huge row stride: the other planes then lie in the gaps between its rows."""
    entry, m, d, sw, sh, dw, dh, _, ky, kc = case
    cb = 2 if entry == "nv12" else 1
    sst = (sc.a16(sw), sc.a16(cb * (sw // 2)))
    ssz = [sh * sst[0]] + [(sh // 2) * sst[1]] * (3 - cb)
    sp = [sum(ssz[:i]) for i in range(len(ssz))]
    dstr = (sc.a16(dw), sc.a16(cb * (dw // 2)))
    dsz = [dh * dstr[0]] + [(dh // 2) * dstr[1]] * (3 - cb)
    dp = [sum(dsz[:i]) for i in range(len(dsz))]
    n, sfst, dfst = 2, sum(ssz), sum(dsz)
    if which == "far":
        n, sfst, dfst = 3, sc.FAR_SRC, sc.FAR_DST
    elif which == "y_top":
        smax, dmax, _, dst_max = LIMITS[ky]
        n, dstr = 1, (sc.top_stride(dh, dw, dmax, dst_max), dstr[1])
        dp = [0] + [2 ** 20 * (i + 1) for i in range(len(dp) - 1)]
    elif which == "chroma_over":
        smax, dmax, _, dst_max = LIMITS[kc]
        n, dstr = 1, (dstr[0], sc.top_stride(dh // 2, cb * (dw // 2), dmax, dst_max) + 16)
        dp = [0] + [2 ** 20 * (i + 1) for i in range(len(dp) - 1)]
    return n, sp, sst, sfst, dp, dstr, dfst


def _yuv_views(buf, case, n, offs, strides, fst, dst_side):
    entry, m, d, sw, sh, dw, dh = case[:7]
    w, h = (dw, dh) if dst_side else (sw, sh)
    out = [torch.as_strided(buf, (n, h, w), (fst, strides[0], 1), offs[0])]
    for o in offs[1:]:
        if entry == "nv12":
            out.append(torch.as_strided(buf, (n, h // 2, w // 2, 2), (fst, strides[1], 2, 1), o))
        else:
            out.append(torch.as_strided(buf, (n, h // 2, w // 2), (fst, strides[1], 1), o))
    return out


@YUV_CASES
@pytest.mark.parametrize("which", ["tight", "y_top", "far"])
def test_yuv_entries_accepted_layouts(case, which, bufs):
    src, dst = bufs
    r = _yuv_make(case)
    n, sp, sst, sfst, dp, dstr, dfst = _yuv_layout(case, which)
    assert (n - 1) * dfst + dp[-1] + (case[6] - 1) * max(dstr) + case[5] <= sc.BUF and (n - 1) * sfst + 2 ** 21 <= sc.BUF
    planes = _yuv_planes(case, n, which == "far")
    dst.fill_(A5)
    for v, (fr, _) in zip(_yuv_views(src, case, n, sp, sst, sfst, False), planes):
        v.copy_(torch.from_numpy(np.array(fr)).to(DEV))
    fused = _yuv_call(r, case, n, sp, sst, sfst, dp, dstr, dfst, src, dst)
    if case[0] == "i420":
        assert fused == (case[7] != "none")
    outs = _yuv_views(dst, case, n, dp, dstr, dfst, True)
    got = [o.cpu().numpy() for o in outs]
    for o in outs:
        o.fill_(A5)
    _untouched(dst)
    for k, (g, (_, exp)) in enumerate(zip(got, planes)):
        _same(g, exp, "%s %s plane %d" % (case[:7], which, k))


@pytest.mark.parametrize("case", [c for c in YUV if LIMITS[c[9]][0]], ids=lambda c: "%s-%s%d-%dx%d" % c[:5])
def test_yuv_entries_reject_a_chroma_layout_before_any_launch(case, bufs):
    """A chroma row stride one step past the largest its kernel accepts, with a valid Y layout: IQO_HIP_EINVAL (the
    fused I420 branch used to answer IQO_HIP_EHIP), and no plane written (the plane-by-plane branch and the NV12
    entry used to launch Y first)."""
    src, dst = bufs
    r = _yuv_make(case)
    n, sp, sst, sfst, dp, dstr, dfst = _yuv_layout(case, "chroma_over")
    assert dp[-1] + (case[6] // 2 - 1) * dstr[1] + 2 * case[5] <= sc.BUF
    for v, (fr, _) in zip(_yuv_views(src, case, n, sp, sst, sfst, False), _yuv_planes(case, n, False)):
        v.copy_(torch.from_numpy(np.array(fr)).to(DEV))
    dst.fill_(A5)
    with pytest.raises(libiqo_amd.IqoError) as e:
        _yuv_call(r, case, n, sp, sst, sfst, dp, dstr, dfst, src, dst)
    assert _einval(e), str(e.value)
    torch.cuda.synchronize()
    _untouched(dst)
