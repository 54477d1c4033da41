"""Fused I420 launches on the GPU: every instantiation launch_yuv420_lanczos / _area / _linear can pick
(tests/yuv_cases.py, one label each from libiqo_amd.host_yuv420_fused) against the CPU oracle per
plane, bit for bit (Lanczos chroma at pxScale 2, as iqo_hip_plan_yuv420 builds it), at small shapes:
layouts with padded strides, gaps, guard rows and misaligned planes, frame counts around the
stand-alone streamer's grid change, the frame chunking loop, a side stream, the tuning options,
host pointers, NV12 agreement and the error returns.

Inputs (yuv_cases.planes_for): a noise frame, a noise frame with flat bands, and a frame whose Y, U and
V planes are the constants 16, 128 and 235.  The reference itself does not keep a constant exactly
on the border rows and columns of pxScale-2 chroma (128 comes out as 125 there), so besides the
oracle equality each plane of that frame is only required to stay nearer its own constant than
either of the others (they are 107 apart or more): a U/V or Y/chroma mix-up fails both checks.
"""
import ctypes

import numpy as np
import pytest

import oracle_lib as ol
import yuv_cases as yc

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
SENT = 0xA5        # destination fill: every byte outside the payloads must keep it
SRC_FILL = 0x3C    # source bytes outside the payloads (never read into a result)
LEAD = 256         # bytes before the first frame and after the last one
ONE = yc.one_per_label()
BY_LABEL = {c[6]: c for c in ONE}


def _make(case):
    m, d, sw, sh, dw, dh, _ = case
    return libiqo_amd.Yuv420Resizer(m, d, sw, sh, dw, dh)


def _dims(case):
    _, _, sw, sh, dw, dh, _ = case
    return (sw, sh, sw // 2, sh // 2), (dw, dh, dw // 2, dh // 2)


def _check_frames(case, got, exp, what=""):
    """got / exp: (Y, U, V) arrays [n, h, w]."""
    for p, name in enumerate("YUV"):
        assert got[p].shape == exp[p].shape, (yc.cid(case), name, what)
        bad = np.argwhere(got[p] != exp[p])
        assert bad.size == 0, "%s %s plane %s: %d bytes differ, first at (frame, row, col) %s: got %d want %d" % (
            yc.cid(case), what, name, len(bad), tuple(bad[0]), got[p][tuple(bad[0])], exp[p][tuple(bad[0])])


def _check_constants(case, got):
    """Frame 2 of planes_for: each plane nearer its own constant than the other two."""
    for p, name in enumerate("YUV"):
        far = np.abs(got[p][2].astype(np.int32) - yc.CONST[p]).max()
        assert far < 53, "%s: constant plane %s is off by %d" % (yc.cid(case), name, far)


def _split_tight(case, out, n):
    """[n, dh*dw*3/2] tight I420 -> (Y, U, V)."""
    _, (dw, dh, cdw, cdh) = _dims(case)
    a, b = dw * dh, dw * dh + cdw * cdh
    return (out[:, :a].reshape(n, dh, dw), out[:, a:b].reshape(n, cdh, cdw), out[:, b:].reshape(n, cdh, cdw))


def _tight(y, u, v):
    n = y.shape[0]
    return np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1)


# ---- 1. every row of the table

@pytest.mark.parametrize("case", yc.CASES, ids=yc.cid)
def test_every_row_matches_oracle(case):
    y, u, v = yc.planes_for(case)
    src = torch.from_numpy(_tight(y, u, v)).to(DEV)
    out, fused = _make(case).resize_frames(src)
    got = _split_tight(case, out.cpu().numpy(), yc.N_FRAMES)
    assert fused == (case[6] != "none"), yc.cid(case)
    _check_frames(case, got, yc.expected_for(case))
    _check_constants(case, got)


# ---- 2. layouts: the three planes at chosen offsets of one sentinel-filled buffer

class Geom:
    """Byte layout of n I420 frames in one flat buffer: plane p of frame f starts at
    LEAD + f * frame + off[p], rows st[p] bytes apart.  Planes follow each other in `order`, `gap` bytes
    apart (then rounded up to 64), each shifted by shift[p]; `guard` Y rows follow each frame."""

    def __init__(self, dims, n, pad=(0, 0), gap=0, guard=0, order=(0, 1, 2), shift=(0, 0, 0)):
        w, h, wc, hc = dims
        self.n = n
        self.w, self.h = (w, wc, wc), (h, hc, hc)
        self.st = (w + pad[0], wc + pad[1], wc + pad[1])
        self.off = [0, 0, 0]
        pos = 0
        for p in order:
            self.off[p] = pos + shift[p]
            pos = self.off[p] + self.st[p] * self.h[p] + gap
            if gap:
                pos = (pos + 63) & ~63
        pos += guard * self.st[0]
        self.frame = (pos + 63) & ~63 if gap or guard else pos
        self.total = 2 * LEAD + n * self.frame

    def view(self, buf, p):
        """[n, h, w] view of plane p's payload in the flat uint8 / bool array buf."""
        return np.lib.stride_tricks.as_strided(buf[LEAD + self.off[p]:], shape=(self.n, self.h[p], self.w[p]),
                                               strides=(self.frame, self.st[p], 1))

    def outside(self, buf):
        mask = np.ones(self.total, dtype=bool)
        for p in range(3):
            self.view(mask, p)[...] = False
        return buf[mask]

    def ptr(self, base, p):
        return base + LEAD + self.off[p]


def _run_layout(r, case, planes, sg, dg, stream=None, n_call=None):
    """Lay the source planes out by sg, resize into a sentinel-filled buffer laid out by dg; returns the
    (Y, U, V) payloads and the fused flag, having checked every byte outside the payloads."""
    sbuf = np.full(sg.total, SRC_FILL, np.uint8)
    for p in range(3):
        sg.view(sbuf, p)[...] = planes[p]
    src = torch.from_numpy(sbuf).to(DEV)
    dst = torch.full((dg.total,), SENT, dtype=torch.uint8, device=DEV)
    assert src.data_ptr() % 256 == 0 and dst.data_ptr() % 256 == 0
    sb, db = src.data_ptr(), dst.data_ptr()
    fused = r.resize_device(sg.n if n_call is None else n_call, sg.st[0], sg.st[1], sg.frame, sg.ptr(sb, 0),
                            sg.ptr(sb, 1), sg.ptr(sb, 2), dg.st[0], dg.st[1], dg.frame, dg.ptr(db, 0), dg.ptr(db, 1),
                            dg.ptr(db, 2), stream)
    if stream is not None:
        stream.synchronize()
    dbuf = dst.cpu().numpy()
    out = dg.outside(dbuf)
    assert (out == SENT).all(), "%s: %d bytes outside the three payloads were written" % (
        yc.cid(case), int((out != SENT).sum()))
    return tuple(dg.view(dbuf, p).copy() for p in range(3)), fused


# name -> (Geom keyword arguments of the source, of the destination, fused as the label says)
LAYOUTS = {
    "tight": ({}, {}, True),
    "padded": (dict(pad=(32, 16), gap=64, guard=3), dict(pad=(32, 16), gap=64, guard=3), True),
    "v_before_u": (dict(order=(0, 2, 1)), dict(order=(0, 2, 1)), True),
    "u_plus_1": (dict(gap=64, shift=(0, 1, 0)), dict(gap=64, shift=(0, 1, 0)), False),
    "y_plus_1": (dict(gap=64, shift=(1, 0, 0)), dict(gap=64, shift=(1, 0, 0)), False),
    "dst_u_plus_1": (dict(gap=64), dict(gap=64, shift=(0, 1, 0)), False),
}


@pytest.mark.parametrize("layout", list(LAYOUTS))
@pytest.mark.parametrize("case", ONE, ids=yc.cid)
def test_layout_sweep(case, layout):
    skw, dkw, can_fuse = LAYOUTS[layout]
    sd, dd = _dims(case)
    n = yc.N_FRAMES
    got, fused = _run_layout(_make(case), case, yc.planes_for(case), Geom(sd, n, **skw), Geom(dd, n, **dkw))
    assert fused == (can_fuse and case[6] != "none"), (yc.cid(case), layout)
    _check_frames(case, got, yc.expected_for(case), layout)
    _check_constants(case, got)


# ---- 3. frame counts, stacked widths, chunking

def _device_noise(case, n, seed):
    """n tight I420 frames of noise made on the device: (tensor [n, bytes], its host copy)."""
    (sw, sh, cw, ch), _ = _dims(case)
    g = torch.Generator(device=DEV)
    g.manual_seed(seed)
    src = torch.randint(0, 256, (n, sw * sh + 2 * cw * ch), dtype=torch.uint8, device=DEV, generator=g)
    return src


def _src_planes(case, src_f):
    """(Y, U, V) of one tight host frame."""
    (sw, sh, cw, ch), _ = _dims(case)
    a, b = sw * sh, sw * sh + cw * ch
    return src_f[:a].reshape(sh, sw), src_f[a:b].reshape(ch, cw), src_f[b:].reshape(ch, cw)


def _check_against_oracle(case, src, out, frames):
    n = out.shape[0]
    for f in frames:
        exp = yc.oracle_planes(case, *_src_planes(case, src[f].cpu().numpy()))
        got = _split_tight(case, out[f:f + 1].cpu().numpy(), 1)
        _check_frames(case, got, tuple(e[None] for e in exp), "frame %d of %d" % (f, n))


FRAME_ROWS = [BY_LABEL["lz_symb10"], BY_LABEL["area44"]]


@pytest.mark.parametrize("n", [1, 3, 16, 24])
@pytest.mark.parametrize("case", FRAME_ROWS, ids=yc.cid)
def test_frame_counts(case, n):
    """Batches of 8 k >= 16 frames are where the stand-alone block-shared streamer takes a 1-D grid
    with an XCD tail split; the fused launch keeps its (band, frame, plane) grid."""
    m, d, sw, sh, dw, dh, _ = case
    (_, _, cw, ch), (_, _, cdw, cdh) = _dims(case)
    px = yc.chroma_shape(case)[4]
    src = _device_noise(case, n, 40 + n)
    out, fused = _make(case).resize_frames(src)
    assert fused
    torch.cuda.synchronize()
    _check_against_oracle(case, src, out, sorted({0, min(7, n - 1), min(8, n - 1), n - 1}))
    # every frame against the three single-plane resizers
    ry = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, 1)
    rc = libiqo_amd.make_resizer(m, d, cw, ch, cdw, cdh, px)
    a, b = sw * sh, sw * sh + cw * ch
    ey = ry.resize_tensor(src[:, :a].reshape(n, sh, sw))
    eu = rc.resize_tensor(src[:, a:b].reshape(n, ch, cw))
    ev = rc.resize_tensor(src[:, b:].reshape(n, ch, cw))
    got = _split_tight(case, out.cpu().numpy(), n)
    _check_frames(case, got, (ey.cpu().numpy(), eu.cpu().numpy(), ev.cpu().numpy()), "single-plane resizers")


@pytest.mark.parametrize("degree", [3, 2])
def test_stacked_width(degree):
    """320 -> 160 columns, 16 frames: the stand-alone plan stacks such frames side by side in one
    workgroup, the fused launch must not."""
    case = ("lanczos", degree, 320, 32, 160, 16, "lz_sym10" if degree == 3 else "lz_sym8")
    assert libiqo_amd.host_yuv420_fused(*case[:6]) == case[6]
    n = 16
    src = _device_noise(case, n, 77)
    out, fused = _make(case).resize_frames(src)
    assert fused
    _check_against_oracle(case, src, out, range(n))


@pytest.mark.parametrize("case", [BY_LABEL["lz_symb10"], BY_LABEL["lz_sym8"], BY_LABEL["area44"], BY_LABEL["lin_up2"]],
                         ids=yc.cid)
def test_chunk_frames_option(case):
    """chunk_frames = 5 on 13 frames: launches of 5, 5 and 3 frames."""
    n = 13
    r = _make(case)
    r.set_option("chunk_frames", 5)
    src = _device_noise(case, n, 78)
    out, fused = r.resize_frames(src)
    assert fused
    _check_against_oracle(case, src, out, range(n))


def test_chunking_above_the_grid_limit():
    """70000 frames in one call: two launches of 35000 (grid.y holds at most 65535)."""
    case = ("lanczos", 3, 64, 32, 32, 16, "lz_sym10")
    assert case in yc.CASES
    n = 70000
    src = _device_noise(case, n, 79)
    out, fused = _make(case).resize_frames(src)
    assert fused
    torch.cuda.synchronize()
    _check_against_oracle(case, src, out, (0, 34999, 35000, 69999))


# ---- 4. a side stream

@pytest.mark.parametrize("case", [BY_LABEL["lz_symb8"], BY_LABEL["area33"], BY_LABEL["lin_up2"]], ids=yc.cid)
def test_side_stream(case):
    """The launch goes to the caller's stream: the source is filled by work queued ahead on that stream."""
    r = _make(case)
    for pl in (0, 1):
        assert libiqo_amd.lib().iqo_hip_plan_prepare(libiqo_amd.lib().iqo_hip_yuv_plane(r._plan, pl)) == 0
    y, u, v = yc.planes_for(case)
    staged = torch.from_numpy(_tight(y, u, v)).to(DEV)
    src = torch.zeros_like(staged)
    filler = torch.empty(1 << 28, dtype=torch.uint8, device=DEV)
    torch.cuda.synchronize()
    stream = torch.cuda.Stream(device=DEV)
    assert stream.cuda_stream != torch.cuda.default_stream(DEV).cuda_stream
    with torch.cuda.stream(stream):
        for i in range(8):
            filler.fill_(i)
        src.copy_(staged)
        out, fused = r.resize_frames(src, stream=stream)
    stream.synchronize()
    assert fused
    got = _split_tight(case, out.cpu().numpy(), yc.N_FRAMES)
    _check_frames(case, got, yc.expected_for(case), "side stream")


# ---- 5. tuning options on either plane: whatever the call then runs, the output is the oracle's

OPTION_ROWS = [yc.CASES[0], yc.CASES[1], ("lanczos", 3, 1920, 64, 960, 32, "lz_sym10")]
OPTIONS = ([("prefetch", v) for v in (1, 2, 3, 4)] + [("stream_variant", v) for v in (0, 1, 2)] +
           [("lanes", v) for v in (0, 33, 47)] + [("bands", v) for v in (0, 1, 5)] + [("force_general", 1)])


@pytest.mark.parametrize("key,value", OPTIONS, ids=lambda o: str(o))
@pytest.mark.parametrize("case", OPTION_ROWS, ids=yc.cid)
def test_option_sweep(case, key, value):
    assert case in yc.CASES and case[6] in ("lz_symb10", "lz_symb8", "lz_sym10")
    src = torch.from_numpy(_tight(*yc.planes_for(case))).to(DEV)
    for plane in (0, 1, None):
        r = _make(case)
        r.set_option(key, value, plane=plane)
        out, fused = r.resize_frames(src)
        print("%s %s=%d plane %s: fused %d" % (yc.cid(case), key, value, plane, fused))
        got = _split_tight(case, out.cpu().numpy(), yc.N_FRAMES)
        _check_frames(case, got, yc.expected_for(case), "%s=%d on plane %s" % (key, value, plane))


# ---- 6. host pointers (the small-frame staged path: one upload, the fused launch, one download)

@pytest.mark.parametrize("pad", [0, 24], ids=["packed", "padded"])
@pytest.mark.parametrize("case", ONE, ids=yc.cid)
def test_host_pointers(case, pad):
    (sw, sh, cw, ch), (dw, dh, cdw, cdh) = _dims(case)
    y, u, v = yc.planes_for(case)
    ey, eu, ev = yc.expected_for(case)
    r = _make(case)
    for f in range(yc.N_FRAMES):
        def padded(a, w):
            b = np.full((a.shape[0], w + pad), SRC_FILL, np.uint8)
            b[:, :w] = a
            return b
        sy, su, sv = padded(y[f], sw), padded(u[f], cw), padded(v[f], cw)
        oy, ou, ov = (np.full((h, w + pad), SENT, np.uint8) for h, w in ((dh, dw), (cdh, cdw), (cdh, cdw)))
        r.resize(sw + pad, sy, cw + pad, su, sv, dw + pad, oy, cdw + pad, ou, ov)
        got = (oy[None, :, :dw], ou[None, :, :cdw], ov[None, :, :cdw])
        _check_frames(case, got, (ey[f:f + 1], eu[f:f + 1], ev[f:f + 1]), "host frame %d" % f)
        if pad:
            assert (oy[:, dw:] == SENT).all() and (ou[:, cdw:] == SENT).all() and (ov[:, cdw:] == SENT).all(), \
                "bytes past a row written"


# ---- 7. NV12 gives the same planes

@pytest.mark.parametrize("case", [BY_LABEL["lz_symb10"], BY_LABEL["area44"], BY_LABEL["lin_up2"]], ids=yc.cid)
def test_nv12_agrees(case):
    m, d, sw, sh, dw, dh, _ = case
    (_, _, cw, ch), (_, _, cdw, cdh) = _dims(case)
    n = yc.N_FRAMES
    y, u, v = yc.planes_for(case)
    out, fused = _make(case).resize_frames(torch.from_numpy(_tight(y, u, v)).to(DEV))
    assert fused
    gy, gu, gv = _split_tight(case, out.cpu().numpy(), n)
    uv = np.stack([u, v], axis=3)  # [n, ch, cw, 2]
    nv = torch.from_numpy(np.concatenate([y.reshape(n, -1), uv.reshape(n, -1)], axis=1)).to(DEV)
    o = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh).resize_frames(nv).cpu().numpy()
    ny = o[:, :dw * dh].reshape(n, dh, dw)
    nuv = o[:, dw * dh:].reshape(n, cdh, cdw, 2)
    _check_frames(case, (ny, nuv[..., 0], nuv[..., 1]), (gy, gu, gv), "NV12 against I420")


# ---- 8. errors

def _error_call(case, **change):
    """One 2-frame call on sentinel-filled buffers with one argument changed; returns (status, dst)."""
    (sw, sh, cw, ch), (dw, dh, cdw, cdh) = _dims(case)
    n = 2
    sg, dg = Geom((sw, sh, cw, ch), n, gap=64), Geom((dw, dh, cdw, cdh), n, gap=64)
    src = torch.full((sg.total,), SRC_FILL, dtype=torch.uint8, device=DEV)
    dst = torch.full((dg.total,), SENT, dtype=torch.uint8, device=DEV)
    sb, db = src.data_ptr(), dst.data_ptr()
    a = dict(n=n, srcStY=sg.st[0], srcStUV=sg.st[1], srcY=sg.ptr(sb, 0), srcU=sg.ptr(sb, 1), srcV=sg.ptr(sb, 2),
             dstStY=dg.st[0], dstStUV=dg.st[1], dstY=dg.ptr(db, 0), dstU=dg.ptr(db, 1), dstV=dg.ptr(db, 2))
    a.update(change)
    r = _make(case)
    fused = ctypes.c_int(-1)
    rc = libiqo_amd.lib().iqo_hip_resize_yuv420_device(
        r._plan, a["n"], a["srcStY"], a["srcStUV"], sg.frame, a["srcY"], a["srcU"], a["srcV"], a["dstStY"],
        a["dstStUV"], dg.frame, a["dstY"], a["dstU"], a["dstV"], None, ctypes.byref(fused))
    torch.cuda.synchronize()
    return rc, fused.value, dst.cpu().numpy()


ERROR_ROWS = [BY_LABEL["lz_sym8"], BY_LABEL["area22"], BY_LABEL["lin_up2"]]


@pytest.mark.parametrize("case", ERROR_ROWS, ids=yc.cid)
def test_errors(case):
    (sw, sh, cw, ch), (dw, dh, cdw, cdh) = _dims(case)
    EINVAL = -1
    bad = [dict(srcStY=sw - 1), dict(srcStUV=cw - 1), dict(dstStY=dw - 1), dict(dstStUV=cdw - 1)]
    bad += [{k: None} for k in ("srcY", "srcU", "srcV", "dstY", "dstU", "dstV")]
    for change in bad:
        rc, fused, dst = _error_call(case, **change)
        assert rc == EINVAL and fused == 0, (yc.cid(case), change, rc)
        assert (dst == SENT).all(), (yc.cid(case), change, "wrote despite the error")
    # no frames: OK, nothing written
    rc, fused, dst = _error_call(case, n=0)
    assert rc == 0 and fused == 0 and (dst == SENT).all()
    # the unchanged call works (the helper itself is sound)
    rc, fused, dst = _error_call(case)
    assert rc == 0 and fused == 1 and not (dst == SENT).all()
    with pytest.raises(libiqo_amd.IqoError, match="invalid argument"):
        _make(case).resize_device(2, sw - 1, cw, sw * sh * 2, 16, 16, 16, dw, cdw, dw * dh * 2, 16, 16, 16)


@pytest.mark.parametrize("dims", [(1, 32, 16, 16), (64, 1, 32, 16), (64, 32, 1, 16), (64, 32, 32, 1)])
@pytest.mark.parametrize("method", ["lanczos", "area", "linear"])
def test_plan_with_a_dimension_below_2_is_an_error(method, dims):
    with pytest.raises(libiqo_amd.IqoError, match="invalid argument"):
        libiqo_amd.Yuv420Resizer(method, 3, *dims)
    p = ctypes.c_void_p()
    rc = libiqo_amd.lib().iqo_hip_plan_yuv420(libiqo_amd._METHODS[method], 3, *dims, 0, ctypes.byref(p))
    assert rc == -1 and not p.value
    assert libiqo_amd.lib().iqo_hip_resize_yuv420_device(None, 1, 64, 32, 3072, 16, 16, 16, 32, 16, 768, 16, 16, 16, None,
                                                         None) == -1
