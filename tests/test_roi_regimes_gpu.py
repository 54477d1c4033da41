"""GPU parity of the batched crop-and-resize in the regimes of tests/roi_regime_cases.py: remainder bands and every
rows-per-workgroup value down to 1 with the largest LDS, one to 4097 boxes (three rounds of the kernel's box search,
arenas regrown while the other one is in flight), extreme frames, all 12 roi_kernel<LZ, C, NORM> instantiations by
name, every source and destination misalignment, and a box offset beyond 4 GiB.  Every output is compared byte for
byte (bit for bit in the float form) with the CPU twin and with the oracle-derived expectation, which
tests/test_roi_regimes_host.py pins to each other without a GPU."""
import os

import numpy as np
import pytest

import norm_cases as nc
import roi_regime_cases as rr

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")
os.environ["IQO_REQUIRE_HIP"] = "1"
SENTINEL = 0xA5
TORCH_DTYPE = {"float32": torch.float32, "float16": torch.float16, "bfloat16": torch.bfloat16}


def _bits(t):
    t = t.contiguous()
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16).cpu().numpy()


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _resizer(case, C):
    return libiqo_amd.RoiResizer(case.method, case.degree, case.dw, case.dh, channels=C)


def _device_frames(case, C):
    """The case's frames on the device with the host array's strides (table B's C = 1 and C = 3 frames are views of
    one buffer, rows 16384 bytes apart)."""
    a = rr.frames(case.fid, C)
    if a.flags["C_CONTIGUOUS"]:
        return torch.from_numpy(a.copy()).to(DEV)
    base = a
    while base.base is not None:
        base = base.base
    flat = torch.from_numpy(np.array(base, copy=True).reshape(-1)).to(DEV)
    return flat.as_strided(a.shape, a.strides, a.__array_interface__["data"][0] - base.__array_interface__["data"][0])


def _padded(n, case, C):
    """(big, out): a sentinel-filled buffer and the [n, dh, dw(, C)] view of it a call writes."""
    tail = (C,) if C > 1 else ()
    big = torch.full((n, case.dh + 2, case.dw + 3) + tail, SENTINEL, dtype=torch.uint8, device=DEV)
    return big, big[:, :case.dh, :case.dw]


def _sentinels_survive(big, case):
    h = big.cpu().numpy()
    mask = np.ones(h.shape, bool)
    mask[:, :case.dh, :case.dw] = False
    assert (h[mask] == SENTINEL).all()


def _check(case, C, pad=False):
    exp = rr.expected(case, C)
    _same(rr.twin(case, C), exp, "twin vs oracle %s C=%d" % (rr.cid(case), C))
    src = _device_frames(case, C)
    r = _resizer(case, C)
    if pad:
        big, out = _padded(len(case.boxes), case, C)
        assert r.resize_rois(src, case.boxes, out=out) is out
        _same(out.cpu().numpy(), exp, "%s C=%d" % (rr.cid(case), C))
        _sentinels_survive(big, case)
    else:
        _same(r.resize_rois(src, case.boxes).cpu().numpy(), exp, "%s C=%d" % (rr.cid(case), C))


# ----------------------------------------------------------------------------- tables A-D

@pytest.mark.parametrize("C", rr.CHANNELS)
@pytest.mark.parametrize("case", rr.TABLE_A, ids=rr.cid)
def test_sizes_bands_degrees(case, C):
    _check(case, C)


@pytest.mark.parametrize("C", rr.CHANNELS)
@pytest.mark.parametrize("case", rr.TABLE_B, ids=rr.cid)
def test_wide_boxes(case, C):
    """rows per workgroup 8 .. 1 (tests/test_roi_regimes_host.py proves which), remainder bands under a band height
    below 8, and a narrow box at rows = 8 inside the wide box's LDS allocation."""
    _check(case, C, pad=True)


@pytest.mark.parametrize("method,degree", rr.WIDEST, ids=["lanczos3", "area"])
def test_widest_box(method, degree):
    """The launch with the largest dynamic LDS the library asks for."""
    case = rr.widest_case(method, degree)
    assert rr.layout(case, 4, case.boxes[0])["lds_bytes"] > libiqo_amd.ROI_LDS_BYTES - 32
    _check(case, 4, pad=True)


@pytest.mark.parametrize("case", rr.TABLE_C + [rr.C_AREA], ids=rr.cid)
def test_box_counts(case):
    """Each count on a fresh plan: 4097 boxes take three search rounds and an arena above the first allocation."""
    _check(case, 3 if case is rr.C_AREA else 1, pad=True)


@pytest.mark.parametrize("counts", [rr.C_QUEUE, rr.C_REGROW], ids=["queue", "regrow"])
def test_box_counts_queued_on_one_stream(counts):
    """One plan, one side stream, no synchronisation between the calls (roi_regime_cases.C_QUEUE / C_REGROW): arenas
    are allocated large, or freed and reallocated, while the launch on the other arena is in flight, then reused."""
    by = {len(c.boxes): c for c in rr.TABLE_C}
    cases = [by[n] for n in counts]
    src = _device_frames(cases[0], 1)
    r = _resizer(cases[0], 1)
    bufs = [_padded(len(c.boxes), c, 1) for c in cases]
    s = torch.cuda.Stream(DEV)
    torch.cuda.synchronize(DEV)
    for c, (_, out) in zip(cases, bufs):
        r.resize_rois(src, c.boxes, out=out, stream=s)
    s.synchronize()
    for i, (c, (big, out)) in enumerate(zip(cases, bufs)):
        _same(out.cpu().numpy(), rr.expected(c, 1), "call %d of %s" % (i, counts))
        _sentinels_survive(big, c)


@pytest.mark.parametrize("C", rr.CHANNELS)
@pytest.mark.parametrize("case", rr.TABLE_D + rr.TABLE_E, ids=rr.cid)
def test_extreme_frames(case, C):
    _check(case, C)


# ----------------------------------------------------------------------------- the 12 instantiations

INSTANCES = [(lz, C, norm) for lz in ("lanczos", "area") for C in rr.CHANNELS for norm in (False, True)]
ORDERS = {1: (0, 0, 0), 3: (2, 0, 1), 4: (3, 1, 0, 2)}


@pytest.mark.parametrize("lz,C,norm", INSTANCES, ids=["roi_kernel<%s,%d,%s>" % (l == "lanczos", c, n) for l, c, n in INSTANCES])
def test_every_instantiation(lz, C, norm):
    """roi_kernel<LZ, C, NORM> by name on table A's 33 x 21 case: an odd width with flipped boxes takes the mirrored
    store of both epilogues; the float form at fp32, fp16 and bf16 with a permuting order."""
    case = rr.A_INSTANCE[lz]
    assert case.dw % 2 == 1 and any(rr.flipped(b) for b in case.boxes) and not all(rr.flipped(b) for b in case.boxes)
    u8 = rr.expected(case, C)
    src = _device_frames(case, C)
    r = _resizer(case, C)
    if not norm:
        _same(rr.twin(case, C), u8, "twin vs oracle")
        _same(r.resize_rois(src, case.boxes).cpu().numpy(), u8, "bytes C=%d" % C)
        return
    order = ORDERS[C]
    scale, bias = nc.NORM_SCALE[:len(order)], nc.NORM_BIAS[:len(order)]
    for dtype in nc.DTYPES:
        bits = nc.expected_bits(u8[..., None] if C == 1 else u8, order, scale, bias, dtype)
        tw = rr.twin(case, C, scale=scale, bias=bias, dtype=dtype, order=order)
        _same(tw.view(bits.dtype), bits, "twin vs numpy %s" % dtype)
        got = r.resize_rois_normalized(src, case.boxes, scale, bias, dtype=TORCH_DTYPE[dtype], order=order)
        _same(_bits(got), bits, "%s C=%d %s" % (lz, C, dtype))


# ----------------------------------------------------------------------------- alignment

@pytest.mark.parametrize("off", (1, 2, 3))
@pytest.mark.parametrize("C", rr.CHANNELS)
@pytest.mark.parametrize("lz", ("lanczos", "area"))
def test_misaligned_source(lz, C, off):
    """The frames as a view at storage byte offset 1, 2, 3 of a larger buffer, rows a multiple of 4 bytes apart: with
    C = 4 every fetch is then misaligned (mis != 0)."""
    case = rr.A_INSTANCE[lz]
    a = rr.frames(case.fid, C)
    F, H, W = a.shape[:3]
    row = (W * C + 3 + 4) & ~3
    buf = torch.full((F * H * row + 8,), 0x3C, dtype=torch.uint8, device=DEV)
    shape, strides = ((F, H, W), (H * row, row, 1)) if C == 1 else ((F, H, W, C), (H * row, row, C, 1))
    src = buf.as_strided(shape, strides, off)
    src.copy_(torch.from_numpy(a.copy()))
    assert src.data_ptr() % 4 == off and src.stride(1) % 4 == 0
    big, out = _padded(len(case.boxes), case, C)
    _resizer(case, C).resize_rois(src, case.boxes, out=out)
    _same(out.cpu().numpy(), rr.expected(case, C), "source at +%d C=%d" % (off, C))
    _sentinels_survive(big, case)
    # the bytes around the view were not needed: the result does not depend on them, and they are what they were
    h = buf.cpu().numpy().copy()
    inside = np.zeros(h.shape, bool)
    np.lib.stride_tricks.as_strided(inside[off:], shape, strides)[...] = True
    assert (h[~inside] == 0x3C).all()


@pytest.mark.parametrize("lz", ("lanczos", "area"))
@pytest.mark.parametrize("how", ("offset1", "odd-rows"))
def test_misaligned_rgba_destination(lz, how):
    """C = 4 stores a pixel as one dword where it is 4-byte aligned and as 4 bytes where it is not.  A destination
    at storage offset 1 takes the byte form everywhere; rows dstW * 4 + 3 bytes apart take both within one launch,
    every alignment occurring."""
    case, C = rr.A_INSTANCE[lz], 4
    n, dh, dw = len(case.boxes), case.dh, case.dw
    row = dw * 4 + (0 if how == "offset1" else 3)
    per = dh * row + 8 + (-dh * row) % 4  # outputs a multiple of 4 bytes apart
    buf = torch.full((n * per + 16,), SENTINEL, dtype=torch.uint8, device=DEV)
    out = buf.as_strided((n, dh, dw, 4), (per, row, 4, 1), 1 if how == "offset1" else 0)
    al = {(out.data_ptr() + i * per + y * row) % 4 for i in range(n) for y in range(dh)}
    assert buf.data_ptr() % 4 == 0 and al == ({1} if how == "offset1" else {0, 1, 2, 3})
    _resizer(case, C).resize_rois(_device_frames(case, C), case.boxes, out=out)
    _same(out.cpu().numpy(), rr.expected(case, C), "destination %s" % how)
    h = buf.cpu().numpy().copy()
    inside = np.zeros(h.shape, bool)
    np.lib.stride_tricks.as_strided(inside[1 if how == "offset1" else 0:], (n, dh, dw, 4), (per, row, 4, 1))[...] = True
    assert (h[~inside] == SENTINEL).all()


# ----------------------------------------------------------------------------- offsets beyond 4 GiB

def test_box_offsets_beyond_4gib():
    """Two frames 2^32 + 4096 bytes apart: the records of frame 1's boxes carry a non-zero high offset word."""
    need = 2 ** 32 + 2 ** 22
    if torch.cuda.mem_get_info()[0] < 6 * 2 ** 30:
        pytest.skip("less than 6 GiB of free device memory")
    case = rr.A_INSTANCE["lanczos"]
    a = rr.frames(case.fid, 1)
    assert a.shape == (2, rr.A_H, rr.A_W)
    buf = torch.empty(need, dtype=torch.uint8, device=DEV)  # left unfilled
    src = buf.as_strided((2, rr.A_H, rr.A_W), (2 ** 32 + 4096, 160, 1))
    src.copy_(torch.from_numpy(a.copy()))
    boxes = [(1, 0, 0, 64, 48), (0, 1, 2, 64, 48), (1, 3, 5, 45, 31, 1), (1, 0, 0, 128, 96), (0, 5, 0, 123, 96, 1),
             (1, 120, 90, 8, 6)]
    assert all(rr.answerable(case.method, case.degree, b, case.dw, case.dh) for b in boxes)
    assert boxes[0][:3] == (1, 0, 0) and any(b[0] == 0 for b in boxes)
    exp = libiqo_amd.host_resize_rois(case.method, case.degree, case.dw, case.dh, a, boxes)  # on the compact copy
    _same(exp, rr.expected(case._replace(boxes=tuple(boxes)), 1), "twin vs oracle")
    big, out = _padded(len(boxes), case, 1)
    _resizer(case, 1).resize_rois(src, boxes, out=out)
    _same(out.cpu().numpy(), exp, "frames 2^32 + 4096 bytes apart")
    _sentinels_survive(big, case)
    del src, buf
    torch.cuda.empty_cache()
