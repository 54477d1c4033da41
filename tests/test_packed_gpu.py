"""GPU parity of the packed (interleaved RGB / RGBA / UV / NV12) resize: channel c of every result
equals the oracle (the reference's Generic resize, restated) run on channel c as a plane, bit for
bit -- through packed_tile_kernel and packed_general_kernel, over shapes, layouts, bands, host
pointers, NV12, the plan cache and the error paths; every packed_tile_kernel<C, NP, LZ> instantiation
and every tile shape (packed_cases.INSTANTIATIONS / GEOMETRY, sections 11 - 13).  Small shapes, 2
frames (3 with the constant-channel frame): well under a second each."""
import gc
import os
import random

import numpy as np
import pytest

import oracle_lib as ol
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


def _make(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    return libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)


def _check(got, exp, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, (what, bad[:4].tolist())


# ---- 1. parity across channels and shapes

@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.sid)
def test_packed_shapes_match_oracle(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    frames = pc.frames_for(shape, C)
    exp = pc.expected_for(shape, C)
    src = torch.from_numpy(frames).to(DEV)
    r = _make(shape, C)
    want = libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px)
    desc = r.describe()
    assert desc["kernel"] == want and desc["channels"] == C
    assert want == ("packed_general" if sw < 8 else "packed_tile")
    out = r.resize_tensor(src)
    assert tuple(out.shape) == (2, dh, dw, C)
    _check(out.cpu().numpy(), exp, (shape, C, want))
    single = r.resize_tensor(src[1])  # [H, W, C]
    assert tuple(single.shape) == (dh, dw, C) and torch.equal(single, out[1])
    r.set_option("force_general", 1)
    assert r.describe()["kernel"] == "packed_general"
    gen = r.resize_tensor(src)
    assert torch.equal(gen, out), (shape, C, "packed_general differs from packed_tile")


@pytest.mark.parametrize("C", CHANNELS)
def test_taps_beyond_the_tile_tables_run_packed_general(C):
    shape = pc.GENERAL_SHAPE  # Lanczos-8 at 2:1
    r = _make(shape, C)
    assert r.describe()["kernel"] == "packed_general"
    out = r.resize_tensor(torch.from_numpy(pc.frames_for(shape, C)).to(DEV)).cpu().numpy()
    _check(out, pc.expected_for(shape, C), (shape, C))


# ---- 2. more than one tile in each axis
#
# Tiles of packed plans with C = 3, 4 at these ratios: CT = 64 output pixels x TH = 16 output rows
# (plan.cpp build_packed_tables; tests/test_packed_host.py checks these two shapes' geometry on the
# host, and describe()["tile_rows"] reports TH).  dstW >= 2 * 64 + 3, dstH >= 2 * 16 + 1, and
# srcW * C is no multiple of 8 (213 * 3, 213 * 4, 301 * 3, 301 * 4).
MULTI_TILE = [("lanczos", 3, 213, 100, 140, 70, 1), ("area", 0, 301, 90, 150, 41, 1)]


@pytest.mark.parametrize("C", [3, 4])
@pytest.mark.parametrize("shape", MULTI_TILE, ids=pc.sid)
def test_packed_several_tiles_each_axis(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    assert dw >= 2 * 64 + 3 and dh >= 2 * 16 + 1 and dh < 80 and (sw * C) % 8 != 0
    r = _make(shape, C)
    desc = r.describe()
    assert desc["kernel"] == "packed_tile" and desc["tile_rows"] == 16
    frames = pc.frames_for(shape, C)
    out = r.resize_tensor(torch.from_numpy(frames).to(DEV)).cpu().numpy()
    _check(out, pc.expected_for(shape, C), (shape, C))


# ---- 3. layouts: misaligned source base, padded strides, guard bytes

@pytest.mark.parametrize("C", CHANNELS)
@pytest.mark.parametrize("shape", [pc.SHAPES[0], pc.SHAPES[9]], ids=pc.sid)
def test_packed_misaligned_padded_layout(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    frames = pc.frames_for(shape, C)
    exp = pc.expected_for(shape, C)
    n = frames.shape[0]
    sst, dst_st = sw * C + 3, dw * C + 5
    sfst, dfst = sh * sst, dh * dst_st
    sbuf = torch.zeros(1 + n * sfst + 64, dtype=torch.uint8, device=DEV)
    sview = sbuf[1:1 + n * sfst].view(n, sh, sst)  # base misaligned by 1 byte
    sview[:, :, :sw * C] = torch.from_numpy(frames.reshape(n, sh, sw * C)).to(DEV)
    dbuf = torch.full((64 + n * dfst + 64,), SENTINEL, dtype=torch.uint8, device=DEV)
    r = _make(shape, C)
    assert r.describe()["kernel"] == "packed_tile"
    for force in (0, 1):
        dbuf.fill_(SENTINEL)
        r.set_option("force_general", force)
        r.resize_device(n, sst, sfst, sview.data_ptr(), dst_st, dfst, dbuf.data_ptr() + 64)
        torch.cuda.synchronize()
        full = dbuf.cpu().numpy()
        body = full[64:64 + n * dfst].reshape(n, dh, dst_st)
        _check(body[:, :, :dw * C].reshape(n, dh, dw, C), exp, (shape, C, force))
        assert (body[:, :, dw * C:] == SENTINEL).all(), (shape, C, force, "wrote into the row padding")
        assert (full[:64] == SENTINEL).all() and (full[64 + n * dfst:] == SENTINEL).all(), (shape, C, force,
                                                                                           "wrote into the guards")


# ---- 4. bands

@pytest.mark.parametrize("shape", [pc.SHAPES[7], pc.SHAPES[2]], ids=pc.sid)  # one downscale, one upscale
def test_packed_row_bands_are_byte_identical(shape):
    C = 3
    m, d, sw, sh, dw, dh, px = shape
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    r = _make(shape, C)
    full = r.resize_tensor(src)
    _check(full.cpu().numpy(), pc.expected_for(shape, C), (shape, "unsharded"))
    cuts = [0, dh // 5 + 1, (2 * dh) // 3, dh]  # 3 uneven bands
    parts = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        s0, sn = r.band_src_rows(r0, r1 - r0)
        window = src[:, s0:s0 + sn].contiguous()
        band = torch.empty((2, r1 - r0, dw, C), dtype=torch.uint8, device=DEV)
        r.resize_band(2, r0, r1 - r0, s0, sw * C, sn * sw * C, window, dw * C, (r1 - r0) * dw * C, band,
                      torch.cuda.current_stream())
        parts.append(band)
    torch.cuda.synchronize()
    assert torch.equal(torch.cat(parts, dim=1), full)


def test_packed_band_window_must_cover_the_halo():
    shape, C = pc.SHAPES[7], 3
    m, d, sw, sh, dw, dh, px = shape
    r = _make(shape, C)
    r0, rows = dh // 2, 10
    s0, sn = r.band_src_rows(r0, rows)
    assert s0 > 0
    window = torch.zeros((1, sn, sw, C), dtype=torch.uint8, device=DEV)
    band = torch.empty((1, rows, dw, C), dtype=torch.uint8, device=DEV)
    with pytest.raises(libiqo_amd.IqoError):  # starts one row below the halo
        r.resize_band(1, r0, rows, s0 + 1, sw * C, sn * sw * C, window, dw * C, rows * dw * C, band)
    r.resize_band(1, r0, rows, s0, sw * C, sn * sw * C, window, dw * C, rows * dw * C, band)
    torch.cuda.synchronize()


# ---- 5. host pointers

@pytest.mark.parametrize("shape", [pc.SHAPES[0], pc.SHAPES[11]], ids=pc.sid)
def test_packed_host_pointers_padded_stride(shape):
    C = 4
    m, d, sw, sh, dw, dh, px = shape
    frame = pc.frames_for(shape, C)[0]
    exp = pc.expected_for(shape, C)[0]
    r = _make(shape, C)
    sst, dst_st = sw * C + 7, dw * C + 9
    src = np.zeros((sh, sst), np.uint8)
    src[:, :sw * C] = frame.reshape(sh, sw * C)
    out = np.full((dh, dst_st), 7, np.uint8)
    r.resize(sst, src, dst_st, out)
    _check(out[:, :dw * C].reshape(dh, dw, C), exp, shape)
    assert (out[:, dw * C:] == 7).all(), "bytes past the row written"
    with pytest.raises(libiqo_amd.IqoError):
        r.resize(sw * C - 1, src, dst_st, out)


# ---- 6. NV12

@pytest.mark.parametrize("case", [("lanczos", 3, 64, 48, 32, 24), ("area", 0, 60, 44, 40, 30)],
                         ids=lambda c: "%s%d_%dx%d" % c[:4])
def test_nv12_planes_match_oracle(case):
    m, d, sw, sh, dw, dh = case
    n = 2
    cw, ch, cdw, cdh = sw // 2, sh // 2, dw // 2, dh // 2
    y = np.stack([ol.gen("noise", sw, sh, 900 + f)[:, :sw] for f in range(n)])
    uv = np.stack([pc.packed_noise(cw, ch, 2, 910 + f) for f in range(n)])
    uv[1, : ch // 2, :, 1] = 255
    src = torch.from_numpy(np.concatenate([y.reshape(n, -1), uv.reshape(n, -1)], axis=1)).to(DEV)
    r = libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
    ky, kuv = r.describe()
    assert ky == libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, 1) and kuv == "packed_tile"
    out = r.resize_frames(src).cpu().numpy()
    assert out.shape == (n, dw * dh + 2 * cdw * cdh)
    pxc = 2 if m == "lanczos" else 1
    for f in range(n):
        oy = out[f, : dw * dh].reshape(dh, dw)
        ouv = out[f, dw * dh:].reshape(cdh, cdw, 2)
        assert (oy == ol.run_oracle(m, d, sw, sh, dw, dh, 1, y[f])).all(), (case, f, "Y")
        for c, name in ((0, "U"), (1, "V")):
            e = ol.run_oracle(m, d, cw, ch, cdw, cdh, pxc, np.ascontiguousarray(uv[f, :, :, c]))
            assert (ouv[:, :, c] == e).all(), (case, f, name)


# ---- 7. plan cache: a destroyed packed plan never comes back for a planar request, nor the reverse

@pytest.mark.parametrize("first", [4, 1], ids=["packed_then_planar", "planar_then_packed"])
def test_plan_cache_keeps_channels_apart(first):
    shape = ("lanczos", 3, 72, 40, 48, 27, 1)  # (no other test uses this shape: the cache is per process)
    m, d, sw, sh, dw, dh, px = shape
    for C in (first, 5 - first):
        r = _make(shape, C)
        desc = r.describe()
        assert desc["channels"] == C
        if C == 1:
            assert desc["kernel"] == libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, px)
            assert not desc["kernel"].startswith("packed")
            frame = ol.gen("noise", sw, sh, 3)[:, :sw]
            out = r.resize_tensor(torch.from_numpy(frame).to(DEV)).cpu().numpy()
            _check(out, ol.run_oracle(m, d, sw, sh, dw, dh, px, frame), (shape, C))
        else:
            assert desc["kernel"] == "packed_tile"
            frames = pc.frames_for(shape, C)
            out = r.resize_tensor(torch.from_numpy(frames).to(DEV)).cpu().numpy()
            _check(out, pc.expected_for(shape, C), (shape, C))
        del r
        gc.collect()  # iqo_hip_plan_destroy: the plan goes to the cache


# ---- 8. channels = 1 through the packed constructor is the planar plan

@pytest.mark.parametrize("shape", [pc.SHAPES[0], ("lanczos", 3, 384, 216, 192, 108, 1), pc.SHAPES[9], pc.SHAPES[11]],
                         ids=pc.sid)
def test_one_channel_packed_plan_is_the_planar_plan(shape):
    import ctypes
    m, d, sw, sh, dw, dh, px = shape
    planar = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px)
    one = libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px)
    L = libiqo_amd.lib()
    L.iqo_hip_plan_destroy(one._plan)  # swap the handle for one made by iqo_hip_plan_packed(channels = 1)
    one._plan = ctypes.c_void_p()
    rc = L.iqo_hip_plan_packed(ol.METHODS[m], d, 1, sw, sh, dw, dh, px, 0, ctypes.byref(one._plan))
    assert rc == 0
    assert one.describe() == planar.describe() and one.describe()["channels"] == 1
    src = torch.from_numpy(np.stack([ol.gen("noise", sw, sh, 5 + f)[:, :sw] for f in range(2)])).to(DEV)
    a, b = planar.resize_tensor(src), one.resize_tensor(src)
    assert torch.equal(a, b)
    _check(a[0].cpu().numpy(), ol.run_oracle(m, d, sw, sh, dw, dh, px, src[0].cpu().numpy()), shape)


# ---- 9. errors

def test_packed_errors():
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.make_resizer("lanczos", 3, 40, 24, 27, 17, channels=0)
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.make_resizer("area", 0, 40, 24, 27, 17, channels=5)
    C, (sw, sh, dw, dh) = 3, (40, 24, 27, 17)
    r = libiqo_amd.make_resizer("lanczos", 3, sw, sh, dw, dh, channels=C)
    src = torch.zeros((1, sh, sw, C), dtype=torch.uint8, device=DEV)
    dst = torch.zeros((1, dh, dw, C), dtype=torch.uint8, device=DEV)
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_device(1, sw * C - 1, sh * sw * C, src, dw * C, dh * dw * C, dst)
    with pytest.raises(libiqo_amd.IqoError):
        r.resize_device(1, sw * C, sh * sw * C, src, dw * C - 1, dh * dw * C, dst)
    with pytest.raises(libiqo_amd.IqoError):  # a planar tensor for a packed plan
        r.resize_tensor(torch.zeros((1, sh, sw), dtype=torch.uint8, device=DEV))
    r.resize_device(1, sw * C, sh * sw * C, src, dw * C, dh * dw * C, dst)
    torch.cuda.synchronize()


# ---- 10. seeded fuzz

def _fuzz_cases():
    """24 seeded shapes, sides 4..96, all three methods, C per case.  Linear upscales beyond 2x (the
    reference reads outside its rows there: no pinned answer) and Lanczos shapes the plan rejects
    (ol.lanczos_rows_defined: the reference writes rows >= dstH) are left out while generating."""
    rng = random.Random(1409)
    out = []
    while len(out) < 24:
        m = ("lanczos", "area", "linear")[len(out) % 3]
        d = rng.randint(1, 5) if m == "lanczos" else 0
        sw, sh, dw, dh = (rng.randint(4, 96) for _ in range(4))
        if m == "linear" and (dw > 2 * sw or dh > 2 * sh):
            continue
        if m == "lanczos" and not ol.lanczos_rows_defined(d, sh, dh, 1):
            continue
        out.append((m, d, sw, sh, dw, dh, 1, rng.choice(CHANNELS)))
    return out


@pytest.mark.parametrize("case", _fuzz_cases(), ids=lambda c: "%s%d_%dx%d_%dx%d_px%d_c%d" % c)
def test_packed_random_shapes_match_oracle(case):
    shape, C = case[:7], case[7]
    frames = pc.frames_for(shape, C)
    exp = np.stack([pc.oracle_packed(shape, f) for f in frames])
    r = _make(shape, C)
    out = r.resize_tensor(torch.from_numpy(frames).to(DEV)).cpu().numpy()
    _check(out, exp, (case, r.describe()["kernel"]))


# ---- 11. every packed_tile_kernel<C, NP, LZ> instantiation and every tile shape
#
# packed_cases.INSTANTIATIONS has one row per (C, NP, LZ), GEOMETRY the tile shapes (every CT and
# TH with two tiles or more and a partial last one); tests/test_packed_host.py proves both censuses
# and the rows' literals on the host.  Each row: frames_for's two frames plus a frame whose channels
# are the constants (0, 255, 1, 254)[:C]; byte for byte against the oracle, no tolerance.

def _cell(row):
    shape, C, CT, TH, NP = row
    return "C=%d NP=%d LZ=%s CT=%d TH=%d %s" % (C, NP, shape[0] == "lanczos", CT, TH, pc.sid(shape))


def _check_cell(got, exp, row, what):
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %s differs at %d bytes, first [frame, y, x, c] %s" % (_cell(row), what, len(bad),
                                                                                    bad[:4].tolist())


def _cell_io(row):
    """Frames [3, sh, sw, C] (frames_for's two and the constant one) and their oracle results."""
    shape, C = row[0], row[1]
    const = pc.const_frame(shape, C)
    frames = np.concatenate([pc.frames_for(shape, C), const[None]])
    exp = np.concatenate([pc.expected_for(shape, C), pc.oracle_packed(shape, const)[None]])
    return frames, exp


def _run_cell(row, constants_kept=True):
    shape, C, CT, TH, NP = row
    frames, exp = _cell_io(row)
    r = _make(shape, C)
    desc = r.describe()
    assert desc["kernel"] == "packed_tile" and desc["tile_rows"] == TH and desc["channels"] == C, (_cell(row), desc)
    src = torch.from_numpy(frames).to(DEV)
    out = r.resize_tensor(src)
    got = out.cpu().numpy()
    _check_cell(got, exp, row, "packed_tile vs the oracle")
    if constants_kept:  # a wrong byte selector shows as cross-talk between the channels
        want = np.broadcast_to(np.array(pc.CONST_CHANNELS[:C], np.uint8), got[2].shape)
        _check_cell(got[2:], want[None], row, "constant channels")
    r.set_option("force_general", 1)
    assert r.describe()["kernel"] == "packed_general"
    gen = r.resize_tensor(src)
    _check_cell(gen.cpu().numpy(), got, row, "packed_general vs packed_tile")


@pytest.mark.parametrize("row", pc.INSTANTIATIONS, ids=pc.cell_id)
def test_packed_every_instantiation(row):
    _run_cell(row)


@pytest.mark.parametrize("row", pc.GEOMETRY, ids=pc.cell_id)
def test_packed_tile_geometries(row):
    _run_cell(row)


@pytest.mark.parametrize("row", pc.LANCZOS_WIDE_UPSCALES, ids=pc.cell_id)
def test_packed_wide_lanczos_upscales(row):
    """CT = 512 at C = 2 and CT = 256 at C = 4 under Lanczos: upscales above 2x, where the reference
    itself does not keep the constant frame (packed_cases.LANCZOS_WIDE_UPSCALES), so that frame is
    compared with the oracle like the others."""
    _run_cell(row, constants_kept=False)


# ---- 12. layouts over the matrix: wide stores with a guarded row end, byte-shifted sources,
#          byte-shifted destinations

LAYOUT_ROWS = [pc.GEOMETRY[0], pc.GEOMETRY[1], pc.GEOMETRY[4], pc.GEOMETRY[5], pc.GEOMETRY[10], pc.GEOMETRY[11],
               pc.GEOMETRY[12], pc.LANCZOS_WIDE_UPSCALES[1], pc.INSTANTIATIONS[31], pc.INSTANTIATIONS[63]]


def test_layout_rows_cover_the_kernel_paths():
    assert len(LAYOUT_ROWS) >= 8
    assert {r[1] for r in LAYOUT_ROWS} == {2, 3, 4}
    assert {r[0][0] == "lanczos" for r in LAYOUT_ROWS} == {True, False}
    assert any(r[2] >= 256 for r in LAYOUT_ROWS) and any(r[3] == 2 for r in LAYOUT_ROWS)
    assert all(r[0][4] % 4 for r in LAYOUT_ROWS)  # the last quad of a row is partial: single-byte stores


def _up4(v):
    return (v + 3) & ~3


@pytest.mark.parametrize("row", LAYOUT_ROWS, ids=pc.cell_id)
def test_packed_layout_sweep(row):
    shape, C, CT, TH, NP = row
    m, d, sw, sh, dw, dh, px = shape
    n = 2
    frames, exp = pc.frames_for(shape, C), pc.expected_for(shape, C)
    r = _make(shape, C)
    assert r.describe()["kernel"] == "packed_tile"
    G = 64  # guard bytes before the base and after the last frame
    wide_st = _up4(dw * C + 8)  # a multiple of 4 with >= 8 bytes of padding: a store past the row's end lands in it
    # (name, source base offset, srcSt, destination base offset, dstSt)
    layouts = [("wide stores, guarded row end", 0, sw * C, 0, wide_st)]
    layouts += [("source shifted by %d" % k, k, _up4(sw * C) + 4, 0, wide_st) for k in (1, 2, 3)]
    layouts += [("destination shifted by %d" % k, 0, sw * C, k, wide_st) for k in (1, 2, 3)]
    for name, soff, sst, doff, dst_st in layouts:
        assert sst % 4 == 0 or soff == 0
        assert dst_st % 4 == 0 and dst_st >= dw * C + 8
        sfst, dfst = sh * sst, dh * dst_st
        sbuf = torch.zeros(soff + n * sfst + 64, dtype=torch.uint8, device=DEV)
        assert sbuf.data_ptr() % 4 == 0
        sview = sbuf[soff:soff + n * sfst].view(n, sh, sst)
        sview[:, :, :sw * C] = torch.from_numpy(frames.reshape(n, sh, sw * C)).to(DEV)
        dbuf = torch.full((G + doff + n * dfst + G,), SENTINEL, dtype=torch.uint8, device=DEV)
        assert dbuf.data_ptr() % 4 == 0
        r.resize_device(n, sst, sfst, sview.data_ptr(), dst_st, dfst, dbuf.data_ptr() + G + doff)
        torch.cuda.synchronize()
        full = dbuf.cpu().numpy()
        body = full[G + doff:G + doff + n * dfst].reshape(n, dh, dst_st)
        _check_cell(body[:, :, :dw * C].reshape(n, dh, dw, C), exp, row, name)
        pad = np.argwhere(body[:, :, dw * C:] != SENTINEL)
        assert pad.size == 0, "%s: %s wrote into the row padding at [frame, y, byte] %s" % (_cell(row), name,
                                                                                          pad[:4].tolist())
        assert (full[:G + doff] == SENTINEL).all(), "%s: %s wrote before the base" % (_cell(row), name)
        assert (full[G + doff + n * dfst:] == SENTINEL).all(), "%s: %s wrote past the last frame" % (_cell(row), name)


# ---- 13. bands at C = 2 and C = 4: one-row bands and band starts inside a tile

BAND_ROWS = [pc.GEOMETRY[13], pc.GEOMETRY[14], pc.GEOMETRY[8], pc.GEOMETRY[9]]  # C = 2, 4 down; C = 2, 4 up


def test_band_rows_cover_both_directions():
    assert sorted((r[1], r[0][2] > r[0][4]) for r in BAND_ROWS) == [(2, False), (2, True), (4, False), (4, True)]
    assert all(r[0][5] > r[3] for r in BAND_ROWS)  # two row tiles or more


@pytest.mark.parametrize("row", BAND_ROWS, ids=pc.cell_id)
def test_packed_uneven_row_bands(row):
    shape, C, CT, TH, NP = row
    m, d, sw, sh, dw, dh, px = shape
    src = torch.from_numpy(pc.frames_for(shape, C)).to(DEV)
    r = _make(shape, C)
    assert r.describe()["kernel"] == "packed_tile" and r.describe()["tile_rows"] == TH
    full = r.resize_tensor(src)
    _check_cell(full.cpu().numpy(), pc.expected_for(shape, C), row, "unsharded vs the oracle")
    cuts = [0, 1, TH - 1, TH + 1, dh // 2, dh - 2, dh]
    assert cuts == sorted(set(cuts)), cuts
    parts = []
    for r0, r1 in zip(cuts[:-1], cuts[1:]):
        s0, sn = r.band_src_rows(r0, r1 - r0)
        window = src[:, s0:s0 + sn].contiguous()
        band = torch.empty((2, r1 - r0, dw, C), dtype=torch.uint8, device=DEV)
        r.resize_band(2, r0, r1 - r0, s0, sw * C, sn * sw * C, window, dw * C, (r1 - r0) * dw * C, band,
                      torch.cuda.current_stream())
        parts.append(band)
    torch.cuda.synchronize()
    _check_cell(torch.cat(parts, dim=1).cpu().numpy(), full.cpu().numpy(), row, "bands %s vs unsharded" % cuts)


# ---- 14. NV12 upscale: the UV plane runs at C = 2 with pxScale 2, upscaling

def test_nv12_upscale_planes_match_oracle():
    test_nv12_planes_match_oracle(("lanczos", 3, 64, 48, 160, 120))


# ---- 15. Lanczos shapes whose top border rows exceed dstH are rejected before any launch

@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", pc.REJECTED, ids=pc.sid)
def test_rejected_lanczos_shapes_raise(shape, C):
    m, d, sw, sh, dw, dh, px = shape
    assert not ol.lanczos_rows_defined(d, sh, dh, px)
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.make_resizer(m, d, sw, sh, dw, dh, px, channels=C)
    if px == 1:
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.Nv12Resizer(m, d, sw, sh, dw, dh)
