"""GPU parity of the packed (interleaved RGB / RGBA / UV / NV12) resize: channel c of every result
equals the oracle (the reference's Generic resize, restated) run on channel c as a plane, bit for
bit -- through packed_tile_kernel and packed_general_kernel, over shapes, layouts, bands, host
pointers, NV12, the plan cache and the error paths.  Small shapes, 2 frames: a few seconds each."""
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
    reference reads outside its rows there: no pinned answer) are left out while generating."""
    rng = random.Random(1409)
    out = []
    while len(out) < 24:
        m = ("lanczos", "area", "linear")[len(out) % 3]
        d = rng.randint(1, 5) if m == "lanczos" else 0
        sw, sh, dw, dh = (rng.randint(4, 96) for _ in range(4))
        if m == "linear" and (dw > 2 * sw or dh > 2 * sh):
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
