"""The integer RGB -> YUV definition of the "resize to NV12 / I420" entries, on the CPU: the table against the
standards' real coefficients, the library's host twins (iqo_host_rgb_to_yuv, iqo_host_rgb_to_yuv420)
against tests/rgbyuv_cases.py's numpy over all 2^24 triples and at the edge sizes, the properties
include/iqo_hip.h states (grey, ranges, the live upper clamp of full-range U and V, non-negative
accumulators), the round trip through iqo_host_yuv_to_rgb, and the workspace query.  No GPU."""
import ctypes
import functools

import numpy as np
import pytest

import rgbyuv_cases as ry

import libiqo_amd

EINVAL = -1
SIZE_MAX = ctypes.c_size_t(-1).value


@functools.lru_cache(maxsize=None)
def all_triples():
    """uint8 [2^24, 3], read-only: every (R, G, B)."""
    i = np.arange(1 << 24, dtype=np.uint32)
    out = np.stack([(i >> 16).astype(np.uint8), (i >> 8).astype(np.uint8), i.astype(np.uint8)], axis=1)
    out.setflags(write=False)
    return out


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_table_is_the_rounded_real_coefficients(standard):
    t = ry.TABLE[standard]
    assert t == ry.real_constants(standard)
    yoff, cyr, cyg, cyb, cur, cug, cub, cvr, cvg, cvb = t
    assert cur + cug == cub and cvg + cvb == cvr
    assert cyr + cyg + cyb == ry.luma_scale(standard) == (14071 if yoff else 16384)


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_host_444_is_the_formula_on_every_triple(standard):
    rgb = all_triples()
    y, u, v = libiqo_amd.host_rgb_to_yuv(standard, rgb)
    ey, eu, ev = ry.rgb_to_yuv(standard, rgb)
    assert np.array_equal(y, ey) and np.array_equal(u, eu) and np.array_equal(v, ev)
    # by name too
    y2, _, _ = libiqo_amd.host_rgb_to_yuv(ry.NAMES[standard], rgb[:4096])
    assert np.array_equal(y2, ey[:4096])


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_properties_of_the_definition(standard):
    rgb = all_triples()
    limited = standard not in ry.FULL_RANGE
    ay, au, av = ry.accumulators(standard, rgb[:, 0], rgb[:, 1], rgb[:, 2], ry.SHIFT)
    # no accumulator is negative (the smallest is the rounding term), none passes 2^22: no lower clamp
    lowest = min(ay.min(), au.min(), av.min())
    assert lowest == ((16 << ry.SHIFT) + 8192 if limited else 8192)  # Y of black
    assert max(ay.max(), au.max(), av.max()) <= 1 << 22
    y, u, v = ry.rgb_to_yuv(standard, rgb, raw=True)
    assert y.max() <= 255  # Y needs no clamp
    grey = rgb[:, 0] == rgb[:, 1]
    grey &= rgb[:, 1] == rgb[:, 2]
    assert grey.sum() == 256 and (u[grey] == 128).all() and (v[grey] == 128).all()
    assert (y[grey][0], y[grey][-1]) == ((16, 235) if limited else (0, 255))
    if limited:
        assert (y.min(), y.max()) == (16, 235)
        assert (u.min(), u.max()) == (16, 240) and (v.min(), v.max()) == (16, 240)
    else:
        # the min is live: 256 before it, at pure blue (U) and pure red (V)
        assert u.max() == 256 and v.max() == 256
        assert u[0x0000ff] == 256 and v[0xff0000] == 256
        assert (y.min(), y.max()) == (0, 255) and u.min() >= 0 and v.min() >= 0
    # the sums of four pixels: the same bounds two bits up
    s = np.array([[0, 0, 0], [1020, 1020, 1020], [0, 0, 1020], [1020, 0, 0], [1020, 1020, 0], [0, 1020, 1020],
                  [0, 1020, 0], [1020, 0, 1020]], np.int32)
    _, su, sv = ry.accumulators(standard, s[:, 0], s[:, 1], s[:, 2], ry.SUM_SHIFT)
    assert min(su.min(), sv.min()) >= 32768 and max(su.max(), sv.max()) <= 1 << 24


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_round_trip_through_host_yuv_to_rgb(standard):
    rgb = all_triples()
    y, u, v = libiqo_amd.host_rgb_to_yuv(standard, rgb)
    back = libiqo_amd.host_yuv_to_rgb(standard, y, u, v)
    err = np.abs(back.astype(np.int16) - rgb.astype(np.int16))
    bound = 1 if standard in ry.FULL_RANGE else 2
    print("%s: round-trip max error %d, mean %.3f" % (ry.NAMES[standard], err.max(), err.mean()))
    assert err.max() <= bound


def _noise(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


@pytest.mark.parametrize("size", ry.HOST_SIZES, ids=lambda s: "%dx%d" % s)
def test_host_420_is_the_formula(size):
    w, h = size
    for standard in ry.STANDARDS:
        img = _noise(w, h, 100 * w + h + standard)
        y, u, v = libiqo_amd.host_rgb_to_yuv420(standard, img)
        ey, eu, ev = ry.rgb_to_yuv420(standard, img)
        assert y.shape == (h, w) and u.shape == v.shape == (h // 2, w // 2)
        assert np.array_equal(y, ey) and np.array_equal(u, eu) and np.array_equal(v, ev), (size, standard)


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_host_420_on_pure_blue_and_pure_red_blocks(standard):
    for colour, plane in (((0, 0, 255), 1), ((255, 0, 0), 2)):
        img = np.broadcast_to(np.array(colour, np.uint8), (2, 2, 3)).copy()
        raw = ry.rgb_to_yuv420(standard, img, raw=True)
        if standard in ry.FULL_RANGE:
            assert raw[plane][0, 0] == 256  # the sum form reaches 256 there: the min is live
        else:
            assert raw[plane][0, 0] == 240
        got = libiqo_amd.host_rgb_to_yuv420(standard, img)
        exp = ry.rgb_to_yuv420(standard, img)
        assert all(np.array_equal(g, e) for g, e in zip(got, exp))
        assert got[plane][0, 0] == min(255, int(raw[plane][0, 0]))


@pytest.mark.parametrize("standard", ry.STANDARDS, ids=ry.NAMES.get)
def test_sum_form_is_the_pixel_form_on_flat_blocks(standard):
    rgb = all_triples()[::251]  # 66,842 colours, every byte value in every channel
    assert all(len(np.unique(rgb[:, c])) == 256 for c in range(3))
    flat = np.broadcast_to(rgb[:, None, None, :], (len(rgb), 2, 2, 3))
    y4, u4, v4 = ry.rgb_to_yuv(standard, rgb)
    y, u, v = ry.rgb_to_yuv420(standard, flat)
    assert np.array_equal(u[:, 0, 0], u4) and np.array_equal(v[:, 0, 0], v4)
    assert np.array_equal(y, np.broadcast_to(y4[:, None, None], y.shape))
    # ... and through the library, as one image of 2 x 2 blocks side by side
    img = np.ascontiguousarray(flat[:4096].transpose(1, 0, 2, 3).reshape(2, 2 * 4096, 3))
    _, gu, gv = libiqo_amd.host_rgb_to_yuv420(standard, img)
    assert np.array_equal(gu[0], u4[:4096]) and np.array_equal(gv[0], v4[:4096])


def test_host_entries_reject():
    L = libiqo_amd.lib()
    rgb = np.zeros((2, 2, 3), np.uint8)
    y, u, v = np.zeros(4, np.uint8), np.zeros(1, np.uint8), np.zeros(1, np.uint8)
    p = lambda a: a.ctypes.data  # noqa: E731
    for standard in (-1, 4):
        assert L.iqo_host_rgb_to_yuv(standard, 4, p(rgb), p(y), p(y), p(y)) == EINVAL
        assert L.iqo_host_rgb_to_yuv420(standard, 2, 2, p(rgb), p(y), p(u), p(v)) == EINVAL
    for args in ((None, p(y), p(u), p(v)), (p(rgb), None, p(u), p(v)), (p(rgb), p(y), None, p(v)),
                 (p(rgb), p(y), p(u), None)):
        assert L.iqo_host_rgb_to_yuv(0, 1, *args) == EINVAL
        assert L.iqo_host_rgb_to_yuv420(0, 2, 2, *args) == EINVAL
    assert L.iqo_host_rgb_to_yuv420(0, 1, 2, p(rgb), p(y), p(u), p(v)) == EINVAL
    assert L.iqo_host_rgb_to_yuv420(0, 2, 1, p(rgb), p(y), p(u), p(v)) == EINVAL
    assert (y == 0).all() and (u == 0).all() and (v == 0).all()
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_rgb_to_yuv("bt2020", rgb)
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_rgb_to_yuv420(0, rgb[..., :2])


def test_gpu_cases_cover_what_they_claim():
    for shape in ry.GPU_SHAPES:
        m, d, sw, sh, dw, dh, px = shape
        for C in (3, 4):
            assert libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px) == ry.first_pass_kernel(shape, C)
    assert {ry.first_pass_kernel(s, 3) for s in ry.GPU_SHAPES} == {"packed_tile", "packed_general"}
    for C, layout in ry.COMBOS:
        rows = [r for r in ry.GPU_CASES if (r[1], r[2]) == (C, layout)]
        assert {r[3] for r in rows} == set(ry.ORDERS) and {r[4] for r in rows} == set(ry.STANDARDS)
    for method in ("lanczos", "area", "linear"):
        ratios = {s[4] > s[2] for s in ry.GPU_SHAPES if s[0] == method}
        assert ratios == {True, False}, method
    dws, dhs = {s[4] for s in ry.GPU_SHAPES}, {s[5] for s in ry.GPU_SHAPES}
    assert {2, 3} <= dws and {1, 4, 7} <= {w % 8 for w in dws} and {2, 3} <= dhs


def test_workspace_query():
    q = libiqo_amd.rgb_yuv_workspace_bytes
    # rows of 8-pixel groups, padded to 16 bytes; + 15 for the base
    assert q(33, 17, 3, 3) == 3 * 17 * 128 + 15      # 40 pixels x 3 = 120 -> 128
    assert q(33, 17, 4, 3) == 3 * 17 * 160 + 15
    assert q(2, 2, 3, 1) == 2 * 32 + 15              # 8 pixels x 3 = 24 -> 32
    assert q(8, 2, 4, 0) == 15
    for dw, dh, C, n in ((1920, 1080, 3, 64), (52, 36, 4, 5)):
        assert q(dw, dh, C, n) >= n * dh * dw * C + 15
        assert q(dw, dh, C, n) - 15 == n * (q(dw, dh, C, 1) - 15)
    # saturation instead of a wrap; SIZE_MAX for what no plan has
    assert q(1 << 20, 1 << 20, 4, 1 << 30) == SIZE_MAX
    assert q((1 << 31) - 1, (1 << 31) - 1, 4, SIZE_MAX) == SIZE_MAX
    assert q(1 << 31, 2, 3, 1) == SIZE_MAX and q(2, 1 << 31, 3, 1) == SIZE_MAX
    assert q(64, 64, 2, 1) == SIZE_MAX and q(64, 64, 5, 1) == SIZE_MAX and q(64, 64, 1, 1) == SIZE_MAX
    big = q((1 << 31) - 1, (1 << 31) - 1, 4, 1)
    assert big < SIZE_MAX and q((1 << 31) - 1, (1 << 31) - 1, 4, 2) == SIZE_MAX
