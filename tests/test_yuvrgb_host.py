"""NV12 / I420 resize straight to RGB (iqo_hip_resize_nv12_rgb_device and its siblings), the part that
needs no GPU: the integer YUV -> RGB definition through iqo_host_yuv_to_rgb on all 2^24 triples, its
constants, the exported symbols and their header declarations, the null-plan status, the workspace
query, the Python surface, and whether the inputs of tests/test_yuvrgb_gpu.py reach both clamps.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import yuv_cases as yc
import yuvrgb_cases as yr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1

ENTRIES = {
    # name: argument count
    "iqo_hip_yuv_rgb_workspace_bytes": 3,
    "iqo_hip_resize_nv12_rgb_device": 16,
    "iqo_hip_resize_nv12_norm_device": 16,
    "iqo_hip_resize_yuv420_rgb_device": 18,    # U and V pointers, and the trailing `fused`
    "iqo_hip_resize_yuv420_norm_device": 18,
    "iqo_host_yuv_to_rgb": 6,
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


@pytest.fixture(scope="module")
def triples():
    """All 2^24 (Y, U, V), read-only."""
    a = np.arange(1 << 24, dtype=np.uint32)
    out = tuple(((a >> s) & 255).astype(np.uint8) for s in (16, 8, 0))
    for p in out:
        p.setflags(write=False)
    return out


# ---- the definition

@pytest.mark.parametrize("standard", yr.STANDARDS, ids=lambda s: yr.NAMES[s])
def test_host_formula_on_every_triple(standard, triples):
    import libiqo_amd
    y, u, v = triples
    got = libiqo_amd.host_yuv_to_rgb(standard, y, u, v)
    exp = yr.yuv_to_rgb(standard, y, u, v)
    bad = np.flatnonzero((got != exp).any(axis=1))
    assert bad.size == 0, "%d triples differ, first (Y, U, V) = %s: got %s want %s" % (
        bad.size, (y[bad[0]], u[bad[0]], v[bad[0]]), got[bad[0]], exp[bad[0]])
    # both clamps are live in every channel, and int32 has ample room (the issue's figures)
    raw = yr.raw_rgb(standard, y, u, v)
    assert (raw.min(axis=0) < 0).all() and (raw.max(axis=0) > 255).all()
    assert np.abs(raw.astype(np.int64)).max() << yr.SHIFT <= 8954873 + (1 << yr.SHIFT)


def test_constants_are_the_rounded_real_coefficients():
    for s in yr.STANDARDS:
        assert yr.real_constants(s) == yr.TABLE[s], yr.NAMES[s]
    # the one table of the library holds the same rows, in IQO_CS_* order
    rows = re.findall(r"\{\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\}\s*,",
                      _read("libiqo_amd", "csrc", "colorspace.hpp"))
    assert [tuple(int(x) for x in r) for r in rows] == [yr.TABLE[s] for s in yr.STANDARDS]
    # ... and nowhere else in the sources is one of them restated
    for name in ("abi.hip", "kernels_color.hip", "kernels.hpp"):
        assert "19077" not in _read("libiqo_amd", "csrc", name), name


def test_grey_and_range_ends():
    import libiqo_amd
    g = np.arange(256, dtype=np.uint8)
    mid = np.full(256, 128, np.uint8)
    for s in (yr.BT601_FULL, yr.BT709_FULL):  # grey is the identity
        assert (libiqo_amd.host_yuv_to_rgb(s, g, mid, mid) == g[:, None]).all(), yr.NAMES[s]
    for s in (yr.BT601_LIMITED, yr.BT709_LIMITED):  # 16 -> 0, 235 -> 255, monotone in between
        rgb = libiqo_amd.host_yuv_to_rgb(s, g, mid, mid)
        assert (rgb[16] == 0).all() and (rgb[235] == 255).all() and (rgb[:16] == 0).all() and (rgb[235:] == 255).all()
        assert (np.diff(rgb[:, 0].astype(int)) >= 0).all() and (rgb[17] > 0).all() and (rgb[234] < 255).all()


def test_host_formula_errors():
    import libiqo_amd
    L = libiqo_amd.lib()
    a = np.zeros(4, np.uint8)
    out = np.full(12, 0xA5, np.uint8)
    p, o = a.ctypes.data, out.ctypes.data
    assert L.iqo_host_yuv_to_rgb(0, 4, p, p, p, o) == 0
    for bad in ((-1, 4, p, p, p, o), (4, 4, p, p, p, o), (0, 4, None, p, p, o), (0, 4, p, None, p, o),
                (0, 4, p, p, None, o), (0, 4, p, p, p, None)):
        assert L.iqo_host_yuv_to_rgb(*bad) == EINVAL, bad
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_yuv_to_rgb("bt2020", a, a, a)
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_yuv_to_rgb(0, a, a, a[:2])


# ---- the ABI surface

def test_library_exports_the_entries():
    import libiqo_amd
    L = libiqo_amd.lib()
    for name, nargs in ENTRIES.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.iqo_hip_yuv_rgb_workspace_bytes.restype is ctypes.c_size_t


def test_header_declares_the_entries_and_the_enum():
    h = _read("include", "iqo_hip.h")
    for name in ENTRIES:
        assert re.search(r"\b(int|size_t)\s+%s\s*\(" % name, h), name
    for name, value in (("IQO_CS_BT601_LIMITED", 0), ("IQO_CS_BT601_FULL", 1), ("IQO_CS_BT709_LIMITED", 2),
                        ("IQO_CS_BT709_FULL", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), h), name
    # the header's table is the definition's
    for s in yr.STANDARDS:
        assert re.search(r"\s+".join(str(c) for c in yr.TABLE[s]), h), yr.NAMES[s]


def test_python_constants():
    import libiqo_amd
    assert (libiqo_amd.CS_BT601_LIMITED, libiqo_amd.CS_BT601_FULL, libiqo_amd.CS_BT709_LIMITED,
            libiqo_amd.CS_BT709_FULL) == (0, 1, 2, 3)
    assert libiqo_amd.COLOR_STANDARDS == {v: k for k, v in yr.NAMES.items()}
    assert libiqo_amd.RGB_ORDERS == yr.ORDERS
    for name in ("host_yuv_to_rgb", "yuv_rgb_workspace_bytes", "CS_BT709_LIMITED"):
        assert name in libiqo_amd.__all__, name


def test_null_plan_is_einval():
    import libiqo_amd
    L = libiqo_amd.lib()
    order = (ctypes.c_int * 4)(0, 1, 2, 3)
    n = libiqo_amd.Norm(1, 3)
    for i in range(3):
        n.order[i], n.scale[i], n.bias[i] = i, 1.0, 0.0
    fused = ctypes.c_int(7)
    # never dereferenced: the null plan is rejected first
    src, dst, ws = 0x1000, 0x2000, 0x3000
    assert L.iqo_hip_resize_nv12_rgb_device(None, 1, 64, 64, 6144, src, src, 0, 3, order, 192, 12288, dst, ws, 1 << 20,
                                            None) == EINVAL
    assert L.iqo_hip_resize_nv12_norm_device(None, 1, 64, 64, 6144, src, src, 0, ctypes.byref(n), 256, 16384, 49152, dst,
                                             ws, 1 << 20, None) == EINVAL
    assert L.iqo_hip_resize_yuv420_rgb_device(None, 1, 64, 32, 6144, src, src, src, 0, 3, order, 192, 12288, dst, ws,
                                              1 << 20, None, ctypes.byref(fused)) == EINVAL
    assert fused.value == 0
    fused.value = 7
    assert L.iqo_hip_resize_yuv420_norm_device(None, 1, 64, 32, 6144, src, src, src, 0, ctypes.byref(n), 256, 16384,
                                               49152, dst, ws, 1 << 20, None, ctypes.byref(fused)) == EINVAL
    assert fused.value == 0


def test_workspace_query():
    import libiqo_amd
    q = libiqo_amd.yuv_rgb_workspace_bytes
    sizes = [2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 224, 1079, 1080, 1920, 3840]
    frames = [0, 1, 2, 3, 64, 65535]
    for w in sizes:
        for h in sizes:
            for n in frames:
                need = n * (w * h + 2 * (w // 2) * (h // 2))
                assert q(w, h, n) >= need, (w, h, n)
    # monotone in every argument
    for w in sizes:
        for h in sizes:
            assert [q(w, h, n) for n in frames] == sorted(q(w, h, n) for n in frames)
    for n in frames:
        for fixed in sizes:
            ws = [q(w, fixed, n) for w in range(2, 70)]
            hs = [q(fixed, h, n) for h in range(2, 70)]
            assert ws == sorted(ws) and hs == sorted(hs), (fixed, n)
    # the padding is rows rounded to 16 bytes and the base's 15: at most a sixth of a 224 x 224 batch
    assert q(224, 224, 64) <= 64 * 224 * 224 * 3 // 2 * 7 // 6
    # a size no plan has saturates instead of wrapping
    assert q(1 << 40, 1 << 40, 1 << 40) == ctypes.c_size_t(-1).value


def test_python_methods():
    import libiqo_amd
    for cls in (libiqo_amd.Nv12Resizer, libiqo_amd.Yuv420Resizer):
        sig = inspect.signature(cls.resize_rgb)
        assert list(sig.parameters) == ["self", "src", "standard", "order", "out", "stream"], cls
        assert (sig.parameters["standard"].default, sig.parameters["order"].default) == ("bt709", "rgb")
        assert sig.parameters["out"].default is None and sig.parameters["stream"].default is None
        sig = inspect.signature(cls.resize_normalized)
        assert list(sig.parameters) == ["self", "src", "scale", "bias", "standard", "dtype", "order", "out",
                                        "stream"], cls
        assert sig.parameters["standard"].default == "bt709" and sig.parameters["dtype"].default is None
        assert sig.parameters["order"].default == (0, 1, 2)
        # what existed stays
        assert callable(cls.resize_frames) and callable(cls.resize_device) and callable(cls.set_option)


# ---- the GPU tests' shapes: the plans take them, and the inputs reach the clamps

def _clamp_counts(case, standard):
    """[[R, G, B below 0], [R, G, B above 255]] over the frames of the case."""
    y, u, v = yr.expected_planes(case)
    raw = yr.planes_to_rgb(standard, y, u, v, raw=True)
    return [[int((raw[..., c] < 0).sum()) for c in range(3)], [int((raw[..., c] > 255).sum()) for c in range(3)]]


def test_every_gpu_shape_has_a_plan_and_an_oracle():
    import libiqo_amd
    for case, _ in yr.I420_CASES:
        m, d, sw, sh, dw, dh, label = case
        assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == label
    for shape, _ in yr.NV12_CASES:
        m, d, sw, sh, dw, dh = shape
        libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh)  # raises for a shape the Y plan rejects
        k = libiqo_amd.host_packed_kernel_for(m, d, 2, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1)
        assert k in ("packed_tile", "packed_general")
        y, u, v = yr.expected_planes(yr.nv12_case(shape))
        assert y.shape == (yr.N_FRAMES, dh, dw) and u.shape == v.shape == (yr.N_FRAMES, dh // 2, dw // 2)
    # both UV kernels are reached without force_general too
    kinds = {libiqo_amd.host_packed_kernel_for(m, d, 2, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1)
             for (m, d, sw, sh, dw, dh), _ in yr.NV12_CASES}
    assert kinds == {"packed_tile", "packed_general"}


def test_nv12_shapes_cover_the_kernel_edges():
    shapes = [s for s, _ in yr.NV12_CASES]
    dws, dhs = [s[4] for s in shapes], [s[5] for s in shapes]
    assert 2 in dws and 3 in dws and 2 in dhs
    assert {1, 4, 7} <= {w % 8 for w in dws}
    assert any(w % 2 and h % 2 for w, h in zip(dws, dhs)) and ("lanczos", 3, 64, 32, 33, 17) in shapes
    # an odd width whose clamped chroma sample lies in the previous thread's group (cw % 4 == 0)
    assert any(w % 2 and (w // 2) % 4 == 0 for w in dws)
    for m in ("lanczos", "area", "linear"):
        assert any(s[0] == m and s[4] > s[2] for s in shapes), m + " up-scale"
        assert any(s[0] == m and s[4] < s[2] for s in shapes), m + " down-scale"
    for group in (yr.I420_CASES, yr.NV12_CASES):
        used = [s for _, s in group]
        assert all(used.count(s) >= 2 for s in yr.STANDARDS)


def test_inputs_reach_both_clamps_in_every_channel():
    """On every shape the GPU tests use, each on its own, every one of R, G and B is clamped at 0 somewhere
    and at 255 somewhere (computed from the oracle planes, with the standard the shape is tested under)."""
    for group, to_case in ((yr.I420_CASES, lambda c: c), (yr.NV12_CASES, yr.nv12_case)):
        for c, standard in group:
            case = to_case(c)
            counts = np.array(_clamp_counts(case, standard))
            assert counts.min() > 0, (yc.cid(case), yr.NAMES[standard], counts.tolist())


def test_clamp_frames_reach_the_clamps_under_every_standard():
    """The two flat frames alone do it, whatever the standard: at the smallest shape (2 x 2 pixels, one
    chroma sample per frame) and at one that averages 48 source pixels per output."""
    small = yr.nv12_case(("area", 0, 16, 16, 2, 2))
    wide = next(c for c, _ in yr.I420_CASES if c[6] == "area6y")
    for case in (small, wide):
        y, u, v = (p[yc.N_FRAMES:] for p in yr.expected_planes(case))
        for standard in yr.STANDARDS:
            raw = yr.planes_to_rgb(standard, y, u, v, raw=True)
            assert ((raw < 0).any(axis=(0, 1, 2)) & (raw > 255).any(axis=(0, 1, 2))).all(), (yc.cid(case), standard)


def test_oracle_chroma_matches_between_the_layouts():
    """An NV12 frame's U and V are the I420 planes' (the packed plan resizes every channel on its own), so
    one expected value serves both resizers."""
    case = yr.nv12_case(yr.NV12_CASES[0][0])
    y, u, v = yc.planes_for(case)
    m, d, sw, sh, dw, dh, _ = case
    cw, ch, cdw, cdh, px = yc.chroma_shape(case)
    eu = ol.run_oracle(m, d, cw, ch, cdw, cdh, px, u[0])
    assert np.array_equal(eu, yc.expected_for(case)[1][0])
    frames = yr.nv12_frames(case)
    assert frames.shape == (yr.N_FRAMES, sw * sh + 2 * cw * ch)
    assert np.array_equal(frames[:yc.N_FRAMES, sw * sh:].reshape(yc.N_FRAMES, ch, cw, 2)[..., 1], v)
