"""NV12 / I420 to RGB with chroma filtered to the full output grid (IQO_CHROMA_FULL, chroma="full"), the
part that needs no GPU: the header and the exported symbols, the Python surface, the host query of the
chroma plan's kernel family and its rejections, the workspace query, the null-plan and bad-mode returns,
and whether the shapes of tests/test_yuv444_gpu.py have an oracle answer, reach both clamps and tell the
full grid from replicated chroma.
"""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import oracle_lib as ol
import yuv444_cases as y4
import yuvrgb_cases as yr

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

ENTRIES = {
    # name: (return type, argument count)
    "iqo_hip_nv12_plan_set_chroma": ("int", 2),
    "iqo_hip_yuv_plan_set_chroma": ("int", 2),
    "iqo_hip_nv12_plan_chroma": ("int", 1),
    "iqo_hip_yuv_plan_chroma": ("int", 1),
    "iqo_hip_yuv_rgb_workspace_bytes_chroma": ("size_t", 4),
    "iqo_host_yuv_chroma_full_kernel": ("int", 7),
}


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


# ---- the ABI surface

def test_header_declares_the_entries_and_the_constants():
    h = _read("include", "iqo_hip.h")
    for name, (ret, nargs) in ENTRIES.items():
        m = re.search(r"\b%s\s+%s\s*\(([^)]*)\)\s*;" % (ret, name), h)
        assert m, name
        assert len(m.group(1).split(",")) == nargs, name
    for name, value in (("IQO_CHROMA_REPLICATE", 0), ("IQO_CHROMA_FULL", 1)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), h), name
    # the definition stands next to the standards: after IQO_CS_*, before the calls it governs
    assert h.index("IQO_CS_BT709_FULL = 3") < h.index("IQO_CHROMA_FULL = 1") < h.index("int iqo_hip_resize_nv12_rgb_device")
    # no existing signature changed
    assert re.search(r"size_t\s+iqo_hip_yuv_rgb_workspace_bytes\s*\(size_t dstW, size_t dstH, size_t nFrames\)\s*;", h)


def test_library_exports_the_entries():
    import libiqo_amd
    L = libiqo_amd.lib()
    for name, (_, nargs) in ENTRIES.items():
        assert hasattr(L, name), name
        assert len(getattr(L, name).argtypes) == nargs, name
    assert L.iqo_hip_yuv_rgb_workspace_bytes_chroma.restype is ctypes.c_size_t


def test_python_surface():
    import libiqo_amd
    assert (libiqo_amd.CHROMA_REPLICATE, libiqo_amd.CHROMA_FULL) == (0, 1)
    for name in ("CHROMA_REPLICATE", "CHROMA_FULL", "host_chroma_full_kernel", "yuv_rgb_workspace_bytes"):
        assert name in libiqo_amd.__all__, name
    for cls in (libiqo_amd.Nv12Resizer, libiqo_amd.Yuv420Resizer):
        sig = inspect.signature(cls.__init__)
        assert list(sig.parameters) == ["self", "method", "degree", "srcW", "srcH", "dstW", "dstH", "device", "chroma"]
        assert sig.parameters["chroma"].default == "replicate" and sig.parameters["device"].default is None
        assert cls.chroma == "replicate"
        assert callable(cls.chroma_kernel) and callable(cls.set_chroma)
        assert list(inspect.signature(cls.set_option).parameters) == ["self", "key", "value", "plane"]
        # a mode that does not exist is rejected before a plan (and a device) is asked for
        for bad in ("444", "FULL", 1, None):
            with pytest.raises(libiqo_amd.IqoError):
                cls("area", 0, 16, 16, 8, 8, chroma=bad)
    sig = inspect.signature(libiqo_amd.yuv_rgb_workspace_bytes)
    assert list(sig.parameters) == ["dstW", "dstH", "nFrames", "chroma"] and sig.parameters["chroma"].default == "replicate"
    sig = inspect.signature(libiqo_amd.host_chroma_full_kernel)
    assert list(sig.parameters) == ["method", "degree", "srcW", "srcH", "dstW", "dstH", "layout"]
    assert sig.parameters["layout"].default == "nv12"
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_chroma_full_kernel("area", 0, 16, 16, 8, 8, layout="yuyv")
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.yuv_rgb_workspace_bytes(8, 8, 1, chroma="444")


def test_null_plan_and_bad_mode():
    import libiqo_amd
    L = libiqo_amd.lib()
    for setter in (L.iqo_hip_nv12_plan_set_chroma, L.iqo_hip_yuv_plan_set_chroma):
        for mode in (0, 1, 2, -1):
            assert setter(None, mode) == y4.EINVAL
    assert L.iqo_hip_nv12_plan_chroma(None) == y4.EINVAL
    assert L.iqo_hip_yuv_plan_chroma(None) == y4.EINVAL
    assert L.iqo_hip_nv12_plane(None, 2) is None and L.iqo_hip_yuv_plane(None, 2) is None


# ---- the host query

def test_host_query_reports_the_families():
    import libiqo_amd
    q = libiqo_amd.host_chroma_full_kernel
    for layout, rows in (("nv12", y4.NV12_CASES), ("i420", y4.I420_CASES)):
        for case, _, family in rows:
            m, d, sw, sh, dw, dh, _ = case
            assert q(m, d, sw, sh, dw, dh, layout=layout) == family, (layout, case)
            # ... which is what the plane resizers' own queries say of srcW/2 x srcH/2 -> dstW x dstH at pxScale 1
            if layout == "nv12":
                assert libiqo_amd.host_packed_kernel_for(m, d, 2, sw // 2, sh // 2, dw, dh, 1) == family
            else:
                assert libiqo_amd.host_kernel_for(m, d, sw // 2, sh // 2, dw, dh, 1) == family
    assert q("area", 0, 16, 16, 2, 2) == q("area", 0, 16, 16, 2, 2, layout="nv12")
    # the planar lists reach every family named in the issue
    assert {f for _, _, f in y4.I420_CASES} == {"lanczos_up2", "ryg", "lanczos_d32", "lanczos_stream", "walk",
                                                 "area_int", "general", "tile", "linear_up2"}
    assert {f for _, _, f in y4.NV12_CASES} == {"packed_tile", "packed_general"}


def test_host_query_rejections():
    import libiqo_amd
    L = libiqo_amd.lib()
    M = {"lanczos": 0, "area": 1, "linear": 2}
    for (m, d, sw, sh, dw, dh), status in y4.REJECTED:
        for uv2 in (0, 1):
            assert L.iqo_host_yuv_chroma_full_kernel(M[m], d, sw, sh, dw, dh, uv2) == status, (m, sw, sh, dw, dh, uv2)
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_chroma_full_kernel(m, d, sw, sh, dw, dh)
        # the plans above it are accepted: Y, and chroma at half size
        libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh)
        libiqo_amd.host_kernel_for(m, d, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1)
    assert ol.lanczos_rows_defined(3, 3, 3) and ol.lanczos_rows_defined(3, 1, 1, 2) and not ol.lanczos_rows_defined(3, 1, 3)
    # Linear exactly 2x is the last accepted ratio, per axis
    assert L.iqo_host_yuv_chroma_full_kernel(2, 0, 40, 24, 40, 24, 1) >= 0
    assert L.iqo_host_yuv_chroma_full_kernel(2, 0, 40, 24, 41, 24, 1) == y4.EUNSUP
    assert L.iqo_host_yuv_chroma_full_kernel(2, 0, 40, 24, 40, 25, 0) == y4.EUNSUP
    assert L.iqo_host_yuv_chroma_full_kernel(2, 0, 41, 25, 40, 24, 0) >= 0       # srcW/2 = 20
    assert L.iqo_host_yuv_chroma_full_kernel(1, 0, 20, 12, 40, 24, 1) >= 0       # Area has no such limit
    # what the NV12 / I420 plan constructors reject
    for bad in ((3, 0, 16, 16, 8, 8), (-1, 0, 16, 16, 8, 8), (1, 0, 1, 16, 8, 8), (1, 0, 16, 16, 8, 1)):
        assert L.iqo_host_yuv_chroma_full_kernel(*bad, 1) == y4.EINVAL, bad


# ---- the workspace query

def test_workspace_query():
    import libiqo_amd
    L = libiqo_amd.lib()
    q = libiqo_amd.yuv_rgb_workspace_bytes
    sizes = [2, 3, 7, 8, 9, 15, 16, 17, 31, 32, 33, 224, 1079, 1080, 1920, 3840]
    frames = [0, 1, 2, 3, 64, 65535]
    for w in sizes:
        for h in sizes:
            for n in frames:
                old = L.iqo_hip_yuv_rgb_workspace_bytes(w, h, n)
                assert q(w, h, n) == q(w, h, n, "replicate") == L.iqo_hip_yuv_rgb_workspace_bytes_chroma(w, h, n, 0) == old
                full = q(w, h, n, "full")
                assert full == L.iqo_hip_yuv_rgb_workspace_bytes_chroma(w, h, n, 1)
                assert full >= n * 3 * w * h and full >= old, (w, h, n)
            full = [q(w, h, n, "full") for n in frames]
            assert full == sorted(full)
    for n in frames:
        for fixed in sizes:
            ws = [q(w, fixed, n, "full") for w in range(2, 70)]
            hs = [q(fixed, h, n, "full") for h in range(2, 70)]
            assert ws == sorted(ws) and hs == sorted(hs), (fixed, n)
    # the padding is rows rounded to 16 bytes and the base's 15
    assert q(224, 224, 64, "full") <= 64 * 224 * 224 * 3 * 7 // 6
    # the layout: Y, then U and V at dstH rows, every row padded to 8 pixels and 16 bytes
    for w, h in ((33, 17), (2, 2), (224, 224), (1920, 1080)):
        st = (((w + 7) // 8 * 8) + 15) // 16 * 16
        assert q(w, h, 5, "full") == 5 * 3 * st * h + 15, (w, h)
    # sizes no plan has, and a mode that does not exist, saturate instead of wrapping
    top = ctypes.c_size_t(-1).value
    assert q(1 << 40, 1 << 40, 1 << 40, "full") == top
    assert q((1 << 31) - 1, (1 << 31) - 1, 1 << 40, "full") == top
    assert q(1 << 31, 2, 1, "full") == top
    for mode in (2, -1):
        assert L.iqo_hip_yuv_rgb_workspace_bytes_chroma(224, 224, 1, mode) == top


# ---- the GPU tests' shapes

ALL_ROWS = y4.NV12_CASES + y4.I420_CASES


def test_every_shape_has_plans_and_an_oracle_answer():
    import libiqo_amd
    for case, standard, _ in ALL_ROWS:
        m, d, sw, sh, dw, dh, layout = case
        libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh)  # raises for a shape the Y plan rejects
        libiqo_amd.host_kernel_for(m, d, sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1)
        if m == "lanczos":
            assert ol.lanczos_rows_defined(d, sh, dh) and ol.lanczos_rows_defined(d, sh // 2, dh)
        if m == "linear":
            assert dw <= 2 * (sw // 2) and dh <= 2 * (sh // 2)
        y, u, v = y4.expected_planes(case)
        assert y.shape == u.shape == v.shape == (yr.N_FRAMES, dh, dw)
        assert np.array_equal(y, yr.expected_planes(case)[0])  # Y is the existing Y plane
    for rows in (y4.NV12_CASES, y4.I420_CASES):
        assert [s for _, s, _ in rows] == [yr.STANDARDS[i % 4] for i in range(len(rows))]


def test_inputs_reach_both_clamps_in_every_channel():
    for case, standard, _ in ALL_ROWS:
        raw = y4.raw_rgb(case, standard)
        lo, hi = (raw < 0).sum(axis=(0, 1, 2)), (raw > 255).sum(axis=(0, 1, 2))
        assert lo.min() > 0 and hi.min() > 0, (case, lo.tolist(), hi.tolist())


def test_full_differs_from_replicated_chroma():
    """A kernel that still replicates a half-size plane fails every row."""
    for case, standard, _ in ALL_ROWS:
        full, rep = y4.expected_rgb(case, standard), yr.expected_rgb(case, standard)
        assert full.shape == rep.shape
        assert (full != rep).any(), case


def test_shapes_cover_the_edges():
    dws = [c[4] for c, _, _ in y4.NV12_CASES]
    dhs = [c[5] for c, _, _ in y4.NV12_CASES]
    assert 2 in dws and 3 in dws and 2 in dhs
    assert {1, 4, 6, 7, 0} <= {w % 8 for w in dws}
    assert any(w % 2 and h % 2 for w, h in zip(dws, dhs)) and any(h % 2 and not w % 2 for w, h in zip(dws, dhs))
    shapes = [c[:6] for c, _, _ in y4.NV12_CASES]
    assert ("lanczos", 3, 64, 32, 33, 17) in shapes
    assert any(m == "lanczos" and (sw // 2, sh // 2) == (dw, dh) for m, _, sw, sh, dw, dh in shapes)   # identity chroma
    assert any(m == "linear" and (2 * (sw // 2), 2 * (sh // 2)) == (dw, dh) for m, _, sw, sh, dw, dh in shapes)
    for m in ("lanczos", "area"):
        assert any(s[0] == m and s[4] > s[2] // 2 for s in shapes), m + " chroma up-scale"
        assert any(s[0] == m and s[4] < s[2] // 2 for s in shapes), m + " chroma down-scale"
    # more than one pixel group per row and more than one 256-thread block per call
    assert any(w > 16 for w in dws)
    assert any(yr.N_FRAMES * c[5] * ((c[4] + 7) // 8) > 256 for c, _, _ in ALL_ROWS)
