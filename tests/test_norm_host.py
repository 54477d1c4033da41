"""Normalised planar float output of the packed resize (iqo_hip_resize_device_norm), the part that
needs no GPU: the ABI symbol and its header declaration, the null-plan status, the Python surface,
and the property of the test constants that lets tests/test_norm_gpu.py tell a fused multiply-add
from the pinned two-rounding epilogue.
"""
import ctypes
import inspect
import os
import re

import numpy as np

import norm_cases as nc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1


def _header():
    with open(os.path.join(ROOT, "include", "iqo_hip.h")) as f:
        return f.read()


def test_library_exports_the_norm_entry():
    import libiqo_amd
    L = libiqo_amd.lib()
    assert hasattr(L, "iqo_hip_resize_device_norm")
    assert len(L.iqo_hip_resize_device_norm.argtypes) == 11


def test_header_declares_the_norm_entry():
    h = _header()
    assert re.search(r"int\s+iqo_hip_resize_device_norm\s*\(\s*iqo_hip_plan\s*\*", h)
    assert re.search(r"\}\s*iqo_hip_norm\s*;", h)
    for name, value in (("IQO_OUT_F32", 1), ("IQO_OUT_F16", 2), ("IQO_OUT_BF16", 3)):
        assert re.search(r"\b%s\s*=\s*%d\b" % (name, value), h), name
    assert (nc.OUT_F32, nc.OUT_F16, nc.OUT_BF16) == (1, 2, 3)
    # the 1-channel restriction is part of the documented interface
    at = re.search(r"enum\s*\{\s*IQO_OUT_F32", h).start()
    assert "IQO_HIP_EUNSUP" in h[at - 3000:at]


def test_python_struct_matches_the_header_layout():
    import libiqo_amd
    n = libiqo_amd.Norm
    assert [f[0] for f in n._fields_] == ["dtype", "planes", "order", "scale", "bias"]
    assert ctypes.sizeof(n) == 4 + 4 + 16 + 16 + 16
    assert (libiqo_amd.OUT_F32, libiqo_amd.OUT_F16, libiqo_amd.OUT_BF16) == (1, 2, 3)


def test_null_plan_is_einval():
    import libiqo_amd
    L = libiqo_amd.lib()
    n = libiqo_amd.Norm(nc.OUT_F32, 3)
    for i in range(3):
        n.order[i], n.scale[i], n.bias[i] = i, 1.0, 0.0
    # never dereferenced: the null plan is rejected first
    rc = L.iqo_hip_resize_device_norm(None, 1, 64, 64 * 64, 0x1000, ctypes.byref(n), 64, 64 * 64, 3 * 64 * 64, 0x2000,
                                      None)
    assert rc == EINVAL


def test_resize_normalized_on_every_resizer_class():
    import libiqo_amd
    for cls in (libiqo_amd.LanczosResizer, libiqo_amd.AreaResizer, libiqo_amd.LinearResizer):
        fn = getattr(cls, "resize_normalized")
        params = list(inspect.signature(fn).parameters)
        assert params == ["self", "src", "scale", "bias", "dtype", "order", "out", "stream"], (cls, params)


def test_constants_tell_an_fma_from_two_roundings():
    """For every channel's (scale, bias) some byte values give different float32 results under one
    rounding (a fused multiply-add) and under two: the noise frames of the GPU tests hold every byte
    value, so a contracted epilogue cannot pass them."""
    v = np.arange(256, dtype=np.uint8)
    counts = []
    for s, b in zip(nc.NORM_SCALE, nc.NORM_BIAS):
        assert isinstance(s, np.float32) and isinstance(b, np.float32)
        two, one = nc.affine_f32(v, s, b), nc.fma_f32(v, s, b)
        counts.append(int((two.view(np.int32) != one.view(np.int32)).sum()))
        assert np.isfinite(two.astype(np.float16)).all()  # every value is finite in fp16
    assert all(c >= 1 for c in counts), counts
    assert counts == [133, 132, 124, 158], counts


def test_noise_frames_hold_the_fma_sensitive_bytes():
    """The frames the GPU tests feed do contain byte values at which the two forms differ (the
    inputs are resized first, so this is checked on the expected U8 output of one shape)."""
    import packed_cases as pc
    u8 = pc.expected_for(pc.SHAPES[0], 3)
    for c in range(3):
        two = nc.affine_f32(u8[..., c], nc.NORM_SCALE[c], nc.NORM_BIAS[c])
        one = nc.fma_f32(u8[..., c], nc.NORM_SCALE[c], nc.NORM_BIAS[c])
        assert (two.view(np.int32) != one.view(np.int32)).any(), c
