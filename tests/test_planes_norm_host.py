"""Planar U8 frames straight to normalised tensors (iqo_hip_resize_planes_norm_device), the part that needs
no GPU: the two ABI symbols and their header declarations, the null-plan status, the workspace query, the
Python surface, and the expected-value helper of tests/planes_norm_cases.py against a hand-written numpy
expression.
"""
import ctypes
import inspect
import os
import re

import numpy as np

import norm_cases as nc
import planes_norm_cases as pn

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
EINVAL = -1
SIZE_MAX = (1 << (8 * ctypes.sizeof(ctypes.c_size_t))) - 1


def _header():
    with open(os.path.join(ROOT, "include", "iqo_hip.h")) as f:
        return f.read()


def test_library_exports_both_entries():
    import libiqo_amd
    L = libiqo_amd.lib()
    assert len(L.iqo_hip_planes_norm_workspace_bytes.argtypes) == 4
    assert L.iqo_hip_planes_norm_workspace_bytes.restype is ctypes.c_size_t
    assert len(L.iqo_hip_resize_planes_norm_device.argtypes) == 15


def test_header_declares_both_entries():
    h = _header()
    assert re.search(r"size_t\s+iqo_hip_planes_norm_workspace_bytes\s*\(\s*size_t\s+dstW\s*,\s*size_t\s+dstH\s*,"
                     r"\s*int\s+srcPlanes\s*,\s*size_t\s+nFrames\s*\)", h)
    m = re.search(r"int\s+iqo_hip_resize_planes_norm_device\s*\(([^)]*)\)", h)
    assert m
    args = [a.strip() for a in m.group(1).split(",")]
    assert len(args) == 15 and args[0].startswith("iqo_hip_plan") and args[2] == "int srcPlanes", args
    # iqo_hip_resize_device_norm's comment sends planar callers here
    at = re.search(r"enum\s*\{\s*IQO_OUT_F32", h).start()
    assert "iqo_hip_resize_planes_norm_device" in h[at - 3000:at]


def test_null_plan_is_einval():
    import libiqo_amd
    L = libiqo_amd.lib()
    n = libiqo_amd.Norm(nc.OUT_F32, 3)
    for i in range(3):
        n.order[i], n.scale[i], n.bias[i] = i, 1.0, 0.0
    # never dereferenced: the null plan is rejected first
    rc = L.iqo_hip_resize_planes_norm_device(None, 1, 3, 64, 64 * 64, 3 * 64 * 64, 0x1000, ctypes.byref(n), 64 * 4,
                                             64 * 64 * 4, 3 * 64 * 64 * 4, 0x2000, 0x3000, 1 << 20, None)
    assert rc == EINVAL


def test_workspace_query():
    import libiqo_amd
    q = libiqo_amd.planes_norm_workspace_bytes
    for dw, dh, P, n in [(1, 1, 1, 1), (27, 17, 3, 2), (224, 224, 3, 64), (1920, 1080, 4, 64), (5, 40, 1, 40)]:
        v = q(dw, dh, P, n)
        assert n * P * dh * dw <= v < SIZE_MAX, (dw, dh, P, n, v)
        # monotone in each argument
        assert q(dw + 1, dh, P, n) >= v and q(dw, dh + 1, P, n) >= v and q(dw, dh, P, n + 1) >= v
        assert P == 4 or q(dw, dh, P + 1, n) >= v
    assert q(27, 17, 3, 0) == 15  # no frames: the rounding of the base only
    assert q(27, 17, 0, 2) == SIZE_MAX and q(27, 17, 5, 2) == SIZE_MAX and q(27, 17, -1, 2) == SIZE_MAX
    assert q(27, 17, 3, 1 << 62) == SIZE_MAX and q(1920, 1080, 4, SIZE_MAX) == SIZE_MAX
    assert q(1 << 31, 17, 3, 2) == SIZE_MAX and q(27, 1 << 31, 3, 2) == SIZE_MAX
    # the largest frame a plan can have: saturated or exact, never wrapped
    big = (1 << 31) - 1
    for P in (1, 2, 3, 4):
        assert q(big, big, P, 1) >= P * big * big
    assert q(big, big, 4, 2) == SIZE_MAX


def test_new_methods_on_every_class():
    import libiqo_amd
    for cls in (libiqo_amd.LanczosResizer, libiqo_amd.AreaResizer, libiqo_amd.LinearResizer):
        params = list(inspect.signature(cls.resize_planes_normalized).parameters)
        assert params == ["self", "src", "scale", "bias", "dtype", "order", "out", "stream"], (cls, params)
        # the pinned signature of the packed form is unchanged
        params = list(inspect.signature(cls.resize_normalized).parameters)
        assert params == ["self", "src", "scale", "bias", "dtype", "order", "out", "stream"], (cls, params)
    for cls in (libiqo_amd.Nv12Resizer, libiqo_amd.Yuv420Resizer):
        params = list(inspect.signature(cls.resize_luma_normalized).parameters)
        assert params == ["self", "src", "scale", "bias", "dtype", "out", "stream"], (cls, params)
        params = list(inspect.signature(cls.resize_normalized).parameters)
        assert params == ["self", "src", "scale", "bias", "standard", "dtype", "order", "out", "stream"], (cls, params)


def test_expected_bits_helper():
    """An order with a repeat and a drop, against the expression written out per plane."""
    rng = np.random.RandomState(5)
    u8 = rng.randint(0, 256, size=(2, 4, 3, 5)).astype(np.uint8)
    order, scale, bias = (2, 2, 0), nc.NORM_SCALE[:3], nc.NORM_BIAS[:3]  # planes 1 and 3 dropped, 2 repeated
    f32 = np.empty((2, 3, 3, 5), np.float32)
    for p in range(3):
        prod = (u8[:, order[p]].astype(np.float32) * np.float32(scale[p])).astype(np.float32)
        f32[:, p] = prod + np.float32(bias[p])
    assert f32.dtype == np.float32
    got = pn.expected_bits(u8, order, scale, bias, "float32")
    assert got.shape == (2, 3, 3, 5) and got.dtype == np.int32 and (got == f32.view(np.int32)).all()
    got = pn.expected_bits(u8, order, scale, bias, "float16")
    assert got.dtype == np.int16 and (got == f32.astype(np.float16).view(np.int16)).all()
    got = pn.expected_bits(u8, order, scale, bias, "bfloat16")
    assert (got == nc.bf16_bits(f32)).all()
    # the repeated plane under two maps gives two different planes
    assert (got[:, 0] != got[:, 1]).any()


def test_frames_and_their_fma_sensitive_bytes():
    """frames_for: other bytes per plane, the flat third in plane 0 of frame 1 only; and the resized noise
    holds bytes at which one rounding and two roundings differ, so a contracted epilogue cannot pass."""
    shape = pn.RYG
    src = pn.frames_for(shape)
    assert src.shape == (2, 3, shape[3], shape[2]) and src.dtype == np.uint8
    w3 = shape[2] // 3
    assert (src[1, 0, :, :w3] == 255).all()
    assert not (src[1, 1, :, :w3] == 255).all() and not (src[0, 0, :, :w3] == 255).all()
    assert len({src[f, c].tobytes() for f in range(2) for c in range(3)}) == 6
    u8 = pn.expected_u8(shape)
    assert u8.shape == (2, 3, shape[5], shape[4])
    for c in range(3):
        two = nc.affine_f32(u8[:, c], nc.NORM_SCALE[c], nc.NORM_BIAS[c])
        one = nc.fma_f32(u8[:, c], nc.NORM_SCALE[c], nc.NORM_BIAS[c])
        assert (two.view(np.int32) != one.view(np.int32)).any(), c


def test_shapes_reach_their_families():
    import libiqo_amd
    for shape, family in pn.SHAPES:
        assert libiqo_amd.host_kernel_for(*shape) == family, shape
