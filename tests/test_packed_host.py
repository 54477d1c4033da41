"""Packed (interleaved RGB / RGBA / UV) resize, the part that needs no GPU: the packed tiling
(plan.cpp build_packed_tables) over the tile tables, run through a scalar emulation of
packed_tile_kernel's index arithmetic (tests/native/packed_emul.cpp, test-only), reproduces the
per-channel oracle; the host-only kernel query; the Python surface.  The GPU parity tests
(tests/test_packed_gpu.py) run the kernels themselves.
"""
import ctypes
import inspect
import os
import subprocess

import numpy as np
import pytest

import oracle_lib as ol
import packed_cases as pc

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
METHODS = {"lanczos": 0, "area": 1, "linear": 2}


@pytest.fixture(scope="module")
def emul():
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "libpacked_emul.so")
    csrc = os.path.join(ROOT, "libiqo_amd", "csrc")
    srcs = [os.path.join(HERE, "native", "packed_emul.cpp"), os.path.join(csrc, "plan.cpp")]
    deps = srcs + [os.path.join(csrc, "plan.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())  # private name + rename: xdist workers may rebuild together
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + csrc,
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    lib = ctypes.CDLL(so)
    lib.packed_emul.restype = ctypes.c_int
    lib.packed_emul.argtypes = ([ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 6 +
                                [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_int)])
    return lib


def run_emul(lib, shape, C, img, dst_pad=0):
    m, d, sw, sh, dw, dh, px = shape
    img = np.ascontiguousarray(img)
    dst = np.full((dh, dw * C + dst_pad), 0xA5, np.uint8)
    geom = (ctypes.c_int * 6)()
    rc = lib.packed_emul(METHODS[m], d, C, sw, sh, dw, dh, px, img.ctypes.data, sw * C, dst.ctypes.data,
                         dst.shape[1], geom)
    return rc, dst, list(geom)


@pytest.mark.parametrize("C", [2, 3, 4])
@pytest.mark.parametrize("shape", pc.SHAPES, ids=pc.sid)
def test_packed_tile_tables_match_oracle(emul, shape, C):
    import libiqo_amd
    m, d, sw, sh, dw, dh, px = shape
    kernel = libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px)
    frames = pc.frames_for(shape, C)
    exp = pc.expected_for(shape, C)
    for f in range(frames.shape[0]):
        rc, out, _ = run_emul(emul, shape, C, frames[f], dst_pad=3)
        assert rc in (0, 1)
        # the emulation and the library agree on which shapes the packed tile kernel takes
        assert kernel == ("packed_tile" if rc == 0 else "packed_general")
        if rc:
            continue
        assert (out[:, dw * C:] == 0xA5).all()
        got = out[:, :dw * C].reshape(dh, dw, C)
        bad = np.argwhere(got != exp[f])
        assert bad.size == 0, bad[:5].tolist()
        if ol.ref_available():
            # the reference's own Generic code, strict-IEEE build: the product (and the oracle) build
            # their tables strict-IEEE, and where the reference's -Ofast build rounds a table entry
            # differently the strict answer is the pinned one (tests/test_oracle_golden.py)
            ref = pc.oracle_packed(shape, frames[f], lambda *a: ol.run_ref(*a, strict=True))
            assert np.array_equal(got, ref)


def test_packed_emulation_covers_the_tile_shapes(emul):
    """All of the shapes but the srcW < 8 one go through the packed tile tables, for every C."""
    for shape in pc.SHAPES:
        for C in (2, 3, 4):
            rc, _, _ = run_emul(emul, shape, C, pc.frames_for(shape, C)[0])
            assert rc == (1 if shape[2] < 8 else 0), (shape, C)


def test_packed_emulation_spans_several_tiles(emul):
    """More than one tile in each axis (the shapes test_packed_gpu.py uses for the same purpose)."""
    for shape in (("lanczos", 3, 213, 100, 140, 70, 1), ("area", 0, 301, 90, 150, 41, 1)):
        for C in (3, 4):
            img = pc.packed_noise(shape[2], shape[3], C, 5)
            rc, out, geom = run_emul(emul, shape, C, img)
            assert rc == 0
            CT, TH = geom[0], geom[1]
            assert shape[4] >= 2 * CT + 3 and shape[5] >= 2 * TH + 1
            assert np.array_equal(out.reshape(shape[5], shape[4], C), pc.oracle_packed(shape, img))


def test_host_packed_kernel_for():
    import libiqo_amd
    L = libiqo_amd.lib()
    for shape in pc.SHAPES:
        m, d, sw, sh, dw, dh, px = shape
        for C in (2, 3, 4):
            k = L.iqo_host_packed_kernel_for(METHODS[m], d, C, sw, sh, dw, dh, px)
            assert k == (15 if sw < 8 else 14), (shape, C)
        assert (L.iqo_host_packed_kernel_for(METHODS[m], d, 1, sw, sh, dw, dh, px) ==
                L.iqo_host_kernel_for(METHODS[m], d, sw, sh, dw, dh, px))
        for C in (0, 5):
            assert L.iqo_host_packed_kernel_for(METHODS[m], d, C, sw, sh, dw, dh, px) < 0
    m, d, sw, sh, dw, dh, px = pc.GENERAL_SHAPE
    for C in (2, 3, 4):
        assert L.iqo_host_packed_kernel_for(METHODS[m], d, C, sw, sh, dw, dh, px) == 15
        assert libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px) == "packed_general"
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_packed_kernel_for("lanczos", 3, 5, 40, 24, 27, 17)


def test_general_shape_is_rejected_by_the_tile_tables(emul):
    """Lanczos-8 at 2:1 has more taps than the widest tile instantiation: no tile tables, so no
    packed tile tables either."""
    img = pc.packed_noise(pc.GENERAL_SHAPE[2], pc.GENERAL_SHAPE[3], 3, 1)
    rc, _, _ = run_emul(emul, pc.GENERAL_SHAPE, 3, img)
    assert rc == 1


def test_python_surface():
    import libiqo_amd
    assert libiqo_amd.KERNELS[14] == "packed_tile" and libiqo_amd.KERNELS[15] == "packed_general"
    assert callable(libiqo_amd.host_packed_kernel_for)
    assert inspect.isclass(libiqo_amd.Nv12Resizer)
    for name in ("resize_device", "resize_frames"):
        assert callable(getattr(libiqo_amd.Nv12Resizer, name))
    for fn in (libiqo_amd.make_resizer, libiqo_amd.LanczosResizer.__init__, libiqo_amd.AreaResizer.__init__,
               libiqo_amd.LinearResizer.__init__):
        assert inspect.signature(fn).parameters["channels"].default == 1
    for name in ("Nv12Resizer", "host_packed_kernel_for"):
        assert name in libiqo_amd.__all__


# ---- the instantiation matrix and the tile shapes (packed_cases.INSTANTIATIONS / GEOMETRY)

MATRIX = pc.INSTANTIATIONS + pc.GEOMETRY + pc.LANCZOS_WIDE_UPSCALES


def test_instantiation_matrix_is_the_full_product():
    """One row per packed_tile_kernel<C, NP, LZ>: 3 x 11 x 2 = 66, over the NP list plan.hpp holds."""
    import re
    text = open(os.path.join(ROOT, "libiqo_amd", "csrc", "plan.hpp")).read()
    k = re.search(r"constexpr int kTileNP\[\]\s*=\s*\{([^}]*)\}", text)
    assert k and tuple(int(v) for v in k.group(1).split(",")) == pc.TILE_NP
    cells = [(C, NP, shape[0] == "lanczos") for shape, C, _, _, NP in pc.INSTANTIATIONS]
    assert len(cells) == 66 and len(set(cells)) == 66
    assert set(cells) == {(C, NP, LZ) for C in (2, 3, 4) for NP in pc.TILE_NP for LZ in (True, False)}
    for shape, C, CT, TH, NP in pc.INSTANTIATIONS:
        m, d, sw, sh, dw, dh, px = shape
        assert sh <= 48 and dw <= 40 and dh <= 32 and sh != dh, shape
    assert {s[0][0] for s in pc.INSTANTIATIONS if s[0][0] != "lanczos"} == {"area", "linear"}
    assert sum(s[0][6] == 2 for s in pc.INSTANTIATIONS) >= 6  # negative border divisors


def test_matrix_shapes_have_a_pinned_answer():
    for shape, C, _, _, _ in MATRIX:
        m, d, sw, sh, dw, dh, px = shape
        assert m != "lanczos" or ol.lanczos_rows_defined(d, sh, dh, px), shape
        assert m != "linear" or (dw <= 2 * sw and dh <= 2 * sh), shape
    for m, d, sw, sh, dw, dh, px in pc.REJECTED:
        assert not ol.lanczos_rows_defined(d, sh, dh, px)
    assert {s[6] for s in pc.REJECTED} == {1, 2}


def test_geometry_covers_every_tile_shape(emul):
    """Every CT and every TH, each with two tiles or more and a partial last one."""
    cts, ths, odd_bytes, both_borders = set(), set(), False, False
    for shape, C, CT, TH, NP in pc.GEOMETRY:
        m, d, sw, sh, dw, dh, px = shape
        rc, _, geom = run_emul(emul, shape, C, pc.packed_noise(sw, sh, C, 3))
        assert rc == 0 and geom[:3] == [CT, TH, NP], (shape, C, geom)
        nTx = geom[3]
        if dw > CT and dw % CT and dw % 4:
            assert nTx >= 2
            cts.add(CT)
            both_borders |= bool(geom[4] and geom[5])
        if dh > TH and dh % TH:
            ths.add(TH)
        odd_bytes |= (sw * C) % 8 != 0
    assert cts == {64, 128, 256, 512} and ths == {2, 4, 8, 16}
    assert odd_bytes and both_borders
    # the wide Lanczos upscales: CT = 512 at C = 2, CT = 256 at C = 4, upscaling by more than 2
    assert {(C, CT) for _, C, CT, _, _ in pc.LANCZOS_WIDE_UPSCALES} == {(2, 512), (4, 256)}
    assert all(s[0][4] > 2 * s[0][2] and s[0][4] > s[2] and s[0][4] % 4 for s in pc.LANCZOS_WIDE_UPSCALES)


@pytest.mark.parametrize("row", MATRIX, ids=pc.cell_id)
def test_matrix_rows_match_their_literals_and_the_oracle(emul, row):
    import libiqo_amd
    shape, C, CT, TH, NP = row
    m, d, sw, sh, dw, dh, px = shape
    assert libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px) == "packed_tile"
    frames = list(pc.frames_for(shape, C)) + [pc.const_frame(shape, C)]
    exp = list(pc.expected_for(shape, C)) + [pc.oracle_packed(shape, frames[2])]
    if row not in pc.LANCZOS_WIDE_UPSCALES:  # (the GPU tests assert these constants of the kernel's output)
        assert (exp[2] == np.array(pc.CONST_CHANNELS[:C], np.uint8)).all(), "the reference does not keep the constants"
    for f, e in zip(frames, exp):
        rc, out, geom = run_emul(emul, shape, C, f, dst_pad=5)
        assert rc == 0 and geom[:3] == [CT, TH, NP], (pc.cell_id(row), rc, geom)
        assert (out[:, dw * C:] == 0xA5).all()
        bad = np.argwhere(out[:, :dw * C].reshape(dh, dw, C) != e)
        assert bad.size == 0, (pc.cell_id(row), bad[:4].tolist())


@pytest.mark.parametrize("shape", pc.REJECTED, ids=pc.sid)
def test_rejected_lanczos_shapes_raise(emul, shape):
    """The top border rows exceed dstH: no plan, from any constructor or host query (the calls fail
    on the host, before any device is looked at)."""
    import libiqo_amd
    m, d, sw, sh, dw, dh, px = shape
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, px)
    for C in (1, 2, 3, 4):
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_packed_kernel_for(m, d, C, sw, sh, dw, dh, px)
    L = libiqo_amd.lib()
    plan = ctypes.c_void_p()
    assert L.iqo_hip_plan_lanczos(d, sw, sh, dw, dh, px, 0, ctypes.byref(plan)) == -1 and not plan  # IQO_HIP_EINVAL
    for C in (1, 3):
        assert L.iqo_hip_plan_packed(0, d, C, sw, sh, dw, dh, px, 0, ctypes.byref(plan)) == -1 and not plan
    if px == 1:  # the Y plane of a 4:2:0 / NV12 frame of this size
        assert L.iqo_hip_plan_yuv420(0, d, sw, sh, dw, dh, 0, ctypes.byref(plan)) == -1 and not plan
        assert L.iqo_hip_plan_nv12(0, d, sw, sh, dw, dh, 0, ctypes.byref(plan)) == -1 and not plan
    else:        # ... and the chroma planes (pxScale 2) of a frame twice this size
        assert L.iqo_hip_plan_nv12(0, d, 2 * sw, 2 * sh, 2 * dw, 2 * dh, 0, ctypes.byref(plan)) == -1 and not plan
    img = pc.packed_noise(sw, sh, 3, 1)
    assert run_emul(emul, shape, 3, img)[0] == -1
    # the same sizes with rows to spare are accepted
    assert libiqo_amd.host_kernel_for(m, d, sw, 4 * sh, dw, 4 * dh, px)
