"""Fused I420 selection, no GPU: libiqo_amd.host_yuv420_fused (iqo_host_yuv420_fused) is the host
function the three fused launchers call, so the label it reports is the kernel a device call runs.
The case table (tests/yuv_cases.py) must reach every instantiation; tests/test_yuv_gpu.py runs it."""
import pytest

import libiqo_amd
import oracle_lib as ol
import yuv_cases as yc

FAST = {"lanczos": "lanczos_stream", "area": "area_int", "linear": "linear_up2"}


def test_label_table_is_the_librarys():
    assert yc.LABELS == [libiqo_amd.YUV420_FUSED[i] for i in range(len(libiqo_amd.YUV420_FUSED))]
    assert len(yc.LABELS) == 15 and yc.LABELS[0] == "none"


def test_census_every_instantiation_has_a_row():
    have = {c[6] for c in yc.CASES}
    assert have == set(yc.LABELS), sorted(set(yc.LABELS) - have)
    assert len(have - {"none"}) == 14
    assert sorted(c[6] for c in yc.one_per_label()) == sorted(yc.LABELS)
    assert len(set(yc.CASES)) == len(yc.CASES)
    assert all(16 <= c[3] <= 64 for c in yc.CASES if c[6] != "none" and c[0] != "linear")  # cheap oracle rows


@pytest.mark.parametrize("case", yc.CASES, ids=yc.cid)
def test_row_label_is_the_selection(case):
    m, d, sw, sh, dw, dh, label = case
    assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == label
    # the oracle must have an answer for every plane of every row
    cw, ch, cdw, cdh, px = yc.chroma_shape(case)
    if m == "lanczos":
        assert ol.lanczos_rows_defined(d, sh, dh, 1) and ol.lanczos_rows_defined(d, ch, cdh, px)
    if label == "none":
        return
    # a fused row: the same fast family on Y and on chroma
    ky = libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, 1)
    kc = libiqo_amd.host_kernel_for(m, d, cw, ch, cdw, cdh, px)
    want = "area_int" if label == "lin_d2" else FAST[m]
    assert ky == kc == want, (ky, kc)


@pytest.mark.parametrize("cfg,label", [
    (("lanczos", 3, 3840, 2160, 1920, 1080), "lz_symb10"),   # BASELINE C2
    (("lanczos", 2, 640, 480, 320, 240), "lz_sym8"),         # C1
    (("area", 0, 7680, 4320, 1920, 1080), "area44"),         # C3
    (("linear", 0, 1920, 1080, 3840, 2160), "lin_up2"),      # C4
])
def test_baseline_shapes_are_pinned(cfg, label):
    assert libiqo_amd.host_yuv420_fused(*cfg) == label


@pytest.mark.parametrize("cfg", [
    ("lanczos", 3, 1, 48, 1, 24),        # a dimension < 2, each of the four
    ("lanczos", 3, 64, 1, 32, 1),
    ("area", 0, 64, 32, 1, 16),
    ("linear", 0, 64, 32, 128, 1),
    ("lanczos", 3, 0, 0, 0, 0),
    ("lanczos", 8, 115, 18, 16, 6),      # Lanczos rows without a defined answer (include/iqo_hip.h)
    ("lanczos", 16, 230, 36, 32, 12),    # ... on the chroma plane too (degree 16 / pxScale 2 at half size)
])
def test_invalid_requests_are_errors(cfg):
    m, d, sw, sh, dw, dh = cfg
    lib = libiqo_amd.lib()
    if m == "lanczos" and min(cfg[2:]) >= 2:
        assert not ol.lanczos_rows_defined(d, sh, dh, 1)
    rc = lib.iqo_host_yuv420_fused(libiqo_amd._METHODS[m], d, sw, sh, dw, dh)
    assert rc == -1, rc  # IQO_HIP_EINVAL, never a table index
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh)


def test_invalid_method_is_an_error():
    lib = libiqo_amd.lib()
    for method in (-1, 3, 99):
        assert lib.iqo_host_yuv420_fused(method, 3, 64, 32, 32, 16) == -1


def test_query_agrees_with_plane_queries_on_random_shapes():
    """A fused label needs the same fusable family on both planes; anything else is "none"."""
    import random
    rng = random.Random(11)
    n = 0
    for _ in range(400):
        m = rng.choice(["lanczos", "area", "linear"])
        d = rng.choice([2, 3, 4])
        dw, dh = 16 * rng.randint(1, 140), 2 * rng.randint(4, 40)
        rx, ry = rng.choice([(2, 2), (4, 4), (4, 2), (3, 3), (6, 2), (1, 1), (8, 4), (2, 6)])
        if m == "linear" and rng.random() < 0.5:
            sw, sh, dw, dh = dw, dh, 2 * dw, 2 * dh
        else:
            sw, sh = dw * rx, dh * ry
        if m == "lanczos" and not (ol.lanczos_rows_defined(d, sh, dh, 1) and ol.lanczos_rows_defined(d, sh // 2, dh // 2, 2)):
            continue
        label = libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh)
        assert label in yc.LABELS
        if label != "none":
            px = 2 if m == "lanczos" else 1
            ky = libiqo_amd.host_kernel_for(m, d, sw, sh, dw, dh, 1)
            kc = libiqo_amd.host_kernel_for(m, d, sw // 2, sh // 2, dw // 2, dh // 2, px)
            assert ky == kc and ky in ("lanczos_stream", "area_int", "linear_up2"), (m, d, sw, sh, dw, dh, label)
            assert label.startswith({"lanczos_stream": "lz_", "linear_up2": "lin_up2"}.get(ky, "area" if m == "area" else "lin_d2"))
            n += 1
    assert n > 50
