"""The instantiation table of tests/instance_cases.py against the library's own account, without a GPU.

The library names the template instantiation a call runs (include/iqo_hip.h iqo_hip_instance): one table and one
lookup per kernel family serve the launch functions and the host queries alike.  Here: the table is complete
(every instantiation the library enumerates has a row or a reasoned UNREACHABLE entry, none twice), every row's
shape and options select exactly the row's instantiation, the host tables of every ratio-kernel row pass the
scalar emulation of the kernels' arithmetic at these tiny shapes, and every misuse of the new entry points is
rejected.  tests/test_instance_gpu.py then launches each row.
"""
import ctypes

import numpy as np
import pytest

import instance_cases as ic
import libiqo_amd
import packed_cases as pc
from test_ratio_tables import emul, run_emul  # noqa: F401  (the emulation's fixture)

EINVAL = -1  # IQO_HIP_EINVAL


def _enumerated(kernel):
    """Keys of the library's enumeration that belong to `kernel` (ryg and ryu share the ryg family)."""
    family = "ryg" if kernel == "ryu" else kernel
    return [ic.key_of(i["kernel"], {k: v for k, v in i.items() if k != "kernel"})
            for i in libiqo_amd.host_instances(family) if i["kernel"] == kernel]


def test_counts_are_the_documented_ones():
    """Literals: a new instantiation fails here until the table (and DESIGN.md) knows it."""
    assert {k: len(_enumerated(k)) for k in ic.COUNTS} == {
        "ryx": 37, "ryg": 60, "ryu": 30, "tile": 22, "walk": 60, "lanczos_up2": 4, "lanczos_d32": 5, "lanczos_d31": 5,
        "lanczos_u23": 2, "linear_u23": 2, "area_d32": 3}
    assert ic.COUNTS == {k: len(_enumerated(k)) for k in ic.COUNTS}
    assert sum(ic.COUNTS.values()) == 230
    assert sum(len(libiqo_amd.host_instances(f)) for f in ic.FAMILIES) == 230
    assert len(ic.INSTANTIATIONS) + len(ic.UNREACHABLE) == 230
    # the families with a single kernel have no table
    for name in ("general", "lanczos_stream", "area_int", "linear_up2", "packed_tile", "packed_general"):
        assert libiqo_amd.host_instances(name) == []
    assert libiqo_amd.lib().iqo_host_instance_count(99) == 0 and libiqo_amd.lib().iqo_host_instance_count(-1) == 0


@pytest.mark.parametrize("kernel", sorted(ic.COUNTS))
def test_table_is_complete(kernel):
    lib_keys = _enumerated(kernel)
    assert len(set(lib_keys)) == len(lib_keys), "the library's table names an instantiation twice"
    rows = [ic.key_of(r[0], r[1]) for r in ic.INSTANTIATIONS if r[0] == kernel]
    unreachable = [ic.key_of(u[0], u[1]) for u in ic.UNREACHABLE if u[0] == kernel]
    assert len(set(rows)) == len(rows), "two rows for one instantiation"
    assert len(set(unreachable)) == len(unreachable) and not set(rows) & set(unreachable)
    missing = set(lib_keys) - set(rows) - set(unreachable)
    unknown = (set(rows) | set(unreachable)) - set(lib_keys)
    assert not missing, "instantiations without a row: %s" % sorted(missing)
    assert not unknown, "rows for instantiations the library does not have: %s" % sorted(unknown)
    assert len(rows) + len(unreachable) == ic.COUNTS[kernel]


def test_unreachable_is_the_walker_only():
    assert len(ic.UNREACHABLE) <= 24
    for kernel, params, reason in ic.UNREACHABLE:
        assert kernel == "walk", "a %s entry is a failure of the search, not a finding" % kernel
        assert "plan.cpp:" in reason or "not found within the bounds" in reason
        # the 24 the first CPU search left open: non-Lanczos NP >= 4, non-Lanczos NP 3 / VY 6, Lanczos NP 1 / NV 2,
        # Lanczos NP 2 / VY 4 / NV 2
        lz, NP, VY, NV = params.get("LZ", 0), params["NP"], params["VY"], params["NV"]
        assert (not lz and (NP >= 4 or (NP, VY) == (3, 6))) or (lz and (NP, NV) == (1, 2)) or \
            (lz and (NP, VY, NV) == (2, 4, 2)), params
    for row in ic.EXTRA:
        assert row[0] in ic.EXACT_FAMILIES


@pytest.mark.parametrize("row", ic.ALL_ROWS, ids=ic.rid)
def test_row_selects_its_instantiation(row):
    kernel, params, method, degree, sw, sh, dw, dh, px, options = row
    assert ic.pinned_answer(method, degree, sw, sh, dw, dh, px), "no pinned answer for this shape"
    if kernel in ic.SEARCHED_KERNELS:  # the search bounds
        assert 16 <= sw <= 512 and 8 <= sh <= 160 and 16 <= dw <= 512 and 16 <= dh <= 320
    want = ic.instance_of(row)
    assert libiqo_amd.host_instance_for(method, degree, sw, sh, dw, dh, px, options) == want
    # ... and with no more than the alignment the family needs (the GPU test's padded layout)
    sa, da = ic.align_of(kernel)
    assert libiqo_amd.host_instance_for(method, degree, sw, sh, dw, dh, px, options, sa, da) == want
    # the family, as host_kernel_for names it, where the row needs no option to get there
    family = "ryg" if kernel == "ryu" else kernel
    if all(k in ("ryg_cpt", "ryx_split", "ryx_adj", "ryx_uc", "ryx_cpt", "ryu", "ryu_run", "ratio_prefetch") for k, _ in options):
        assert libiqo_amd.host_kernel_for(method, degree, sw, sh, dw, dh, px) == family


def _emul_kind(row):
    kernel, params = row[0], row[1]
    if kernel == "ryu":
        return "ryu_run" if params.get("RUN") else "ryu"
    return kernel if kernel in ("ryx", "ryg") or kernel in ic.EXACT_FAMILIES else None


@pytest.mark.parametrize("row", [r for r in ic.ALL_ROWS if _emul_kind(r)], ids=ic.rid)
def test_host_tables_pass_the_emulation(emul, row):  # noqa: F811
    """tests/native/ratio_emul.cpp builds the kernel's host tables itself (plan.cpp) and runs the kernel's
    arithmetic as scalars: equal to the oracle on every frame the GPU test will use."""
    kernel, params, method, degree, sw, sh, dw, dh, px, options = row
    names, frames = ic.frames_of(row)
    exp = ic.expected_of(row)
    for i, name in enumerate(names):
        rc, out = run_emul(emul, _emul_kind(row), method, degree, sw, sh, dw, dh, px, frames[i])
        assert rc == 0, (ic.rid(row), "the emulation has no tables for this shape", rc)
        bad = np.argwhere(out != exp[i])
        assert bad.size == 0, (ic.rid(row), name, bad[:4].tolist())


def test_rejected_uses():
    L = libiqo_amd.lib()
    d = libiqo_amd.Instance()
    ok = (0, 3, 40, 24, 27, 17, 1)
    assert L.iqo_host_instance_for(*ok, None, 0, 16, 16, ctypes.byref(d)) == 0
    # null descriptor, null plan, null option array with a count
    assert L.iqo_host_instance_for(*ok, None, 0, 16, 16, None) == EINVAL
    assert L.iqo_host_instance_for(*ok, None, 1, 16, 16, ctypes.byref(d)) == EINVAL
    assert L.iqo_hip_plan_instance(None, 16, 16, ctypes.byref(d)) == EINVAL
    assert L.iqo_host_instance_at(12, 0, None) == EINVAL
    # an alignment that is no power of two in 1 .. 16; an unknown method
    for sa, da in ((3, 16), (16, 0), (32, 16)):
        assert L.iqo_host_instance_for(*ok, None, 0, sa, da, ctypes.byref(d)) == EINVAL
    assert L.iqo_host_instance_for(3, *ok[1:], None, 0, 16, 16, ctypes.byref(d)) == EINVAL
    # an index past the count, a negative one, a family without a table
    n = L.iqo_host_instance_count(12)
    assert n == 37 and L.iqo_host_instance_at(12, n - 1, ctypes.byref(d)) == 0
    assert L.iqo_host_instance_at(12, n, ctypes.byref(d)) == EINVAL
    assert L.iqo_host_instance_at(12, -1, ctypes.byref(d)) == EINVAL
    assert L.iqo_host_instance_at(0, 0, ctypes.byref(d)) == EINVAL
    # unknown option key, values outside an option's range (ryg_cpt: 0, 2, 3, 4)
    for options in ([("no_such_option", 1)], [("ryg_cpt", 1)], [("ryg_cpt", 5)], [("ryx_split", 5)], [("ryx_split", -1)],
                    [("ratio_prefetch", 9)], [("ryg_cpt", 3), ("bogus", 0)]):
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_instance_for("lanczos", 3, 40, 24, 27, 17, 1, options)
    # a Lanczos shape every plan constructor rejects
    for shape in pc.REJECTED:
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_instance_for(*shape)
    # a forced prefetch depth the family's kernel does not instantiate: rejected, not the default depth
    for kernel, method, degree, sw, sh, dw, dh, depth in ic.BAD_PREFETCH:
        assert libiqo_amd.host_instance_for(method, degree, sw, sh, dw, dh)["kernel"] == kernel
        with pytest.raises(libiqo_amd.IqoError):
            libiqo_amd.host_instance_for(method, degree, sw, sh, dw, dh, 1, [("ratio_prefetch", depth)])


def test_single_kernel_families_report_the_family_alone():
    assert libiqo_amd.host_instance_for("lanczos", 3, 384, 216, 192, 108) == {"kernel": "lanczos_stream"}
    assert libiqo_amd.host_instance_for("lanczos", 3, 40, 24, 27, 17, 1, [("force_general", 1)]) == {"kernel": "general"}
