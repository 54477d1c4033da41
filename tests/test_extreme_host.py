"""Extreme inputs, the part that needs no GPU (tests/extreme_cases.py builds the frames).

For every case the oracle's stage statistics (iqo_oracle_run_stats) must show that the frame set reaches
every regime the shape can reach: both clamps of both passes, the analytic extreme of each pass, negative
border numerators, both numerator signs over negative denominators, and -- for the cases marked so --
border quotients that wrap int16.  "Can reach" comes from the statistics themselves (a shape without
border columns has no border numerators), never from a typed-in list.

The same frames go through the CPU emulations of the kernels' arithmetic (tests/native/ratio_emul.cpp,
tile_emul.cpp, packed_emul.cpp) and must equal the oracle bit for bit; and the oracle is pinned on them to
the reference's own Generic code by the hashes of tests/golden/extreme.json (oracle/gen_golden.py
--extreme), and directly where oracle/_ref is built.
"""
import ctypes
import json
import os
import subprocess

import numpy as np
import pytest

import extreme_cases as ec
import oracle_lib as ol

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "libiqo_amd", "csrc")
# tests/native/ratio_emul.cpp kinds that take Lanczos tables
RATIO_KINDS = {"lanczos_d32": 0, "lanczos_up2": 1, "lanczos_u23": 3, "lanczos_d31": 5, "ryx": 6, "ryg": 9, "ryu": 10,
               "ryu_run": 11}


def _build(name):
    """tests/native/<name>.cpp + plan.cpp as a shared library, the way test_ratio_tables.py and its siblings do."""
    out = os.path.join(HERE, "native", "_build")
    os.makedirs(out, exist_ok=True)
    so = os.path.join(out, "lib%s.so" % name)
    srcs = [os.path.join(HERE, "native", name + ".cpp"), os.path.join(CSRC, "plan.cpp")]
    deps = srcs + [os.path.join(CSRC, "plan.hpp")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in deps):
        tmp = "%s.%d.tmp" % (so, os.getpid())  # private name + rename: xdist workers may rebuild together
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", "-I" + CSRC,
                               "-o", tmp] + srcs)
        os.replace(tmp, so)
    return ctypes.CDLL(so)


@pytest.fixture(scope="module")
def ratio_emul():
    lib = _build("ratio_emul")
    lib.ratio_emul.restype = ctypes.c_int
    lib.ratio_emul.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.c_void_p] * 2
    return lib


@pytest.fixture(scope="module")
def tile_emul():
    lib = _build("tile_emul")
    lib.tile_emul.restype = ctypes.c_int
    lib.tile_emul.argtypes = [ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 5 + [ctypes.c_void_p, ctypes.c_void_p,
                                                                                  ctypes.POINTER(ctypes.c_int)]
    return lib


@pytest.fixture(scope="module")
def packed_emul():
    lib = _build("packed_emul")
    lib.packed_emul.restype = ctypes.c_int
    lib.packed_emul.argtypes = ([ctypes.c_int, ctypes.c_uint] + [ctypes.c_int] * 6 +
                                [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int,
                                 ctypes.POINTER(ctypes.c_int)])
    return lib


@pytest.fixture(scope="module")
def extreme_golden():
    with open(os.path.join(HERE, "golden", "extreme.json")) as f:
        doc = json.load(f)
    by_case = {}
    for e in doc["entries"]:
        by_case.setdefault(e["case"], {})[e["frame"]] = e
    return by_case


# ----------------------------------------------------------------------------- the case table itself

def test_case_table_is_well_formed():
    import libiqo_amd
    ids = [ec.cid(c) for c in ec.PLANAR]
    assert len(set(ids)) == len(ids)
    for c in ec.PLANAR:
        assert ol.lanczos_rows_defined(c.d, c.sh, c.dh, c.px), c
        assert libiqo_amd.host_kernel_for("lanczos", c.d, c.sw, c.sh, c.dw, c.dh, c.px) == c.kernel, c
        assert max(c.sw, c.dw) <= 1024
    for k, d, sw, sh, dw, dh, C, _ in ec.PACKED:
        assert ol.lanczos_rows_defined(d, sh, dh, 1)
        assert libiqo_amd.host_packed_kernel_for("lanczos", d, C, sw, sh, dw, dh, 1) == k
    for case in ec.FUSED:
        m, d, sw, sh, dw, dh, label = case
        assert ol.lanczos_rows_defined(d, sh, dh, 1) and ol.lanczos_rows_defined(d, sh // 2, dh // 2, 2)
        assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == label
    import yuv_cases
    assert {c[6] for c in ec.FUSED} == {c[6] for c in yuv_cases.CASES if c[0] == "lanczos" and c[6] != "none"}
    assert all(c in yuv_cases.CASES for c in ec.FUSED)
    # every Lanczos kernel family the plans pick has a case
    assert {c.kernel for c in ec.PLANAR} == {"lanczos_stream", "lanczos_up2", "lanczos_d32", "lanczos_d31",
                                             "lanczos_u23", "ryx", "ryg", "walk", "tile", "general"}


# ----------------------------------------------------------------------------- regimes

def analytic_extremes(c):
    """(largest Y-main work value, largest interior X-main sum) any frame can produce with the rows of an
    output column's window all at their own extreme: 255 * sum(positive Y taps), times sum(positive X taps),
    over the interior rows and columns.  int64 numpy, from the oracle's tables."""
    out = []
    for axis, (s, t) in ((1, (c.sh, c.dh)), (0, (c.sw, c.dw))):
        tab = ol.oracle_tables("lanczos", c.d, c.sw, c.sh, c.dw, c.dh, c.px, axis).astype(np.int64)
        _, phase, mb, me = ec.axis_geometry(tab, s, t)
        pos = np.where(tab > 0, tab, 0).sum(axis=1)
        out.append(int(pos[phase[mb:me]].max()) if me > mb else None)
    y, x = out
    return (None if y is None else 255 * y), (None if y is None or x is None else 255 * y * x)


def regime_misses(c, total, noise):
    """The regimes the frame set's summed statistics `total` do not reach although the shape can."""
    miss = []

    def need(cond, what):
        if not cond:
            miss.append(what)

    ymax, xmax = analytic_extremes(c)
    if total["ym_n"]:
        need(total["ym_neg"] > 0, "Y main below 0")
        need(total["ym_hi"] > 0, "Y main above 255*64")
        need(total["ym_max"] == ymax, "Y main extreme %s != %s" % (total["ym_max"], ymax))
    if total["xm_n"]:
        need(total["xm_neg"] > 0, "X main below 0")
        need(total["xm_hi"] > 0, "X main above 255")
        if xmax is not None:
            need(total["xmi_max"] == xmax, "X main extreme %s != %s" % (total["xmi_max"], xmax))
    if total["yb_n"]:
        need(total["yb_nume_neg"] > 0, "Y border numerator below 0")
        need(total["yb_q_neg"] > 0, "Y border quotient below 0")
        need(total["yb_q_hi"] > 0, "Y border quotient above 255*64")
    if total["xb_n"]:
        need(total["xb_nume_neg"] > 0, "X border numerator below 0")
        need(total["xb_q_lo"] > 0, "X border clamp at 0")
        need(total["xb_q_hi"] > 0, "X border clamp at 255")
    if total["yb_deno_neg"]:
        need(total["yb_dneg_nume_neg"] > 0, "Y border: negative numerator over a negative denominator")
        need(total["yb_dneg_nume_pos"] > 0, "Y border: positive numerator over a negative denominator")
    if total["xb_deno_neg"]:
        need(total["xb_dneg_nume_neg"] > 0, "X border: negative numerator over a negative denominator")
        need(total["xb_dneg_nume_pos"] > 0, "X border: positive numerator over a negative denominator")
    if c.wrap:
        need(total["yb_q_wrap"] + total["xb_q_wrap"] > 0, "border quotient wraps int16")
    need((noise["yb_deno_zero_rows"] > 0) == c.trap, "the case table's `trap` column is wrong")
    return miss


def sum_stats(stats):
    out = {}
    for k in ol.STATS_FIELDS:
        v = [s[k] for s in stats]
        out[k] = min(v) if k.endswith("_min") else max(v) if k.endswith("_max") else sum(v)
    return out


COLUMNS = ("ym_neg ym_hi yb_nume_neg yb_deno_neg yb_q_wrap xm_neg xm_hi xb_nume_neg xb_deno_neg xb_q_lo xb_q_hi "
           "xb_q_wrap").split()


@pytest.mark.parametrize("c", ec.PLANAR + ec.other_planes(), ids=ec.cid)
def test_frames_reach_every_regime(c):
    names, frames = ec.frames_of(c)
    exp = ec.expected_of(c)
    stats = []
    for f in range(frames.shape[0]):
        out, st = ol.run_oracle_stats("lanczos", c.d, c.sw, c.sh, c.dw, c.dh, c.px, frames[f])
        assert np.array_equal(out, exp[f]), (names[f], "iqo_oracle_run_stats and iqo_oracle_run differ")
        stats.append(st)
    total = sum_stats(stats)
    print("%-42s %-7s %s" % (ec.cid(c), "", " ".join("%11s" % k for k in COLUMNS)))  # DESIGN.md "Extreme inputs"
    for label, st in (("noise", stats[0]), ("extreme", sum_stats(stats[1:]))):
        print("%-42s %-7s %s" % (ec.cid(c), label, " ".join("%11d" % st[k] for k in COLUMNS)))
    assert regime_misses(c, total, stats[0]) == []


def test_noise_alone_misses_the_regimes():
    """The control: on the headline downscale shapes the noise frame never clamps an interior pixel at 0 or
    255 and never divides a negative border numerator -- what the extreme frames are for."""
    for c in ec.PLANAR[:3]:
        _, frames = ec.frames_of(c)
        _, st = ol.run_oracle_stats("lanczos", c.d, c.sw, c.sh, c.dw, c.dh, c.px, frames[0])
        assert st["xm_neg"] == 0 and st["xb_nume_neg"] == 0, (c, st)
        assert regime_misses(c, st, st) != []


# ----------------------------------------------------------------------------- emulations

@pytest.mark.parametrize("c", ec.PLANAR, ids=ec.cid)
def test_emulations_match_oracle(c, ratio_emul, tile_emul):
    names, frames = ec.frames_of(c)
    exp = ec.expected_of(c)
    covered = set()
    for f in range(frames.shape[0]):
        src = np.ascontiguousarray(frames[f])
        for kind, code in RATIO_KINDS.items():
            dst = np.zeros((c.dh, c.dw), np.uint8)
            rc = ratio_emul.ratio_emul(code, 0, c.d, c.sw, c.sh, c.dw, c.dh, c.px, src.ctypes.data, dst.ctypes.data)
            assert rc in (0, 1), (kind, rc)
            if rc == 0:
                covered.add(kind)
                bad = np.argwhere(dst != exp[f])
                assert bad.size == 0, (kind, names[f], bad[:4].tolist(), dst[tuple(bad[0])], exp[f][tuple(bad[0])])
        dst = np.zeros((c.dh, c.dw), np.uint8)
        n_pairs = ctypes.c_int(0)
        rc = tile_emul.tile_emul(0, c.d, c.sw, c.sh, c.dw, c.dh, c.px, src.ctypes.data, dst.ctypes.data,
                                 ctypes.byref(n_pairs))
        assert rc == (0 if c.tile else 1), ("tile tables", rc, "the case table's `tile` column is wrong")
        if rc == 0:
            covered.add("tile")
            bad = np.argwhere(dst != exp[f])
            assert bad.size == 0, ("tile", names[f], bad[:4].tolist(), dst[tuple(bad[0])], exp[f][tuple(bad[0])])
    if c.kernel in RATIO_KINDS or c.kernel == "tile":
        assert c.kernel in covered, (c.kernel, sorted(covered))


@pytest.mark.parametrize("row", [r for r in ec.PACKED if r[0] == "packed_tile"], ids=lambda r: "L%d-%dx%d-C%d" % (r[1], r[2], r[3], r[6]))
def test_packed_emulation_matches_oracle(row, packed_emul):
    _, d, sw, sh, dw, dh, C, _ = row
    src, exp = ec.packed_frames(d, sw, sh, dw, dh, C)
    for f in range(src.shape[0]):
        img = np.ascontiguousarray(src[f])
        dst = np.full((dh, dw * C + 3), 0xA5, np.uint8)
        geom = (ctypes.c_int * 6)()
        rc = packed_emul.packed_emul(0, d, C, sw, sh, dw, dh, 1, img.ctypes.data, sw * C, dst.ctypes.data,
                                     dst.shape[1], geom)
        assert rc == 0
        assert (dst[:, dw * C:] == 0xA5).all()
        bad = np.argwhere(dst[:, :dw * C].reshape(dh, dw, C) != exp[f])
        assert bad.size == 0, (f, bad[:4].tolist())


# ----------------------------------------------------------------------------- the oracle against the reference

@pytest.mark.parametrize("c", ec.PLANAR, ids=ec.cid)
def test_oracle_matches_reference_on_extreme_frames(c, extreme_golden):
    names, frames = ec.frames_of(c)
    exp = ec.expected_of(c)
    gold = extreme_golden[ec.cid(c)]
    assert sorted(gold) == sorted(names)
    for f, name in enumerate(names):
        g = gold[name]
        assert "%016x" % ol.fnv1a64(frames[f]) == g["in"], (name, "the frame builder changed: regenerate extreme.json")
        if c.trap:  # the reference divides by zero on this shape: nothing to compare, and it is never called
            assert g.get("ref_traps") is True and "fnv" not in g
            continue
        assert "ref_traps" not in g
        want = g["fnv"] if g["ofast_strict_agree"] else g["fnv_strict"]
        assert "%016x" % ol.fnv1a64(exp[f]) == want, name
        if ol.ref_available():
            ref = ol.run_ref("lanczos", c.d, c.sw, c.sh, c.dw, c.dh, c.px, frames[f], strict=True)
            bad = np.argwhere(ref != exp[f])
            assert bad.size == 0, (name, bad[:4].tolist(), exp[f][tuple(bad[0])], ref[tuple(bad[0])])
