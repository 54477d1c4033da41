"""Crop-and-resize regimes (tests/roi_regime_cases.py), the part that needs no GPU: the CPU twin equals the Generic
oracle on every case of tables A-D; the reference's own build agrees where it runs the shape clean; and the PROOFS
that the tables are in the regimes they name -- rows per workgroup and remainder bands (through
iqo_host_roi_box_layout), the arena above its first allocation, the search depth, and the oracle's stage statistics
on the extreme frames against their noise control.
"""
import numpy as np
import pytest

import libiqo_amd
import oracle_lib as ol
import roi_cases
import roi_regime_cases as rr

EUNSUP = -5


def _same(got, exp, what):
    assert got.shape == exp.shape and got.dtype == exp.dtype, (what, got.shape, exp.shape, got.dtype, exp.dtype)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, "%s: %d elements differ, first at %s: got %s want %s" % (
        what, len(bad), bad[0].tolist(), got[tuple(bad[0])], exp[tuple(bad[0])])


def _check_reference(case, C):
    """The reference's own result == the oracle on the boxes its sanitizer build runs clean (roi_cases._ref_clean's
    rule, at this case's output size).  The strict-IEEE build, as tests/test_packed_host.py: the product and the oracle
    build their tables strict-IEEE, and where the reference's -Ofast build rounds a table entry differently (Linear
    31 -> 21 rows is such a shape) the strict answer is the pinned one.  Returns the boxes compared."""
    n = 0
    for b in case.boxes:
        w, h = b[3:5]
        if not roi_cases._ref_clean(case.method, case.degree, w, h, case.dw, case.dh):
            continue
        for c in range(C):
            ref = ol.run_ref(case.method, case.degree, w, h, case.dw, case.dh, 1, rr.crop(case, C, b, c), strict=True)
            assert np.array_equal(rr.oracle_plane(case, C, b, c), ref), (rr.cid(case), c, b)
        n += 1
    return n


def _twin_equals_oracle(case, channels, reference=True):
    for C in channels:
        assert len(case.boxes) >= 1
        _same(rr.twin(case, C), rr.expected(case, C), "%s C=%d" % (rr.cid(case), C))
    if reference and ol.ref_available():
        _check_reference(case, min(channels))


# ----------------------------------------------------------------------------- twin == oracle

@pytest.mark.parametrize("case", rr.TABLE_A, ids=rr.cid)
def test_sizes_bands_degrees(case):
    _twin_equals_oracle(case, rr.CHANNELS)


def test_table_a_sizes_degrees_and_refusals():
    by = {(c.method, c.degree, c.dw, c.dh): c for c in rr.TABLE_A}
    sizes = {(1, 1), (5, 3), (7, 9), (32, 20), (33, 21), (56, 52)}
    assert {(c.dw, c.dh) for c in rr.TABLE_A} == sizes
    for m in ("area", "linear"):
        assert {(dw, dh) for (mm, _, dw, dh) in by if mm == m} == sizes
    for deg in (1, 3, 4, 6, 9):
        for size in ((32, 20), (33, 21)):
            assert len(by[("lanczos", deg) + size].boxes) >= 4, (deg, size)
    assert len(by[("lanczos", 1, 5, 3)].boxes) == 6 and len(by[("lanczos", 3, 7, 9)].boxes) == 5
    assert len(by[("area", 0, 33, 21)].boxes) == 6
    for c in rr.TABLE_A:
        assert c.boxes, rr.cid(c)
        # what the table leaves out is refused by the library (over the tap cap), undefined, or above Linear's 2x
        for b in rr.A_BOXES:
            if b in c.boxes or c.method != "lanczos" or not ol.lanczos_rows_defined(c.degree, b[4], c.dh):
                continue
            with pytest.raises(libiqo_amd.IqoError) as e:
                rr.layout(c, 1, b)
            assert e.value.status == EUNSUP
    # refused examples: 2000 -> 64 and 123 -> 5 columns at Lanczos-3 (188 and 148 taps), 96 -> 9 rows at Lanczos-9
    # (192); 48 -> 9 rows at Lanczos-9 is 96 taps and accepted
    for deg, w, h, dw, dh in ((3, 2000, 8, 64, 8), (3, 123, 8, 5, 8), (9, 8, 96, 8, 9)):
        assert max(ol.lanczos_taps(deg, w, dw), ol.lanczos_taps(deg, h, dh)) > libiqo_amd.ROI_MAX_TAPS
        with pytest.raises(libiqo_amd.IqoError) as e:
            libiqo_amd.host_roi_box_layout("lanczos", deg, 1, dw, dh, w, h)
        assert e.value.status == EUNSUP, (deg, w, h, dw, dh)
    assert ol.lanczos_taps(9, 48, 9) == 96
    assert libiqo_amd.host_roi_box_layout("lanczos", 9, 1, 8, 9, 8, 48)["nYp"] == 96
    # remainder bands: 9 = 8 + 1, 20 = 8 + 8 + 4, 21 = 8 + 8 + 5, and flips at an odd width
    for size, groups in (((7, 9), 2), ((32, 20), 3), ((33, 21), 3), ((56, 52), 7), ((5, 3), 1), ((1, 1), 1)):
        c = by[("area", 0) + size]
        for b in c.boxes:
            lay = rr.layout(c, 4, b)
            assert lay["rows"] == min(8, size[1]) and lay["workgroups"] == groups
    assert any(rr.flipped(b) for b in by[("lanczos", 3, 33, 21)].boxes)


@pytest.mark.parametrize("case", rr.TABLE_B, ids=rr.cid)
def test_wide_boxes(case):
    _twin_equals_oracle(case, rr.CHANNELS, reference=False)


@pytest.mark.parametrize("method,degree", rr.WIDEST, ids=["lanczos3", "area"])
def test_widest_box(method, degree):
    case = rr.widest_case(method, degree)
    w = case.boxes[0][3]
    lay = rr.layout(case, 4, case.boxes[0])
    assert lay["rows"] == 1 and lay["workgroups"] == case.dh
    # (pitchDw is odd: one step of it is 2 dwords x 4 channels)
    assert libiqo_amd.ROI_LDS_BYTES - 32 < lay["lds_bytes"] <= libiqo_amd.ROI_LDS_BYTES
    with pytest.raises(libiqo_amd.IqoError) as e:
        libiqo_amd.host_roi_box_layout(method, degree, 4, case.dw, case.dh, w + 1, 8)
    assert e.value.status == EUNSUP
    assert w <= (8 if method == "lanczos" else 16) * case.dw
    print("widest %s-%d box at C = 4: %d columns, %s" % (method, degree, w, lay))
    _twin_equals_oracle(case, (4,), reference=False)


def test_wide_boxes_reach_every_rows_value():
    """Table B through the layout query: every rows value 1, 2, 8, at least two of 3..7, and a remainder band
    below a band height under 8."""
    seen, remainder = {}, []
    for case in rr.TABLE_B:
        for C in rr.CHANNELS:
            for b in case.boxes:
                lay = rr.layout(case, C, b)
                st = libiqo_amd.host_roi_arena_stats(case.method, case.degree, case.dw, case.dh, C, [b], 1,
                                                     rr.frames(case.fid, C).shape[2], rr.B_H)
                assert (lay["workgroups"], lay["lds_bytes"]) == (st["workgroups"], st["lds_bytes"])
                assert lay["workgroups"] == -(-case.dh // lay["rows"])
                assert lay["lds_bytes"] == lay["rows"] * (C * lay["pitchDw"] * 4 + lay["nYp"] * 8)
                seen.setdefault(lay["rows"], []).append((rr.cid(case), C, b[3]))
                if lay["rows"] < 8 and case.dh % lay["rows"]:
                    remainder.append((rr.cid(case), C, b[3], lay["rows"]))
                print("%-28s C=%d w=%4d rows=%d workgroups=%2d lds=%5d nYp=%d NP=%d pitchDw=%d" % (
                    rr.cid(case), C, b[3], lay["rows"], lay["workgroups"], lay["lds_bytes"], lay["nYp"], lay["NP"],
                    lay["pitchDw"]))
    assert {1, 2, 8} <= set(seen), sorted(seen)
    assert len(set(seen) & {3, 4, 5, 6, 7}) >= 2, sorted(seen)
    assert remainder, "no case with dstH % rows != 0 and rows < 8"
    # the narrow box of a Lanczos batch runs 8 rows inside the wide box's allocation
    for case in rr.TABLE_B[:4]:
        wide, narrow = (rr.layout(case, 4, b) for b in case.boxes)
        both = libiqo_amd.host_roi_arena_stats(case.method, case.degree, case.dw, case.dh, 4, case.boxes, 1, rr.B_W, rr.B_H)
        assert narrow["rows"] == 8 and wide["rows"] < 8
        assert narrow["lds_bytes"] < wide["lds_bytes"] == both["lds_bytes"]  # the launch's LDS is the wide box's


@pytest.mark.parametrize("case", rr.TABLE_C + [rr.C_AREA], ids=rr.cid)
def test_box_counts(case):
    C = 3 if case is rr.C_AREA else 1
    _twin_equals_oracle(case, (C,))


def test_box_counts_reach_the_search_and_the_arena():
    assert [len(c.boxes) for c in rr.TABLE_C] == list(rr.C_COUNTS) and len(rr.C_AREA.boxes) == 4097
    # three workgroups per box: a box's first workgroup is not its index
    for b in rr.TABLE_C[-1].boxes[:6]:
        assert rr.layout(rr.TABLE_C[-1], 1, b)["workgroups"] == 3
    assert {b[3:5] for b in rr.TABLE_C[-1].boxes} == set(rr.C_SHAPES)
    assert sum(rr.flipped(b) for b in rr.TABLE_C[-1].boxes) == 4097 // 5
    assert {b[0] for b in rr.TABLE_C[-1].boxes} == {0, 1, 2}
    # the kernel's recurrence: n boxes, 64 lanes `step` apart, the survivor's remainder min(step, n - k step)
    depth = {n: rr.search_rounds(n) for n in rr.C_COUNTS}
    assert depth == {1: 0, 2: 1, 63: 1, 64: 1, 65: 2, 4096: 2, 4097: 3}
    assert rr.search_rounds(4097) >= 3
    # the largest arenas are above the plan's first allocation of 2^16 words, the others far below it
    for case, C in [(c, 1) for c in rr.TABLE_C] + [(rr.C_AREA, 3)]:
        st = libiqo_amd.host_roi_arena_stats(case.method, case.degree, case.dw, case.dh, C, case.boxes, rr.C_FRAMES,
                                             rr.C_W, rr.C_H)
        assert st["workgroups"] == 3 * len(case.boxes)
        assert (st["arena_bytes"] > 4 << 16) == (len(case.boxes) >= 4096), (len(case.boxes), st)
        print("%-28s arena %d bytes, %d workgroups" % (rr.cid(case), st["arena_bytes"], st["workgroups"]))
    assert {n: n >= 4096 for n in rr.C_QUEUE + rr.C_REGROW} == {2: False, 65: False, 4096: True, 4097: True}
    # C_REGROW gives each of the plan's two arenas (used alternately) a small batch first and a large one after
    big = [n >= 4096 for n in rr.C_REGROW]
    assert big[:4] == [False, False, True, True]


@pytest.mark.parametrize("case", rr.TABLE_D + rr.TABLE_E, ids=rr.cid)
def test_extreme_frames(case):
    _twin_equals_oracle(case, rr.CHANNELS)
    if case.fid[0] == "D" and ol.ref_available():  # the first four shapes are there because the reference runs them
        clean = roi_cases._ref_clean(case.method, case.degree, case.fid[2], case.fid[3], case.dw, case.dh)
        assert clean or case not in rr.TABLE_D[:4], rr.cid(case)


def test_extreme_frames_reach_every_regime():
    """The oracle's stage statistics over the crops of table D: every regime roi_kernel has code of its own for is
    reached, and by the extreme frames more often than by the noise control (frame 0 of every set)."""
    noise = dict.fromkeys(rr.D_COUNTERS, 0)
    extreme = dict.fromkeys(rr.D_COUNTERS, 0)
    for case in rr.TABLE_D:
        src = rr.frames(case.fid, 1)
        per = [dict.fromkeys(rr.D_COUNTERS, 0), dict.fromkeys(rr.D_COUNTERS, 0)]
        for i, b in enumerate(case.boxes):
            f, x, y, w, h = b[:5]
            out, st = ol.run_oracle_stats("lanczos", case.degree, w, h, case.dw, case.dh, 1, src[f, y:y + h, x:x + w])
            exp = rr.expected(case, 1, [b])[0]
            assert np.array_equal(out[:, ::-1] if rr.flipped(b) else out, exp)
            assert st["xb_deno_neg"] == 0  # no pxScale here: negative X denominators cannot occur
            for k in rr.D_COUNTERS:
                per[i > 0][k] += st[k]
        for k in rr.D_COUNTERS:
            noise[k] += per[0][k]
            extreme[k] += per[1][k]
        print("%-34s %s" % (rr.cid(case), " ".join("%s %d/%d" % (k, per[0][k], per[1][k]) for k in rr.D_COUNTERS)))
    print("%-34s %s" % ("all (noise/extreme)", " ".join("%s %d/%d" % (k, noise[k], extreme[k]) for k in rr.D_COUNTERS)))
    for k in rr.D_COUNTERS:
        assert extreme[k] > 0, k
        assert extreme[k] > noise[k], (k, noise[k], extreme[k])


def test_flat_and_striped_frames_reach_the_unsigned_extremes():
    """Area at 16 and at 128 taps per axis: flat 255 gives 255 (the sum at its largest does not wrap), flat 0 gives 0,
    and period-1 stripes across an even window average to 127 or 128."""
    for case, taps in ((rr.TABLE_E[0], 16), (rr.TABLE_E[1], libiqo_amd.ROI_MAX_TAPS)):
        w, h = case.fid[1:]
        for axis, (s, d) in enumerate(((w, case.dw), (h, case.dh))):
            assert len(libiqo_amd.host_tables("area", 0, s, 4, d, 4, 1, 0)[0]) == taps, (s, d, axis)
        exp = rr.expected(case, 1)
        assert (exp[0] == 255).all() and (exp[1] == 0).all()
        assert set(np.unique(exp[2:])) <= {127, 128}


# ----------------------------------------------------------------------------- the layout query

def test_box_layout_agrees_with_arena_stats():
    """iqo_host_roi_box_layout on every box of every table == iqo_host_roi_arena_stats of the one-box call."""
    n = 0
    for case, channels in rr.all_cases():
        seen = set()
        for b in case.boxes:
            if b[3:5] in seen:
                continue
            seen.add(b[3:5])
            for C in channels:
                lay = rr.layout(case, C, b)
                st = libiqo_amd.host_roi_arena_stats(case.method, case.degree, case.dw, case.dh, C, [(0, 0, 0, b[3], b[4])],
                                                     1, b[3], b[4])
                assert (lay["workgroups"], lay["lds_bytes"]) == (st["workgroups"], st["lds_bytes"]), (rr.cid(case), C, b)
                assert 1 <= lay["rows"] <= 8 and lay["workgroups"] == -(-case.dh // lay["rows"])
                assert lay["lds_bytes"] == lay["rows"] * (C * lay["pitchDw"] * 4 + lay["nYp"] * 8)
                assert lay["nYp"] % 2 == 0 and lay["pitchDw"] % 2 == 1 and lay["NP"] >= 1
                n += 1
    assert n > 200


def test_box_layout_rejections_and_surface():
    for name in ("host_roi_box_layout", "RoiBoxLayout"):
        assert name in libiqo_amd.__all__
    L = libiqo_amd.lib()
    out = libiqo_amd.RoiBoxLayout()
    assert L.iqo_host_roi_box_layout(1, 0, 1, 8, 8, 16, 16, None) == -1
    assert L.iqo_host_roi_box_layout(3, 0, 1, 8, 8, 16, 16, out) == -1
    assert L.iqo_host_roi_box_layout(1, 0, 1, 8, 8, 0, 16, out) == -1
    assert L.iqo_host_roi_box_layout(1, 0, 2, 8, 8, 16, 16, out) == EUNSUP
    assert L.iqo_host_roi_box_layout(0, 3, 1, 8, 24, 10, 1, out) == -1      # undefined Lanczos rows
    assert L.iqo_host_roi_box_layout(1, 0, 4, 4500, 2, 9000, 2, out) == EUNSUP  # one work row above the LDS
    with pytest.raises(libiqo_amd.IqoError) as e:  # the wrapper names no box index
        libiqo_amd.host_roi_box_layout("area", 0, 1, 8, 8, 0, 16)
    assert (e.value.status, e.value.bad_roi) == (-1, -1) and "box 0 x 16" in str(e.value)
    # the corner tests/roi_cases.py lives in: 8 rows, 3 workgroups
    lay = libiqo_amd.host_roi_box_layout("lanczos", 3, 3, roi_cases.DW, roi_cases.DH, 64, 48)
    assert (lay["rows"], lay["workgroups"]) == (8, 3)
