"""The address-range cases of tests/span_cases.py, without a GPU: every kernel family a 1-channel or packed plan
can report has a row, each row's shape reaches its family and body, the library's table of layout limits equals the
rows' literals, and every layout sits where it claims -- one 16-byte step on either side of a limit."""
import pytest

import libiqo_amd
import instance_cases as ic
import span_cases as sc

ROWS = pytest.mark.parametrize("row", sc.ROWS, ids=sc.rid)


def test_every_kernel_family_has_a_row():
    # (ryu_kernel: the ryg family's sub-kernel, a row of its own)
    assert {r.kernel for r in sc.ROWS} == set(libiqo_amd.KERNELS.values()) | {"ryu"}
    bodies = [(r.inst, sc.stream_body(r, r.frames)[1]) for r in sc.ROWS if r.kernel == "lanczos_stream"]
    assert sorted(bodies) == [("ring", 0), ("stack", 1), ("sym", 1), ("symb", 1), ("symb", 4)]
    assert sc.BY_NAME["stack-5frames"].frames == 5
    area = {r.name: r for r in sc.ROWS if r.kernel == "area_int"}
    assert area["area-2x2"].sw // area["area-2x2"].dw == 2 and area["area-3x3"].sw // area["area-3x3"].dw == 3
    assert area["linear-d2"].method == "linear"
    assert sorted(r.dw // r.sw for r in sc.ROWS if r.kernel == "linear_up2") == [2, 3]
    for k in ("packed_tile", "packed_general"):
        assert sorted(r.norm for r in sc.ROWS if r.kernel == k and r.C == 3) == [False, True]


@ROWS
def test_row_reaches_its_family_and_body(row):
    shape = (row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px)
    if row.C > 1:
        # (force_general is the one option of the packed rows; the host query has no options)
        want = "packed_general" if dict(row.options).get("force_general") else "packed_tile"
        assert libiqo_amd.host_packed_kernel_for(row.method, row.d, row.C, *shape[2:]) == "packed_tile"
        assert row.kernel == want
        return
    got = libiqo_amd.host_instance_for(*shape, options=row.options)
    if row.kernel == "lanczos_stream":
        assert libiqo_amd.host_kernel_for(*shape) == "lanczos_stream" and got == {"kernel": "lanczos_stream"}
        assert sc.stream_body(row, row.frames)[0] == row.inst
        assert sc.stream_body(row, 3)[0] == row.inst  # the `far` layout's 3 frames run the same body
    else:
        assert got == dict(row.inst or {}, kernel=row.kernel)


@ROWS
def test_limits_are_the_librarys_table(row):
    if row.norm:  # iqo_hip_resize_device_norm's documented limits: 2^31 for both frames, 2^24 for srcSt
        assert row.limits == (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 24 - 1, 2 ** 31 - 1)
        return
    family = "ryg" if row.kernel == "ryu" else row.kernel
    assert libiqo_amd.host_layout_limits(family) == row.limits


def test_no_sentinel_dropping_family_reaches_the_sentinel():
    assert libiqo_amd.DROP_OFFSET == sc.DROP == 0x7ff00000
    for k in libiqo_amd.KERNELS.values():
        m = libiqo_amd.host_layout_limits(k)
        if k in sc.SENTINEL_FAMILIES:
            assert 0 < m[0] < sc.DROP and 0 < m[1] < sc.DROP, k
            # sentinel + the largest row offset stays below 2^32: a dropped `sentinel + row offset` cannot wrap
            assert 2 * sc.DROP + 4096 < 2 ** 32
        elif k in ("tile", "packed_tile"):
            assert m[0] == m[1] == 2 ** 31 - 1, k
        else:
            assert m == (0, 0, 0, 0), k
    with pytest.raises(KeyError):
        libiqo_amd.host_layout_limits("nope")


@ROWS
def test_layouts_sit_one_step_either_side_of_the_limit(row):
    smax, dmax, sst_max, dst_max = row.limits
    sb, db = sc.row_bytes(row)
    t, s, d, f = sc.tight(row), sc.src_top(row), sc.dst_top(row), sc.far(row)
    for lay in (t, s, d, f):
        assert sc.accepted(row, lay) and sc.fits(row, lay), lay
        assert lay.src_st % 16 == 0 and lay.dst_st % 16 == 0 and lay.src_fst % 16 == 0 and lay.dst_fst % 16 == 0
        assert lay.src_st >= sb and lay.dst_st >= db
        # frames do not overlap: apart by a frame, or interleaved inside the row stride
        assert lay.dst_fst >= sc.norm_dst_rows(row) * lay.dst_st or lay.frames * lay.dst_fst <= lay.dst_st
    assert f.frames == 3 and f.src_fst > 2 ** 31 and 2 * f.src_fst > 2 ** 32 and f.dst_fst > 2 ** 31
    drows = sc.norm_dst_rows(row)
    if smax:
        # one more step of the top stride is rejected
        assert not sc.accepted(row, s._replace(src_st=s.src_st + 16))
        assert not sc.accepted(row, d._replace(dst_st=d.dst_st + 16))
        # >= 130 rows: the span is what binds, and it ends within one step per row of the limit
        if t.srows >= 130:
            assert smax - (t.srows - 1) * 16 < sc.span(t.srows, s.src_st, sb) <= smax
        else:
            assert s.src_st == sst_max // 16 * 16, "fewer than 130 rows: the top layout is the largest stride"
        if drows >= 130:
            assert dmax - (drows - 1) * 16 < sc.span(drows, d.dst_st, db) <= dmax
    else:
        assert (t.srows - 1) * s.src_st >= 2 ** 32 and (drows - 1) * d.dst_st >= 2 ** 32
        assert sc.over(row) == {}
        return
    o = sc.over(row)
    assert set(o) <= {"src_span", "dst_span", "src_stride", "dst_stride"}
    assert {"src_span", "dst_span"} <= set(o), "both span cases run"
    if sst_max < 2 ** 25 and not row.norm:
        assert "src_stride" in o
    if dst_max < 2 ** 25:
        assert "dst_stride" in o
    for which, lay in o.items():
        assert not sc.accepted(row, lay) and sc.fits(row, lay), which
        back = {"src_span": ("src_st", 16), "dst_span": ("dst_st", 16), "src_stride": ("src_st", 16),
                "dst_stride": ("dst_st", 16)}[which]
        assert sc.accepted(row, lay._replace(**{back[0]: getattr(lay, back[0]) - back[1]})), which
    # the span cases trip the span alone, the stride cases the stride alone
    assert o["src_span"].src_st <= sst_max and o["dst_span"].dst_st <= dst_max
    if "src_stride" in o and not row.norm:
        assert o["src_stride"].src_st > sst_max and sc.span(o["src_stride"].srows, 0, sb) <= smax
    if "dst_stride" in o:
        assert o["dst_stride"].dst_st > dst_max and o["dst_stride"].rows == 1


@pytest.mark.parametrize("name", sc.BAND)
def test_band_under_a_frame_over(name):
    row = sc.BY_NAME[name]
    b = sc.band(row)
    sb, db = sc.row_bytes(row)
    whole = sc.window(row)
    assert sc.span(whole[1], b.src_st, sb) > row.limits[0] and sc.span(row.dh, b.dst_st, db) > row.limits[1]
    assert sc.accepted(row, b) and b.rows == sc.BAND_ROWS and 0 < b.r0 < row.dh - b.rows
    assert sc.fits(row, b)  # the band lies where the frame's layout puts it, inside the buffers


@ROWS
def test_every_shape_has_a_pinned_answer(row):
    assert ic.pinned_answer(row.method, row.d, row.sw, row.sh, row.dw, row.dh, row.px)
