"""The block maps of the frame-folding kernels and the batch table of tests/batch_cases.py, without a GPU.

Every frame-folding launcher reports the grid it launches and the numbers its kernel decodes a workgroup id with
(include/iqo_hip.h iqo_hip_launch_grid): the launcher itself, run up to the launch.  Here: xcd_spread and
xcd_chunks, restated in Python from their definition, are bijections of [0, n) -- for every (C, n) a table row
reaches and for all C <= 40, n < 1500; every row of the table runs the kernel body it names and reaches exactly
the regimes it claims; every body reaches every regime its geometry allows with at most 128 frames, and a regime
that cannot be reached says why.  tests/test_batch_gpu.py then launches every row at every frame count.
"""
import ctypes
import os
import re

import numpy as np
import pytest

import batch_cases as bc
import libiqo_amd

EINVAL = -1  # IQO_HIP_EINVAL
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _grid(row, n):
    return libiqo_amd.host_launch_grid(*bc.query_args(row, n))


def _is_bijection(C, n):
    return np.array_equal(np.sort(bc.xcd_chunks_all(C, n)), np.arange(n))


def test_scalar_and_vector_models_agree():
    for C, n in ((1, 1), (1, 7), (1, 8), (1, 9), (3, 24), (3, 25), (3, 71), (4, 150), (7, 112), (7, 113), (40, 1499)):
        assert [bc.xcd_chunks(L, C, n) for L in range(n)] == bc.xcd_chunks_all(C, n).tolist(), (C, n)
    for n in (1, 5, 8, 13, 64, 71):
        assert sorted(bc.xcd_spread(L, n) for L in range(n)) == list(range(n)), n
        assert [bc.xcd_spread(L, n) for L in range(n)] == [bc.xcd_chunks(L, n + 1, n) for L in range(n)]


def test_chunk_map_is_a_bijection_for_every_small_grid():
    bad = [(C, n) for C in range(0, 41) for n in range(0, 1500) if not _is_bijection(C, n)]
    assert not bad, bad[:10]


def test_chunk_map_sends_a_whole_round_to_eight_neighbouring_chunks():
    """The property the map exists for: in the whole rounds XCD x gets chunks x, x + 8, ... in order."""
    C, n = 3, 8 * 3 * 2 + 11
    got = bc.xcd_chunks_all(C, n)
    for L in range(8 * C * 2):
        assert got[L] // C == 8 * ((L // 8) // C) + L % 8 and got[L] % C == (L // 8) % C


@pytest.mark.parametrize("row", bc.ROWS, ids=bc.rid)
def test_row_reaches_what_it_claims(row):
    body, claims = row[0], row[-1]
    family, small_map = bc.BODIES[body]
    assert max(claims) <= bc.MAX_FRAMES and min(claims) >= 1
    for n, want in sorted(claims.items()):
        g = _grid(row, n)
        assert g["family"] == family and g["frames"] == n, (n, g)
        assert bc.regimes(g) == want, (n, g)
        # the body: ryu_kernel maps by chunks and ryg_kernel by spread; the stacked streamer holds several frames per
        # workgroup and maps nothing; the block-shared one maps by chunks or splits the XCDs' tails
        if body == "lanczos_symb":
            assert g["map"] == ("xcd_tail" if "XT" in want else "chunks") and g["framesPerBlock"] == 1
            assert g["unitsPerBlock"] == 1 and g["unitsPerFrame"] == g["bands"]
        elif body == "lanczos_stack":
            assert g["map"] == "none" and g["framesPerBlock"] >= 2
            assert g["gridX"] == g["bands"] and g["gridY"] == -(-n // g["framesPerBlock"])
        else:
            assert g["map"] == small_map, (n, g)
        if g["map"] == "chunks":
            assert g["blocks"] == g["gridX"] * g["gridY"] and g["chunk"] >= 1
            assert g["units"] == n * g["unitsPerFrame"]
            assert g["blocks"] == -(-g["units"] // g["unitsPerBlock"])
            assert g["chunk"] == -(-g["unitsPerFrame"] // g["unitsPerBlock"])
            assert _is_bijection(g["chunk"], g["blocks"])
            # every unit of every frame is some workgroup's, once: the decode frame = unit // unitsPerFrame
            units = (bc.xcd_chunks_all(g["chunk"], g["blocks"])[:, None] * g["unitsPerBlock"]
                     + np.arange(g["unitsPerBlock"])[None, :]).ravel()
            live = np.sort(units[units < g["units"]])
            assert np.array_equal(live, np.arange(g["units"]))
            assert np.array_equal(np.bincount(live // g["unitsPerFrame"], minlength=n),
                                  np.full(n, g["unitsPerFrame"]))
        elif g["map"] == "spread":
            assert g["blocks"] == g["gridX"] == g["units"] == n * g["unitsPerFrame"]
            assert sorted(bc.xcd_spread(L, g["blocks"]) for L in range(g["blocks"])) == list(range(g["blocks"]))
        elif g["map"] == "xcd_tail":
            assert n % 8 == 0 and n >= 16 and g["tailBands"] > g["bands"]
            assert g["gridX"] == 8 * ((n // 8 - 1) * g["bands"] + g["tailBands"]) and g["gridY"] == 1
            cover = [c for c in bc.xcd_tail_cover(g) if c is not None]
            want_cover = [(f, b) for f in range(n) for b in range(g["tailBands"] if f >= n - 8 else g["bands"])]
            assert sorted(cover) == want_cover


@pytest.mark.parametrize("body", sorted(bc.BODIES))
def test_body_reaches_every_regime_it_can(body):
    rows = [r for r in bc.ROWS if r[0] == body]
    assert 1 <= len(rows) <= 2
    reached = set()
    for row in rows:
        for n in row[-1]:
            reached |= set(bc.regimes(_grid(row, n)).split())
    need = set(bc.required(body))
    assert need <= reached, "%s never reaches %s" % (body, sorted(need - reached))
    for r in bc.CHUNK_REGIMES + ("X", "P"):
        why = bc.UNREACHABLE.get((body, r))
        assert (r in need) != bool(why)
        assert not why or r not in reached, "%s reaches %s, which the table calls unreachable" % (body, r)


def test_table_covers_the_folding_bodies_and_the_asked_shapes():
    assert {r[0] for r in bc.ROWS} == set(bc.BODIES) and len(bc.BODIES) == 14
    assert len({bc.rid(r) for r in bc.ROWS}) == len(bc.ROWS)
    assert {r[3] for r in bc.ROWS if r[0] == "packed_tile"} == {3, 4}
    assert any("bands" in dict(r[9]) for r in bc.ROWS)
    # the chunk-mapped bodies with four waves per workgroup: X and P are required of them, not excused
    for body in ("walk", "lanczos_up2", "lanczos_d32", "lanczos_d31", "area_d32", "lanczos_u23", "linear_u23"):
        assert {"X", "P"} <= set(bc.required(body))


def test_plain_grids_report_no_map():
    """The families that keep the frames in gridDim.y."""
    for method, degree, C, sw, sh, dw, dh, options, family in (
            ("lanczos", 3, 1, 64, 32, 48, 24, (("force_general", 1),), "general"),
            ("area", 0, 1, 64, 32, 32, 16, (), "area_int"),
            ("linear", 0, 1, 64, 32, 128, 64, (), "linear_up2"),
            ("lanczos", 8, 3, 96, 64, 48, 32, (), "packed_general")):
        g = libiqo_amd.host_launch_grid(method, degree, sw, sh, dw, dh, 5, 1, C, options)
        assert g["family"] == family and g["map"] == "none", g
        assert g["gridY"] == 5 and g["chunk"] == 0 and g["units"] == 0, g
        assert g["blocks"] == g["gridX"] >= 1 and g["unitsPerBlock"] == 0 and g["framesPerBlock"] == 1


def test_launches_are_capped_at_65535_frames_and_by_chunk_frames():
    row = bc.ROWS[0]
    assert _grid(row, 70000)["frames"] == 65535
    args = list(bc.query_args(row, 100))
    args[-1] = args[-1] + (("chunk_frames", 30),)
    assert libiqo_amd.host_launch_grid(*args)["frames"] == 25  # four equal launches


def test_misuse_is_rejected():
    L = libiqo_amd.lib()
    d = libiqo_amd.LaunchGrid()
    ref = ctypes.byref(d)
    opts = (libiqo_amd._Option * 1)()
    ok = (0, 3, 1, 64, 32, 48, 24, 1, opts, 0, 4, ref)
    assert L.iqo_host_launch_grid(*ok) == 0 and d.frames == 4
    for i, bad in ((0, 3), (0, -1), (2, 0), (2, 5), (10, 0)):   # method, channels, no frames
        a = list(ok)
        a[i] = bad
        assert L.iqo_host_launch_grid(*a) == EINVAL, (i, bad)
    assert L.iqo_host_launch_grid(*(ok[:11] + (None,))) == EINVAL
    assert L.iqo_host_launch_grid(*(ok[:8] + (None, 1) + ok[10:])) == EINVAL
    assert L.iqo_host_launch_grid(0, 3, 1, 0, 32, 48, 24, 1, opts, 0, 4, ref) == EINVAL  # a rejected shape
    with pytest.raises(libiqo_amd.IqoError):
        libiqo_amd.host_launch_grid("lanczos", 3, 64, 32, 48, 24, 4, options=(("no_such_option", 1),))
    assert L.iqo_hip_plan_launch_grid(None, 4, 0, 1, ref) == EINVAL


@pytest.mark.parametrize("kind,table", [("yuv_rgb", bc.STRIDE_YUV), ("rgb_yuv", bc.STRIDE_RGB_YUV),
                                        ("planes_norm", bc.STRIDE_PLANES)])
def test_grid_stride_calls_take_the_trips_they_claim(kind, table):
    """The conditions of tests/test_batch_gpu.py's grid-stride calls, checked where nothing is launched: the item
    counts lie between `times` and `times` + 1 caps and are no multiple of 256, a trip starts mid-row, mid-frame
    and on another frame of the cycle, and every buffer stays under 64 MiB."""
    cap = libiqo_amd.GRID_STRIDE_BLOCKS
    assert [t for _, t in table] == [1, 2]
    assert all(s[4] % 8 for s, _ in table) and any(s[4] % 2 for s, _ in table)
    for shape, times in table:
        sw, sh, dw, dh = shape[2:6]
        for px in ((8,) if kind == "rgb_yuv" else (8, 4)):
            n, period = bc.stride_plan(kind, shape, px, times, cap, (5,) if kind == "yuv_rgb" else (5, 6, 7, 9, 11))
            ipf, groups = bc.stride_items(kind, shape, px)
            assert groups & (groups - 1) and ipf & (ipf - 1), (shape, px)
            elem = 4 if px == 4 else 2
            if kind == "yuv_rgb":
                sizes = [n * (sw * sh + 2 * (sw // 2) * (sh // 2)), n * dw * dh * (3 * elem if px == 4 else 6),
                         n * dw * dh * 4, libiqo_amd.yuv_rgb_workspace_bytes(dw, dh, n, "full")]
            elif kind == "rgb_yuv":
                sizes = [n * sw * sh * 4, n * (dw * dh + 2 * (dw // 2) * (dh // 2)),
                         libiqo_amd.rgb_yuv_workspace_bytes(dw, dh, 4, n)]
            else:
                sizes = [n * 3 * sw * sh, n * 3 * dw * dh * elem, libiqo_amd.planes_norm_workspace_bytes(dw, dh, 3, n)]
            assert max(sizes) < bc.MAX_BUFFER, (shape, px, n, sizes)


def test_exported_constants_are_the_header_s():
    with open(os.path.join(ROOT, "include", "iqo_hip.h")) as f:
        text = f.read()
    assert int(re.search(r"#define IQO_HIP_GRID_STRIDE_BLOCKS (\d+)u", text).group(1)) == libiqo_amd.GRID_STRIDE_BLOCKS
    maps = re.search(r"enum \{ (IQO_GRID_MAP_NONE[^}]*)\}", text).group(1)
    got = {k.strip()[len("IQO_GRID_MAP_"):].lower(): int(v) for k, v in (e.split("=") for e in maps.split(","))}
    assert got == {v: k for k, v in libiqo_amd.GRID_MAPS.items()}
    # one definition in the sources, used by the three second-pass launchers
    src = os.path.join(ROOT, "libiqo_amd", "csrc")
    uses = {n: open(os.path.join(src, n)).read().count("kGridStrideBlocks)") for n in ("kernels_color.hip", "kernels_norm.hip")}
    assert uses == {"kernels_color.hip": 3, "kernels_norm.hip": 1}
    assert open(os.path.join(src, "kernels.hpp")).read().count("constexpr unsigned kGridStrideBlocks = %d;" % libiqo_amd.GRID_STRIDE_BLOCKS) == 1
