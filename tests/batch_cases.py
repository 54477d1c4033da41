"""Batch sizes that turn the block map of every frame-folding kernel (tests/test_batch_host.py,
tests/test_batch_gpu.py).  Test infrastructure only.

The frame-folding kernels put a whole batch into one range of workgroup ids and decode (column, band, frame) from an
id that xcd_chunks / xcd_spread (kernels_dev.hpp) has permuted.  Which arm of that map a call takes depends on the
batch size alone, and the two- and three-frame calls of the other tests only ever take the tail arm.  This module
restates the two maps in Python from their definition (include/iqo_hip.h, iqo_hip_launch_grid), names the regimes of
a launch from the numbers the launcher itself reports (libiqo_amd.host_launch_grid, Resizer.launch_grid), and lists
small shapes per kernel body with the frame counts that reach each regime.  A row is

    (body, method, degree, channels, sw, sh, dw, dh, pxScale, options, {frames: "regimes"})

with the regimes written out as literals: the host test recomputes them from the host query and fails on any
difference, the GPU test from the live plan before it launches anything.

Regimes of one launch of n workgroup ids in chunks of C (full = n // 8C whole rounds, tail = n - 8C full ids):
    T    full == 0: the tail arm only (what the two- and three-frame tests reach)
    W    full >= 1 and no tail
    WT   full >= 1 and a tail that is not a multiple of 8 (both arms, and both arms of the spread inside the tail)
    W2   full >= 2
    X    unitsPerFrame % unitsPerBlock != 0: some workgroup's waves belong to two frames
    P    units % unitsPerBlock != 0: the last workgroup has spare waves that must do nothing
and, for the bodies that do not map by chunks,
    S    xcd_spread over at least 16 ids that are not a multiple of 8 (both of its arms, more than one id per XCD)
    XT   the block-shared streamer's XCD tail split (frames a multiple of 8, at least 16)
    G    the stacked streamer with a last workgroup that holds fewer frames than the others
"""
import functools

import numpy as np

import oracle_lib as ol
import packed_cases as pc
from instance_cases import RATIO_OFF, TILE_ONLY

MAX_FRAMES = 128  # every regime must be reached with at most this many frames


# ---- the two maps, from their definition

def xcd_spread(L, n):
    """Flat id L of n -> logical id: XCD x = L mod 8 takes a contiguous eighth of [0, n)."""
    x, i, q, r = L % 8, L // 8, n // 8, n % 8
    return x * (q + 1) + i if x < r else r * (q + 1) + (x - r) * q + i


def xcd_chunks(L, C, n):
    """Chunks of C ids dealt round-robin over the XCDs for the whole rounds of 8 chunks, xcd_spread for the rest."""
    C = C or 1
    x, i, full = L % 8, L // 8, n // (8 * C)
    if i < full * C:
        return (8 * (i // C) + x) * C + i % C
    base = 8 * full * C
    return base + xcd_spread(L - base, n - base)


def xcd_chunks_all(C, n):
    """xcd_chunks of every id of [0, n) at once (numpy; the same arithmetic)."""
    C = C or 1
    L = np.arange(n, dtype=np.int64)
    x, i, full = L % 8, L // 8, n // (8 * C)
    base = 8 * full * C
    m = n - base
    Lt = L - base
    xt, it, q, r = Lt % 8, Lt // 8, m // 8, m % 8
    spread = np.where(xt < r, xt * (q + 1) + it, r * (q + 1) + (xt - r) * q + it)
    return np.where(i < full * C, (8 * (i // C) + x) * C + i % C, base + spread)


def xcd_tail_cover(grid):
    """The (frame, band) every workgroup of an XCD-tail-split launch resizes, None for one that exits at once:
    XCD x takes frames x, x + 8, ... in `bands` bands each and its last frame in `tailBands`."""
    F8, bands, tb = grid["frames"] // 8, grid["bands"], grid["tailBands"]
    n_long = (F8 - 1) * bands
    out = []
    for L in range(grid["gridX"]):
        x, i = L % 8, L // 8
        if i < n_long:
            out.append((8 * (i // bands) + x, i % bands))
        else:
            out.append((8 * (F8 - 1) + x, i - n_long) if i - n_long < tb else None)
    return out


def regimes(grid):
    """The regimes (module docstring) of a launch, from a launch_grid dict."""
    r = []
    if grid["map"] == "chunks":
        n, C = grid["blocks"], grid["chunk"]
        full = n // (8 * C)
        tail = n - 8 * full * C
        if full == 0:
            r.append("T")
        if full >= 1 and tail == 0:
            r.append("W")
        if full >= 1 and tail > 0 and tail % 8:
            r.append("WT")
        if full >= 2:
            r.append("W2")
    if grid["map"] == "spread" and grid["blocks"] >= 16 and grid["blocks"] % 8:
        r.append("S")
    if grid["map"] == "xcd_tail":
        r.append("XT")
    if grid["unitsPerBlock"]:
        if grid["unitsPerFrame"] % grid["unitsPerBlock"]:
            r.append("X")
        if grid["units"] % grid["unitsPerBlock"]:
            r.append("P")
    if grid["framesPerBlock"] > 1 and grid["gridY"] >= 2 and grid["frames"] % grid["framesPerBlock"]:
        r.append("G")
    return " ".join(r)


# ---- the table

# body -> (family of the query, map of a small batch): what tells the bodies of one family apart
BODIES = {
    "tile": ("tile", "chunks"), "packed_tile": ("packed_tile", "chunks"), "walk": ("walk", "chunks"),
    "lanczos_up2": ("lanczos_up2", "chunks"), "lanczos_d32": ("lanczos_d32", "chunks"),
    "lanczos_d31": ("lanczos_d31", "chunks"), "area_d32": ("area_d32", "chunks"),
    "lanczos_u23": ("lanczos_u23", "chunks"), "linear_u23": ("linear_u23", "chunks"),
    "ryx": ("ryx", "chunks"), "ryg": ("ryg", "spread"), "ryu": ("ryg", "chunks"),
    "lanczos_symb": ("lanczos_stream", "chunks"), "lanczos_stack": ("lanczos_stream", "none"),
}

# Shapes from tests/instance_cases.py (SEARCHED, EXACT, EXTRA) and tests/packed_cases.py SHAPES; the exact-ratio
# kernels also at the smallest shape with one wave per frame, where four frames share a workgroup; the streamers at
# the narrowest width that is not stacked (srcW 512) and at a stacked one.  One row sets the public `bands` option
# (walker, ryx).
ROWS = [
    ('tile', 'lanczos', 4, 1, 16, 8, 16, 16, 1, (),
     {3: 'T', 8: 'W', 13: 'WT', 16: 'W W2'}),
    ('tile', 'area', 0, 1, 378, 9, 16, 21, 1, TILE_ONLY,
     {3: 'T', 8: 'W', 11: 'WT', 19: 'WT W2'}),
    ('packed_tile', 'lanczos', 3, 3, 40, 24, 27, 17, 1, (),
     {3: 'T', 8: 'W', 11: 'WT', 17: 'WT W2'}),
    ('packed_tile', 'linear', 0, 4, 40, 24, 56, 34, 1, (),
     {2: 'T', 8: 'W', 13: 'WT', 17: 'WT W2'}),
    ('walk', 'area', 0, 1, 17, 17, 16, 16, 1, (),
     {3: 'T X P', 32: 'W X', 37: 'WT X P', 64: 'W W2 X'}),
    ('walk', 'lanczos', 1, 1, 345, 9, 346, 16, 1, RATIO_OFF + (('bands', 3),),
     {3: 'T X P', 11: 'WT X P', 21: 'W W2 X P', 23: 'WT W2 X P'}),
    ('lanczos_up2', 'lanczos', 2, 1, 16, 5, 48, 15, 1, (),
     {3: 'T X P', 32: 'W X', 37: 'WT X P', 61: 'W W2 X P'}),
    ('lanczos_up2', 'lanczos', 2, 1, 200, 60, 400, 120, 1, (),
     {3: 'T X P', 9: 'WT X P', 17: 'W W2 X P', 19: 'W2 X P'}),
    ('lanczos_d32', 'lanczos', 2, 1, 48, 30, 32, 20, 1, (),
     {3: 'T X P', 30: 'W X P', 35: 'WT X P', 62: 'W W2 X P'}),
    ('lanczos_d32', 'lanczos', 2, 1, 240, 150, 160, 100, 1, (),
     {3: 'T X P', 11: 'WT X P', 21: 'W W2 X P', 23: 'WT W2 X P'}),
    ('lanczos_d31', 'lanczos', 2, 1, 48, 30, 16, 10, 1, (),
     {3: 'T X P', 31: 'W X P', 38: 'WT X P', 63: 'W W2 X P'}),
    ('lanczos_d31', 'lanczos', 3, 1, 336, 204, 112, 68, 1, (),
     {3: 'T X P', 13: 'WT X P', 25: 'W W2 X P', 27: 'WT W2 X P'}),
    ('area_d32', 'area', 0, 1, 12, 6, 8, 4, 1, (),
     {3: 'T X P', 29: 'W X P', 33: 'WT X P', 66: 'WT W2 X P'}),
    ('area_d32', 'area', 0, 1, 48, 30, 32, 20, 1, (),
     {3: 'T X P', 15: 'W X P', 17: 'WT X P', 33: 'WT W2 X P'}),
    ('lanczos_u23', 'lanczos', 3, 1, 16, 16, 24, 24, 1, (),
     {3: 'T X P', 32: 'W X', 34: 'WT X P', 65: 'WT W2 X P'}),
    ('lanczos_u23', 'lanczos', 3, 1, 512, 16, 768, 24, 1, (),
     {3: 'T X P', 16: 'W X', 19: 'WT X P', 31: 'W W2 X P'}),
    ('linear_u23', 'linear', 0, 1, 16, 16, 24, 24, 1, (),
     {3: 'T X P', 15: 'W X P', 21: 'WT X P', 35: 'WT W2 X P'}),
    ('linear_u23', 'linear', 0, 1, 512, 16, 768, 24, 1, (),
     {3: 'T', 8: 'W', 11: 'WT', 17: 'WT W2'}),
    ('ryx', 'area', 0, 1, 17, 36, 16, 16, 1, (),
     {3: 'T', 8: 'W', 13: 'WT', 18: 'WT W2'}),
    ('ryx', 'lanczos', 3, 1, 41, 36, 16, 16, 1, (('ryx_split', 3), ('ryx_adj', 0), ('bands', 2)),
     {3: 'T', 8: 'W', 11: 'WT', 17: 'WT W2'}),
    ('ryg', 'linear', 0, 1, 17, 17, 16, 16, 1, (('ryg_cpt', 2),),
     {3: '', 11: 'S', 43: 'S'}),
    ('ryu', 'lanczos', 2, 1, 17, 8, 16, 16, 1, (),
     {3: 'T', 8: 'W', 11: 'WT', 17: 'WT W2'}),
    ('lanczos_symb', 'lanczos', 3, 1, 512, 32, 256, 16, 1, (),
     {3: 'T', 8: 'W', 11: 'WT', 16: 'XT', 17: 'WT W2'}),
    ('lanczos_symb', 'lanczos', 2, 1, 512, 64, 256, 32, 1, (),
     {3: 'T', 8: 'W', 13: 'WT', 17: 'WT W2', 24: 'XT'}),
    ('lanczos_stack', 'lanczos', 3, 1, 64, 32, 32, 16, 1, (),
     {2: '', 7: 'G', 13: 'G'}),
    ('lanczos_stack', 'lanczos', 2, 1, 64, 64, 32, 32, 1, (),
     {5: '', 16: 'G'}),
]

# What each body must reach between its rows, and why the rest cannot be reached.
CHUNK_REGIMES = ("T", "W", "WT", "W2")
_ONE_UNIT = ("one unit per workgroup (a tile / a workgroup of one band and column part): unitsPerBlock is 1, so no "
             "workgroup spans two frames and none is partial")
_SPREAD = ("ryg_kernel keeps xcd_spread (kernels_ratio.hip: the chunk map measured slower for it), which has no whole "
           "rounds; its two arms are regime S")
_STACK = ("lanczos_stack_kernel keeps (band, frame group) in gridDim.x / .y and maps nothing; its partial last group is "
          "regime G")
UNREACHABLE = dict(
    [((b, r), _ONE_UNIT) for b in ("tile", "packed_tile", "ryx", "ryu", "lanczos_symb") for r in ("X", "P")] +
    [(("ryg", r), _SPREAD) for r in CHUNK_REGIMES] + [(("ryg", r), _ONE_UNIT) for r in ("X", "P")] +
    [(("lanczos_stack", r), _STACK) for r in CHUNK_REGIMES + ("X", "P")])
# ... and the regimes of their own that three bodies must reach
ALSO = {"ryg": ("S",), "lanczos_symb": ("XT",), "lanczos_stack": ("G",)}


def required(body):
    return tuple(r for r in CHUNK_REGIMES + ("X", "P") if (body, r) not in UNREACHABLE) + ALSO.get(body, ())


def rid(row):
    body, method, degree, C, sw, sh, dw, dh, px, options, _ = row
    return "%s-%s%d-c%d-%dx%d-%dx%d%s" % (body, method, degree, C, sw, sh, dw, dh,
                                          "-bands%d" % dict(options)["bands"] if "bands" in dict(options) else "")


def query_args(row, frames):
    """Arguments of libiqo_amd.host_launch_grid for `frames` frames of the row."""
    _, method, degree, C, sw, sh, dw, dh, px, options, _ = row
    return (method, degree, sw, sh, dw, dh, frames, px, C, tuple(options))


# ---- frames and their oracle results: distinct noise per frame, one frame with a flat-255 band

def band_frame(n):
    """The frame of an n-frame batch that carries the flat band."""
    return n // 2


def _noise(row, f):
    _, _, _, C, sw, sh, _, _, _, _, _ = row
    seed = 9000 + 131 * f
    return pc.packed_noise(sw, sh, C, seed) if C > 1 else ol.gen("noise", sw, sh, seed)


def _banded(img):
    out = img.copy()
    sh = out.shape[0]
    out[sh // 3: max(sh // 3 + 1, 2 * sh // 3)] = 255
    return out


def _oracle(row, img):
    _, method, degree, C, sw, sh, dw, dh, px, _, _ = row
    if C > 1:
        return pc.oracle_packed((method, degree, sw, sh, dw, dh, px), img)
    return ol.run_oracle(method, degree, sw, sh, dw, dh, px, img)


@functools.lru_cache(maxsize=None)
def _shared(key):
    """(noise frames, their oracle results, oracle results of the same frames with the flat band) for the row's
    largest frame count, computed once and read-only; every smaller batch takes its first frames."""
    row = next(r for r in ROWS if rid(r) == key)
    n = max(row[-1])
    frames = np.stack([_noise(row, f) for f in range(n)])
    exp = np.stack([_oracle(row, f) for f in frames])
    banded = {band_frame(k): None for k in row[-1]}
    for f in banded:
        banded[f] = _oracle(row, _banded(frames[f]))
    for a in (frames, exp) + tuple(banded.values()):
        a.setflags(write=False)
    return frames, exp, banded


def batch_for(row, n):
    """(frames [n, sh, sw(, C)], expected [n, dh, dw(, C)]) of an n-frame batch of the row: frame f is noise of its
    own seed, frame band_frame(n) with its middle third of rows set to 255."""
    frames, exp, banded = _shared(rid(row))
    b = band_frame(n)
    src, want = frames[:n].copy(), exp[:n].copy()
    src[b] = _banded(frames[b])
    want[b] = banded[b]
    return src, want


# ---- grid-stride trips of the second-pass kernels (yuv_rgb_kernel, rgb_yuv_kernel, planes_norm_kernel)
#
# A launch has at most GRID_STRIDE_BLOCKS workgroups of 256 items and strides over the rest.  An item is one thread's
# run of a row: 8 pixels (bytes, float16, bfloat16) or 4 (float32) of yuv_rgb / planes_norm, 8 pixels of a row PAIR of
# rgb_yuv.  (shape, times): the call has between `times` and `times` + 1 times the cap's items, so the loop takes
# `times` further trips.  Small outputs whose groups per row are no power of two in either form, so that a trip starts
# in the middle of a row and of a frame: widths 33 (5 / 9 groups), 22 (3 / 6), 20 (3 / 5) and 17 (3 / 5); 33 and 17 are
# odd, and no width is a multiple of 8.
STRIDE_YUV = ((("lanczos", 3, 64, 32, 33, 17), 1), (("area", 0, 12, 10, 22, 23), 2))  # (5 frames: see stride_plan)
STRIDE_RGB_YUV = ((("area", 0, 12, 10, 22, 25, 1), 1), (("area", 0, 6, 2, 17, 3, 1), 2))
STRIDE_PLANES = ((("lanczos", 3, 40, 24, 20, 12), 1), (("area", 0, 12, 10, 17, 25), 2))
MAX_BUFFER = 64 << 20  # bytes, of every buffer of a call


def stride_items(kind, shape, px):
    """(items per frame, groups per row) of a second-pass launch: kind "yuv_rgb", "rgb_yuv" or "planes_norm"."""
    dw, dh = shape[4], shape[5]
    groups = -(-dw // px)
    return ((dh + 1) // 2 if kind == "rgb_yuv" else dh) * groups, groups


def stride_plan(kind, shape, px, times, cap_blocks, periods=(5, 6, 7, 9, 11)):
    """(frames, period) of the call: the fewest frames about 3 % past `times` caps whose item count is no multiple of
    256, cycling through `period` distinct frames; with every condition the trips must meet asserted."""
    cap = cap_blocks * 256
    ipf, groups = stride_items(kind, shape, px)
    n = times * cap // ipf + max(2, cap // (32 * ipf))
    while (n * ipf) % 256 == 0:
        n += 1
    items = n * ipf
    assert times * cap < items < (times + 1) * cap and items % 256
    assert min((items + 255) // 256, cap_blocks) == cap_blocks          # the launch has exactly the cap's workgroups
    assert cap % ipf and cap % groups                                   # a trip starts mid-frame and mid-row
    period = next(p for p in periods if (cap // ipf) % p)               # ... and on another frame of the cycle
    assert period >= 5
    return n, period
