"""Extreme inputs for the Lanczos kernel families (tests/test_extreme_host.py, tests/test_extreme_gpu.py).
Test infrastructure only.

The Lanczos kernels do not compute what the reference computes but something proven equal under range
arguments (saturating shifts for clamps, multiply-high for divisions, sign flips for negative
denominators).  Noise never leaves the comfortable middle of those ranges; the frames built here do.

tap-sign frames   per axis a 0/1 pattern: walking the outputs, every output whose source window does not
                  overlap the previous target's becomes a target (output 0 and the last output always),
                  and its window is set to 1 on the positive taps, 0 on the negative ones -- or the other
                  way round: the polarity alternates from target to target.  The frame is
                  255 * outer(py, px); two starting polarities per axis and each frame's complement
                  give eight frames.  The first interior output whose taps have the largest positive sum
                  is made a target before the walk, so the analytic extreme 255 * sum(positive taps) of
                  each pass is attained.
border-stress     the same construction on the taps a border row or column really has (those inside the
                  image), for the border outputs with a negative or the smallest denominator on each side,
                  in both polarities: negative numerators over negative denominators, and quotients
                  that wrap int16.

A frame set is one noise frame (the control) followed by the extreme frames.
"""
import collections
import functools

import numpy as np

import oracle_lib as ol

# ----------------------------------------------------------------------------- geometry of one axis


def axis_geometry(tab, src_len, dst_len):
    """(window start of every output, phase of every output, mainBegin, mainEnd) as the reference walks an axis
    (IQOLanczosResizerImpl_Generic.cpp resize / resizeX)."""
    ph, nt = tab.shape
    m = nt // 2
    d = np.arange(dst_len, dtype=np.int64)
    lo = d * src_len // dst_len + 1 - m
    main_begin = min(dst_len, ((m - 1) * dst_len + src_len - 1) // src_len)
    main_end = max(0, (src_len - m) * dst_len // src_len)
    return lo, d % ph, main_begin, main_end


def _paint(pat, coefs, lo, pol):
    """Window at lo: 1 where the tap's sign is `pol`'s (pol 0: positive taps), 0 on the other sign; zero taps
    keep what they have."""
    for i, c in enumerate(coefs):
        s = lo + i
        if 0 <= s < pat.size and c != 0:
            pat[s] = 1 if (c > 0) != bool(pol) else 0


def tap_sign_pattern(tab, src_len, dst_len, flip):
    """0/1 pattern of one axis (module docstring); flip = the starting polarity."""
    lo, phase, mb, me = axis_geometry(tab, src_len, dst_len)
    nt = tab.shape[1]
    pos = np.where(tab > 0, tab, 0).sum(axis=1)
    targets = {0, dst_len - 1}
    if me > mb:  # the first interior output with the largest positive sum
        inner = np.arange(mb, me)
        best = pos[phase[inner]].max()
        clear = inner[(lo[inner] >= lo[0] + nt) & (lo[inner] + nt <= lo[dst_len - 1]) & (pos[phase[inner]] == best)]
        targets.add(int(clear[0] if clear.size else inner[np.argmax(pos[phase[inner]])]))
    fixed = sorted(targets)
    chosen = list(fixed)
    for d in range(dst_len):  # the walk: no overlap with a target before it, nor with a fixed one after it
        if d in targets:
            continue
        before = [t for t in chosen if t < d]
        after = [t for t in fixed if t > d]
        if before and lo[d] < lo[max(before)] + nt:
            continue
        if after and lo[min(after)] < lo[d] + nt:
            continue
        chosen.append(d)
        chosen.sort()
    pat = np.zeros(src_len, np.uint8)
    order = [t for t in chosen if t not in (0, dst_len - 1)] + [0, dst_len - 1]  # the two ends painted last
    rank = {t: k for k, t in enumerate(chosen)}
    for t in order:
        _paint(pat, tab[phase[t]], int(lo[t]), (rank[t] + flip) & 1)
    return pat


def border_outputs(tab, src_len, dst_len):
    """[(output, denominator)] of the border outputs of one axis whose denominator is not zero."""
    lo, phase, mb, me = axis_geometry(tab, src_len, dst_len)
    nt = tab.shape[1]
    out = []
    for d in list(range(0, mb)) + list(range(max(me, mb), dst_len)):
        s = lo[d] + np.arange(nt)
        deno = int(tab[phase[d]][(s >= 0) & (s < src_len)].sum())
        if deno:
            out.append((d, deno))
    return out


def border_stress_patterns(tab, src_len, dst_len):
    """0/1 patterns that stress single border outputs: per side, the output with the smallest |denominator|
    and the one with the most negative denominator, each in both polarities.  [] for an axis without
    border outputs."""
    lo, phase, mb, me = axis_geometry(tab, src_len, dst_len)
    b = border_outputs(tab, src_len, dst_len)
    picks = []
    for side in ([x for x in b if x[0] < mb], [x for x in b if x[0] >= mb]):
        if not side:
            continue
        picks.append(min(side, key=lambda x: (abs(x[1]), x[0]))[0])
        neg = [x for x in side if x[1] < 0]
        if neg:
            picks.append(min(neg, key=lambda x: (x[1], x[0]))[0])
            picks.append(max(neg, key=lambda x: (x[1], -x[0]))[0])
    pats = []
    for pol in (0, 1):
        for base in (0, 1):  # what the samples outside the stressed windows hold
            pat = np.full(src_len, base, np.uint8)
            for t in dict.fromkeys(picks):
                _paint(pat, tab[phase[t]], int(lo[t]), pol)
            pats.append(pat)
    return pats if picks else []


# ----------------------------------------------------------------------------- frames of one plane

@functools.lru_cache(maxsize=None)
def plane_frames(d, sw, sh, dw, dh, px, stress=False, seed=77):
    """(names, frames [n, sh, sw]) of one Lanczos plane: noise, the eight tap-sign frames, and with `stress` the
    border-stress frames.  Read-only, computed once per session."""
    tx = ol.oracle_tables("lanczos", d, sw, sh, dw, dh, px, 0)
    ty = ol.oracle_tables("lanczos", d, sw, sh, dw, dh, px, 1)
    names, frames = ["noise"], [ol.gen("noise", sw, sh, seed)]
    for fy in (0, 1):
        py = tap_sign_pattern(ty, sh, dh, fy) if sh != dh else np.ones(sh, np.uint8)
        for fx in (0, 1):
            pxx = tap_sign_pattern(tx, sw, dw, fx) if sw != dw else np.ones(sw, np.uint8)
            f = (255 * np.outer(py, pxx)).astype(np.uint8)
            names += ["sign%d%d" % (fy, fx), "sign%d%dc" % (fy, fx)]
            frames += [f, 255 - f]
    if stress:
        sy = border_stress_patterns(ty, sh, dh) if sh != dh else []
        sx = border_stress_patterns(tx, sw, dw) if sw != dw else []
        ys = sy or [tap_sign_pattern(ty, sh, dh, 0), tap_sign_pattern(ty, sh, dh, 1)]
        xs = sx or [tap_sign_pattern(tx, sw, dw, 0), tap_sign_pattern(tx, sw, dw, 1)]
        for i in range(max(len(ys), len(xs))):
            for j in (0, 1):  # every Y pattern meets two X patterns
                f = (255 * np.outer(ys[i % len(ys)], xs[(i + j) % len(xs)])).astype(np.uint8)
                names += ["stress%d%d" % (i, j), "stress%d%dc" % (i, j)]
                frames += [f, 255 - f]
    out = np.stack(frames)
    out.setflags(write=False)
    return tuple(names), out


@functools.lru_cache(maxsize=None)
def plane_expected(d, sw, sh, dw, dh, px, stress=False, seed=77):
    """Oracle results of plane_frames(...), read-only."""
    _, fr = plane_frames(d, sw, sh, dw, dh, px, stress, seed)
    out = np.stack([ol.run_oracle("lanczos", d, sw, sh, dw, dh, px, f) for f in fr])
    out.setflags(write=False)
    return out


# ----------------------------------------------------------------------------- the case table

# kernel: what host_kernel_for names for the shape with default options.  tile: the exact-ratio kernels and the
# walker switched off leave the separable tile kernel (True) or, where the tile tables do not take the shape,
# general_kernel (False).  stress: border-stress frames are part of the set (negative denominators, wrapping
# quotients).  wrap: the set must make border quotients wrap int16.  batch: frames per call of the GPU test
# (0: the whole set at once); stream: the case also runs the streamer's option variants.
# trap: one border row of the shape has valid taps that sum to 0: the reference divides by zero there (SIGFPE), so
# the shape has no reference answer and no golden hash; the oracle and the kernels write 0 into that row, and
# the kernels are still held to the oracle.
Case = collections.namedtuple("Case", "kernel d sw sh dw dh px tile stress wrap batch stream trap")


def _c(kernel, d, sw, sh, dw, dh, px=1, tile=True, stress=False, wrap=False, batch=0, stream=False, trap=False):
    return Case(kernel, d, sw, sh, dw, dh, px, tile, stress, wrap, batch, stream, trap)


PLANAR = [
    _c("lanczos_stream", 2, 384, 216, 192, 108, stream=True),
    _c("lanczos_stream", 3, 384, 216, 192, 108, stream=True),
    _c("lanczos_stream", 4, 384, 216, 192, 108, stream=True),
    _c("lanczos_stream", 5, 512, 128, 256, 64, stream=True),
    _c("lanczos_stream", 3, 384, 216, 192, 108, px=2, stress=True),   # negative denominators
    _c("lanczos_stream", 3, 256, 24, 128, 12, px=2, stress=True),
    _c("lanczos_stream", 2, 208, 30, 104, 15, batch=13),              # the frame-stacked streamer
    _c("lanczos_stream", 3, 1024, 64, 512, 32, batch=4),
    _c("lanczos_up2", 2, 192, 108, 384, 216),
    _c("lanczos_up2", 3, 192, 108, 384, 216),
    _c("lanczos_up2", 3, 128, 72, 384, 216),                          # 3x
    _c("lanczos_d32", 3, 384, 216, 256, 144),
    _c("lanczos_d32", 2, 240, 150, 160, 100),
    _c("lanczos_d31", 2, 384, 216, 128, 72),
    _c("lanczos_d31", 3, 384, 216, 128, 72),
    _c("lanczos_u23", 3, 256, 144, 384, 216),
    _c("ryx", 3, 384, 216, 96, 54),
    _c("ryx", 3, 160, 120, 360, 270),
    _c("ryx", 5, 384, 216, 192, 108),
    _c("ryx", 6, 256, 128, 128, 64),
    _c("ryx", 9, 256, 128, 128, 64, tile=False),
    _c("ryg", 3, 100, 37, 130, 71),
    _c("ryg", 4, 200, 140, 137, 93),
    _c("ryg", 3, 480, 272, 250, 137, px=2, stress=True),
    _c("ryg", 3, 240, 136, 500, 275, px=2),
    _c("walk", 5, 200, 140, 300, 200),
    _c("walk", 5, 256, 40, 128, 20, px=2, stress=True),               # negative denominators
    _c("walk", 7, 256, 40, 128, 20, px=2, stress=True),
    _c("tile", 3, 13, 9, 5, 40),
    _c("tile", 9, 64, 48, 1000, 900),
    _c("tile", 7, 256, 24, 128, 12, stress=True, wrap=True, trap=True),   # wrapping quotients
    _c("tile", 9, 128, 16, 256, 32, stress=True, trap=True),              # negative Y denominators
    # the two wrap shapes above have a border row the reference cannot divide (trap); their nearest neighbours
    # it can run, so the oracle's int16 wrap is pinned to the reference itself: a short source at L7, and one
    # that also has negative Y denominators
    _c("tile", 7, 256, 26, 128, 13, stress=True, wrap=True),
    _c("tile", 5, 120, 30, 50, 9, stress=True, wrap=True),
    _c("general", 3, 7, 100, 3, 50, tile=False),
    _c("general", 9, 120, 20, 50, 9, tile=False, stress=True, wrap=True, trap=True),
    _c("general", 8, 64, 30, 16, 12, tile=False, stress=True, trap=True),
    _c("general", 9, 256, 24, 128, 12, tile=False, stress=True, wrap=True),   # as above: wraps, no trap
    _c("general", 7, 120, 24, 50, 13, tile=False, stress=True, wrap=True),
]

# options that switch every exact-ratio kernel and the walker off (tests/test_gpu_parity.py "tile" variant)
TILE_OPTIONS = ("walk", "a32", "d32", "d31", "ryx", "ryg", "up2", "u23", "l23")

# (stream_variant, prefetch, lanes, bands) of test_stream_variants_agree_with_oracle
STREAM_OPTIONS = [(0, 1, 0, 0), (0, 2, 0, 7), (0, 3, 0, 0), (0, 2, 62, 3), (0, 3, 33, 0), (0, 3, 0, 1), (0, 4, 0, 0),
                  (0, 4, 0, 7), (1, 3, 0, 0), (1, 1, 0, 5), (2, 3, 0, 0), (2, 1, 0, 5), (2, 2, 40, 0), (0, 3, 41, 0),
                  (0, 4, 0, 3), (0, 2, 0, 1), (0, 4, 33, 1)]

# (kernel, degree, sw, sh, dw, dh, C, through resize_normalized too)
PACKED = [("packed_tile", 3, 40, 24, 27, 17, C, False) for C in (2, 3, 4)] + \
         [("packed_tile", 3, 64, 48, 32, 24, C, C == 3) for C in (2, 3, 4)] + \
         [("packed_general", 9, 120, 20, 50, 9, C, False) for C in (2, 3, 4)]

# fused I420: the first (smallest) row of tests/yuv_cases.py per Lanczos label; NV12: one shape
FUSED = [("lanczos", 3, 3008, 40, 1504, 20, "lz_symb10"), ("lanczos", 3, 64, 32, 32, 16, "lz_sym10"),
         ("lanczos", 2, 3008, 40, 1504, 20, "lz_symb8"), ("lanczos", 2, 64, 32, 32, 16, "lz_sym8")]
NV12 = ("lanczos", 3, 384, 216, 192, 108)


def other_planes():
    """The planes of the packed and YUV cases as rows of the planar form (kernel: the packed or fused label), for
    the host test's regime check: a packed case's channels (pxScale 1, border-stress frames), a YUV case's luma
    and its chroma (half size, pxScale 2, border-stress frames)."""
    out = {}
    for k, d, sw, sh, dw, dh, _, _ in PACKED:
        trap = (d, sw, sh, dw, dh) == (9, 120, 20, 50, 9)
        out[(d, sw, sh, dw, dh, 1)] = _c(k, d, sw, sh, dw, dh, stress=True, wrap=trap, trap=trap)
    for case in FUSED + [NV12 + ("nv12",)]:
        _, d, sw, sh, dw, dh, label = case
        out[(d, sw, sh, dw, dh, 1)] = _c(label, d, sw, sh, dw, dh)
        out[(d, sw // 2, sh // 2, dw // 2, dh // 2, 2)] = _c(label, d, sw // 2, sh // 2, dw // 2, dh // 2, px=2, stress=True)
    return list(out.values())


def cid(c):
    return "%s-L%d-%dx%d-%dx%d-px%d" % tuple(c[:7])


def frames_of(c):
    return plane_frames(c.d, c.sw, c.sh, c.dw, c.dh, c.px, c.stress)


def expected_of(c):
    return plane_expected(c.d, c.sw, c.sh, c.dw, c.dh, c.px, c.stress)


def packed_frames(d, sw, sh, dw, dh, C):
    """(frames [n, sh, sw, C], expected [n, dh, dw, C]): channel c of frame f is plane frame (f + c) % n of the
    shape's set, so every channel of a pixel carries another frame and a leak between channels shows."""
    _, fr = plane_frames(d, sw, sh, dw, dh, 1, True)
    exp = plane_expected(d, sw, sh, dw, dh, 1, True)
    n = fr.shape[0]
    idx = [[(f + 3 * c) % n for c in range(C)] for f in range(n)]
    src = np.stack([np.stack([fr[i] for i in row], axis=2) for row in idx])
    out = np.stack([np.stack([exp[i] for i in row], axis=2) for row in idx])
    return src, out


def yuv_planes(case):
    """(Y, U, V frames, Y, U, V expected) of an I420 / NV12 shape: luma and chroma frame sets each built from
    their own plan's tables (chroma: half size, pxScale 2); V takes the chroma set rotated by one."""
    _, d, sw, sh, dw, dh = case[:6]
    cs = (d, sw // 2, sh // 2, dw // 2, dh // 2, 2, True)
    _, y = plane_frames(d, sw, sh, dw, dh, 1, False)
    _, c = plane_frames(*cs)
    ye, ce = plane_expected(d, sw, sh, dw, dh, 1, False), plane_expected(*cs)
    n = max(y.shape[0], c.shape[0])
    iy = [f % y.shape[0] for f in range(n)]
    iu = [f % c.shape[0] for f in range(n)]
    iv = [(f + 1) % c.shape[0] for f in range(n)]
    return y[iy], c[iu], c[iv], ye[iy], ce[iu], ce[iv]
