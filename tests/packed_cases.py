"""Shapes, inputs and per-channel oracle results shared by the packed (interleaved) resize tests
(tests/test_packed_host.py, tests/test_packed_gpu.py).  Test infrastructure only.

Channel c of a packed result is by definition the reference Generic resize of channel c taken as
a plane, so the expected image is the oracle run per channel and re-interleaved.
"""
import functools

import numpy as np

import oracle_lib as ol

# (method, degree, sw, sh, dw, dh, pxScale)
SHAPES = [
    ("lanczos", 3, 40, 24, 27, 17, 1),
    ("lanczos", 3, 40, 24, 20, 12, 1),
    ("lanczos", 2, 24, 16, 48, 32, 1),
    ("lanczos", 3, 13, 9, 5, 40, 1),       # narrow: every group is an edge group
    ("lanczos", 3, 5, 4, 3, 3, 1),         # srcW < 8: no tile tables
    ("lanczos", 3, 32, 16, 16, 8, 2),
    ("lanczos", 9, 50, 40, 120, 90, 1),
    ("lanczos", 3, 301, 203, 150, 101, 1),
    ("lanczos", 3, 400, 36, 83, 9, 1),     # 4.8:1, many taps
    ("area", 0, 45, 31, 30, 20, 1),
    ("area", 0, 40, 24, 10, 6, 1),
    ("linear", 0, 40, 24, 56, 34, 1),
    ("linear", 0, 41, 25, 30, 18, 1),
]
# taps beyond the tile tables' widest instantiation: build_tile_tables rejects it (packed_general)
GENERAL_SHAPE = ("lanczos", 8, 96, 64, 48, 32, 1)


def sid(shape):
    return "%s%d-%dx%d-%dx%d-px%d" % shape


def packed_noise(sw, sh, C, seed):
    """[sh, sw, C] uint8 noise."""
    return ol.splitmix_bytes(sw * sh * C, seed).reshape(sh, sw, C).copy()


def frames_for(shape, C, n=2):
    """n frames [n, sh, sw, C]: noise; noise with the left third set to 255; further noise."""
    _, _, sw, sh, _, _, _ = shape
    fr = [packed_noise(sw, sh, C, 11 + 7 * C + i) for i in range(n)]
    if n > 1:
        fr[1][:, : max(1, sw // 3), :] = 255
    return np.stack(fr)


def oracle_packed(shape, img, runner=None):
    """Per-channel oracle of one packed image [sh, sw, C] -> [dh, dw, C]."""
    m, d, sw, sh, dw, dh, px = shape
    run = runner or ol.run_oracle
    return np.stack([run(m, d, sw, sh, dw, dh, px, np.ascontiguousarray(img[:, :, c])) for c in range(img.shape[2])],
                    axis=2)


@functools.lru_cache(maxsize=None)
def _expected(shape, C, n):
    out = np.stack([oracle_packed(shape, f) for f in frames_for(shape, C, n)])
    out.setflags(write=False)
    return out


def expected_for(shape, C, n=2):
    """Oracle results of frames_for(shape, C, n), computed once per session and read-only."""
    return _expected(tuple(shape), C, n)


# ---- every packed_tile_kernel<C, NP, LZ> instantiation, and the tile shapes
#
# Rows of (shape, C, CT, TH, NP): CT x TH is the tile (output pixels x output rows, plan.cpp
# build_packed_tables), NP the horizontal tap pairs (build_tile_tables); LZ is shape[0] == "lanczos".
# The geometry is written out as literals: tests/test_packed_host.py checks it against the host
# tables, tests/test_packed_gpu.py against describe().  Found once by a seeded search on the CPU
# through tests/native/packed_emul.cpp (source rows <= 48, output <= 40 x 32, non-identity Y ratio,
# no Lanczos shape the plan rejects, no Linear upscale above 2x, and the oracle maps const_frame
# to its constants in every pixel), never searched at test time.
TILE_NP = (1, 2, 3, 4, 5, 6, 7, 8, 10, 12, 16)  # plan.hpp kTileNP, restated (the host test compares the two)

# one row per (C, NP, LZ): 3 x 11 x 2 = 66
INSTANTIATIONS = [
    (("lanczos", 2, 9, 39, 9, 19, 1), 2, 128, 16, 1),
    (("lanczos", 4, 8, 28, 8, 16, 2), 3, 64, 16, 1),
    (("lanczos", 4, 13, 15, 13, 12, 2), 4, 64, 16, 1),
    (("lanczos", 1, 17, 16, 21, 19, 1), 2, 128, 16, 2),
    (("lanczos", 1, 11, 12, 12, 15, 2), 3, 64, 16, 2),
    (("lanczos", 1, 22, 16, 29, 30, 2), 4, 64, 16, 2),
    (("lanczos", 2, 17, 29, 27, 10, 1), 2, 128, 16, 3),
    (("lanczos", 2, 14, 39, 16, 19, 1), 3, 64, 16, 3),
    (("lanczos", 2, 23, 25, 13, 29, 2), 4, 64, 16, 3),
    (("lanczos", 3, 66, 15, 32, 9, 2), 2, 128, 16, 4),
    (("lanczos", 3, 28, 14, 31, 19, 1), 3, 64, 16, 4),
    (("lanczos", 3, 12, 32, 20, 5, 2), 4, 64, 16, 4),
    (("lanczos", 4, 8, 15, 5, 32, 2), 2, 128, 16, 5),
    (("lanczos", 1, 35, 25, 9, 19, 1), 3, 64, 16, 5),
    (("lanczos", 2, 23, 25, 14, 22, 1), 4, 64, 16, 5),
    (("lanczos", 5, 10, 19, 12, 21, 1), 2, 128, 16, 6),
    (("lanczos", 2, 75, 33, 33, 28, 1), 3, 64, 16, 6),
    (("lanczos", 4, 24, 13, 20, 8, 1), 4, 64, 16, 6),
    (("lanczos", 4, 45, 13, 31, 23, 1), 2, 128, 16, 7),
    (("lanczos", 1, 66, 32, 11, 6, 1), 3, 64, 16, 7),
    (("lanczos", 6, 17, 40, 24, 31, 1), 4, 64, 16, 7),
    (("lanczos", 2, 58, 26, 9, 13, 2), 2, 128, 16, 8),
    (("lanczos", 3, 49, 36, 21, 6, 1), 3, 64, 16, 8),
    (("lanczos", 6, 27, 12, 24, 15, 1), 4, 64, 16, 8),
    (("lanczos", 9, 9, 38, 13, 16, 2), 2, 128, 16, 10),
    (("lanczos", 5, 22, 21, 13, 22, 1), 3, 64, 16, 10),
    (("lanczos", 1, 156, 28, 20, 25, 1), 4, 64, 16, 10),
    (("lanczos", 3, 274, 18, 27, 17, 2), 2, 128, 16, 12),
    (("lanczos", 1, 190, 30, 20, 20, 1), 3, 64, 16, 12),
    (("lanczos", 3, 90, 23, 29, 26, 1), 4, 64, 16, 12),
    (("lanczos", 2, 161, 16, 29, 20, 1), 2, 128, 16, 16),
    (("lanczos", 9, 44, 25, 29, 28, 1), 3, 64, 16, 16),
    (("lanczos", 8, 39, 23, 25, 28, 1), 4, 64, 16, 16),
    (("area", 0, 8, 24, 9, 5, 1), 2, 128, 16, 1),
    (("linear", 0, 52, 14, 13, 17, 1), 3, 64, 16, 1),
    (("area", 0, 8, 15, 11, 10, 1), 4, 64, 16, 1),
    (("linear", 0, 22, 15, 12, 20, 1), 2, 128, 16, 2),
    (("area", 0, 41, 29, 20, 31, 1), 3, 64, 16, 2),
    (("linear", 0, 15, 19, 20, 27, 1), 4, 64, 16, 2),
    (("area", 0, 71, 22, 19, 14, 1), 2, 128, 16, 3),
    (("area", 0, 29, 39, 7, 28, 1), 3, 64, 16, 3),
    (("area", 0, 89, 28, 22, 15, 1), 4, 64, 16, 3),
    (("area", 0, 158, 23, 29, 20, 1), 2, 128, 16, 4),
    (("area", 0, 143, 13, 27, 27, 1), 3, 64, 16, 4),
    (("area", 0, 28, 20, 5, 18, 1), 4, 64, 16, 4),
    (("area", 0, 106, 25, 14, 7, 1), 2, 128, 16, 5),
    (("area", 0, 134, 38, 17, 24, 1), 3, 64, 16, 5),
    (("area", 0, 172, 12, 24, 29, 1), 4, 64, 16, 5),
    (("area", 0, 58, 20, 6, 15, 1), 2, 128, 16, 6),
    (("area", 0, 196, 32, 21, 7, 1), 3, 64, 16, 6),
    (("area", 0, 144, 31, 15, 26, 1), 4, 64, 16, 6),
    (("area", 0, 252, 22, 25, 13, 1), 2, 128, 16, 7),
    (("area", 0, 197, 18, 17, 31, 1), 3, 64, 16, 7),
    (("area", 0, 131, 24, 12, 10, 1), 4, 64, 16, 7),
    (("area", 0, 180, 26, 13, 12, 1), 2, 128, 16, 8),
    (("area", 0, 443, 31, 32, 12, 1), 3, 64, 4, 8),
    (("area", 0, 125, 17, 10, 10, 1), 4, 64, 16, 8),
    (("area", 0, 129, 13, 8, 19, 1), 2, 128, 16, 10),
    (("area", 0, 166, 18, 10, 32, 1), 3, 64, 16, 10),
    (("area", 0, 379, 23, 25, 8, 1), 4, 64, 4, 10),
    (("area", 0, 204, 28, 11, 6, 1), 2, 128, 16, 12),
    (("area", 0, 111, 36, 6, 18, 1), 3, 64, 16, 12),
    (("area", 0, 190, 36, 9, 28, 1), 4, 64, 16, 12),
    (("area", 0, 238, 30, 9, 31, 1), 2, 128, 16, 16),
    (("area", 0, 147, 31, 6, 8, 1), 3, 64, 16, 16),
    (("area", 0, 352, 26, 11, 16, 1), 4, 64, 8, 16),
]

# tile shapes: every CT in {64, 128, 256, 512} with >= 2 column tiles, a partial last one and
# dstW % 4 != 0 (wide rows, a few output rows tall); every TH in {2, 4, 8, 16} with >= 2 row tiles
# and a partial last one (deep ratios, narrow).  TH < 16 needs a source window that outgrows LDS,
# which only a deep downscale gives; the upscales with two row tiles have TH = 16.
GEOMETRY = [
    (("area", 0, 242, 7, 538, 9, 1), 4, 256, 16, 1),
    (("linear", 0, 300, 7, 538, 9, 1), 2, 256, 16, 2),
    (("area", 0, 242, 7, 538, 9, 1), 2, 512, 16, 1),
    (("area", 0, 120, 9, 270, 7, 1), 3, 128, 16, 1),
    (("lanczos", 2, 160, 11, 267, 8, 2), 2, 256, 16, 3),
    (("lanczos", 3, 250, 11, 278, 8, 1), 3, 128, 16, 4),
    (("area", 0, 230, 12, 150, 7, 1), 2, 128, 16, 2),
    (("linear", 0, 278, 6, 214, 5, 1), 4, 64, 16, 2),
    (("lanczos", 2, 90, 22, 150, 37, 1), 2, 128, 16, 3),
    (("lanczos", 2, 90, 22, 150, 37, 1), 4, 64, 16, 3),
    (("area", 0, 844, 190, 141, 31, 1), 2, 128, 2, 4),
    (("lanczos", 1, 735, 142, 99, 25, 1), 4, 64, 2, 10),
    (("area", 0, 529, 34, 106, 7, 1), 3, 64, 4, 4),
    (("lanczos", 1, 864, 33, 146, 19, 2), 2, 128, 4, 7),
    (("lanczos", 5, 257, 82, 77, 27, 2), 4, 64, 8, 8),
    (("area", 0, 605, 108, 111, 36, 1), 3, 64, 8, 4),
    (("linear", 0, 180, 52, 65, 19, 1), 3, 64, 16, 2),
    (("lanczos", 1, 258, 100, 126, 38, 1), 4, 64, 16, 4),
]

# Lanczos upscales above 2x, the only Lanczos shapes with CT = 512 at C = 2 and CT = 256 at C = 4
# (1080p -> 4K, the UV plane of an NV12 upscale).  They are kept out of GEOMETRY because the
# reference itself does not keep a constant there: the last column's valid taps sum to den <= 8192
# of 16384 (its centre lies more than half a source pixel past the last source column), and
# resizeXborder's rounding term gives trunc(8192 / den) >= 1 for the constant 0.  Same checks
# otherwise; the constant frame is compared with the oracle.
LANCZOS_WIDE_UPSCALES = [
    (("lanczos", 3, 200, 8, 521, 9, 1), 2, 512, 16, 4),
    (("lanczos", 3, 200, 8, 521, 9, 1), 4, 256, 16, 4),
]

# Lanczos shapes whose top border rows exceed dstH (ol.lanczos_rows_defined is False): every plan
# constructor rejects them, and neither the oracle nor the reference is ever run on them.
REJECTED = [("lanczos", 8, 115, 18, 16, 6, 1), ("lanczos", 9, 57, 39, 12, 3, 2)]


def cell_id(row):
    shape, C, CT, TH, NP = row
    return "c%d-np%d-%s-ct%d-th%d-%s" % (C, NP, "lz" if shape[0] == "lanczos" else "al", CT, TH, sid(shape))


CONST_CHANNELS = (0, 255, 1, 254)


def const_frame(shape, C):
    """[sh, sw, C]: channel c is the constant CONST_CHANNELS[c]; so must every output pixel be
    (the taps of every formula sum to their bias), and a wrong byte selector shows as cross-talk."""
    _, _, sw, sh, _, _, _ = shape
    return np.broadcast_to(np.array(CONST_CHANNELS[:C], np.uint8), (sh, sw, C)).copy()
