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
