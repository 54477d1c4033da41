"""Folded Y taps of the block-shared Lanczos 2:1 streamer, host side (no GPU).

The host picks the folded vertical pass from the plan's own table (iqo_host_lanczos_yfold): an outer
tap that is twice its neighbour, as u16 values -- c2 == 2 c1 in the 10-tap window, c1 == 2 c0 in the
12-tap one.  The predicate is checked against the oracle's Y table for every 2:1 degree, and the
folded expression, X = P + 2 P' built with 32-bit adds on packed u16 halves and multiplied once, is
checked against the plain per-tap sum modulo 2^16 in both halves."""
import numpy as np
import pytest

import libiqo_amd
import oracle_lib as ol

SHAPE = (3840, 2160, 1920, 1080)


def _trimmed_y(d):
    t = ol.oracle_tables("lanczos", d, *SHAPE, 1, 1)
    assert t.shape[0] == 1
    t = [int(v) for v in t[0]]
    while t and t[0] == 0:
        t.pop(0)
    while t and t[-1] == 0:
        t.pop()
    return t


def _fold_pair(t):
    """First pair of the fold for a window of len(t) taps, None for windows that do not fold."""
    return {10: 1, 12: 0}.get(len(t))


def _doubles(t):
    q = _fold_pair(t)
    return q is not None and (t[q + 1] & 0xffff) == ((2 * t[q]) & 0xffff)


@pytest.mark.parametrize("d", range(1, 10))
def test_predicate_matches_the_table(d):
    t = _trimmed_y(d)
    assert libiqo_amd.host_lanczos_yfold("lanczos", d, *SHAPE) == _doubles(t), (d, t)


def test_known_tables():
    """The tables the fold was written for (and the unfolded control)."""
    assert _trimmed_y(3) == [1, -2, -4, 9, 28, 28, 9, -4, -2, 1]
    assert _trimmed_y(4)[:6] == [1, 2, -3, -5, 9, 28]
    assert _doubles(_trimmed_y(3)) and _doubles(_trimmed_y(4)) and not _doubles(_trimmed_y(2))


def test_other_methods_and_kernels_do_not_fold():
    assert not libiqo_amd.host_lanczos_yfold("area", 0, *SHAPE)
    assert not libiqo_amd.host_lanczos_yfold("lanczos", 3, 3840, 2160, 1280, 720)  # 3:1
    assert not libiqo_amd.host_lanczos_yfold("lanczos", 3, 1920, 1080, 3840, 2160)  # upscale


def _pk(lo, hi):
    return (lo.astype(np.uint32) | (hi.astype(np.uint32) << np.uint32(16))).astype(np.uint32)


def _pk_mad(a, c, acc):
    """v_pk_mad_u16: per u16 half a * c + acc, modulo 2^16."""
    c = np.uint32(c & 0xffff)
    lo = ((a & np.uint32(0xffff)) * c + (acc & np.uint32(0xffff))) & np.uint32(0xffff)
    hi = ((a >> np.uint32(16)) * c + (acc >> np.uint32(16))) & np.uint32(0xffff)
    return (lo | (hi << np.uint32(16))).astype(np.uint32)


@pytest.mark.parametrize("d", [3, 4])
def test_folded_sum_equals_plain_sum(d):
    t = _trimmed_y(d)
    ny, h, q = len(t), len(t) // 2, _fold_pair(t)
    assert _doubles(t)
    rng = np.random.default_rng(800 + d)
    n = 100000
    rows = rng.integers(0, 256, size=(ny, 2, n + 2), dtype=np.uint32)
    rows[:, :, n] = 0
    rows[:, :, n + 1] = 255
    win = [_pk(rows[k, 0], rows[k, 1]) for k in range(ny)]  # packed u16 pairs, as the window registers
    with np.errstate(over="ignore"):
        pair = [(win[p] + win[ny - 1 - p]).astype(np.uint32) for p in range(h)]  # 32-bit adds
        plain = np.zeros(n + 2, dtype=np.uint32)
        for p in range(h):
            plain = _pk_mad(pair[p], t[p], plain)
        x = (pair[q] + ((pair[q + 1] << np.uint32(1)).astype(np.uint32))).astype(np.uint32)  # add_lshl, add3
        assert int((x & np.uint32(0xffff)).max()) == 1530 and int((x >> np.uint32(16)).max()) == 1530
        folded = np.zeros(n + 2, dtype=np.uint32)
        for p in range(q):
            folded = _pk_mad(pair[p], t[p], folded)
        folded = _pk_mad(x, t[q], folded)
        for p in range(q + 2, h):
            folded = _pk_mad(pair[p], t[p], folded)
    assert np.array_equal(folded & np.uint32(0xffff), plain & np.uint32(0xffff))
    assert np.array_equal(folded >> np.uint32(16), plain >> np.uint32(16))
