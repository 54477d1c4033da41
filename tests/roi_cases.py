"""Shared cases of the batched crop-and-resize tests (tests/test_roi_host.py, tests/test_roi_gpu.py).
Test infrastructure only.

Frames are 3 x (160 x 120) of splitmix noise with up to 4 channels, the output is 32 x 24.  The expected
output of a box is the Generic oracle on the cropped channel plane, per channel (checked against the
reference's own build, by the CPU tests, where that exists and runs the shape clean); a flipped box expects the
same reversed along the columns.
Every box goes through oracle_lib.lanczos_rows_defined before the oracle is called on it.
"""
import functools
import os
import subprocess

import numpy as np

import oracle_lib as ol

FRAMES, FW, FH = 3, 160, 120
DW, DH = 32, 24
METHODS = (("lanczos", 2), ("lanczos", 3), ("lanczos", 5), ("area", 0), ("linear", 0))
CHANNELS = (1, 3, 4)

# (frame, x, y, w, h[, flip]).  x runs through 0..3 mod 4, which gives all four byte misalignments of the
# first pixel for C = 1 (x mod 4) and for C = 3 (3x mod 4); the frames' rows are multiples of 4 bytes.
BOXES = (
    (0, 0, 0, 32, 24),        # identity on both axes
    (0, 1, 3, 64, 48),        # exact 2:1, one phase
    (1, 2, 5, 45, 31),        # multi-phase down
    (1, 3, 7, 20, 13),        # up
    (2, 5, 11, 32, 61),       # X identity
    (2, 6, 40, 97, 24),       # Y identity, 3:1 in X
    (0, 7, 9, 7, 5),          # no main region (left out for Linear: above 2x)
    (2, 29, 20, 131, 100),    # about 4:1, 26 taps per axis at Lanczos-3; ends at the last frame's corner
    (1, 100, 50, 33, 25),
    (1, 150, 60, 1, 10),
    (0, 40, 2, 45, 50),       # the width of (45, 31), another height: shared X table
    (0, 9, 60, 50, 31),       # the height of (45, 31), another width: shared Y table
    (1, 2, 5, 45, 31, 1),     # the third box again, mirrored
    (0, 158, 118, 2, 2),      # frame 0's last two bytes of its last row
)
# the two shapes without a defined Lanczos result (rejected: IQO_HIP_EINVAL)
UNDEFINED = (("lanczos", 3, (0, 4, 4, 10, 1)), ("lanczos", 5, (0, 4, 4, 2, 2)))


def frames(C):
    """uint8 [3, 120, 160] (C = 1) or [3, 120, 160, C]; channel c is the same plane for every C."""
    full = ol.splitmix_bytes(FRAMES * FH * FW * 4, 20240).reshape(FRAMES, FH, FW, 4)
    return np.ascontiguousarray(full[..., 0] if C == 1 else full[..., :C])


def boxes(method, degree):
    """The case list of a method: what the library accepts and the oracle has an answer for."""
    out = []
    for b in BOXES:
        w, h = b[3], b[4]
        if method == "linear" and (DW > 2 * w or DH > 2 * h):
            continue
        if method == "lanczos" and not ol.lanczos_rows_defined(degree, h, DH):
            continue
        out.append(b)
    return out


@functools.lru_cache(maxsize=None)
def _ref_clean(method, degree, w, h, dw=DW, dh=DH):
    """False where the reference itself has no clean run of the shape -- a zero border denominator (it traps:
    several of the tiny Lanczos boxes) or reads past its source (Area at non-integer ratios) -- as its sanitizer
    build tells (the check of tests/test_oracle_golden.py).  Such boxes are pinned by the oracle alone."""
    exe = os.path.join(ol.REF_DIR, "ref_asan_check")
    if not os.path.exists(exe):
        return False
    r = subprocess.run([exe, str(ol.METHODS[method]), str(degree), str(w), str(h), str(dw), str(dh), "1"],
                       stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    return r.returncode == 0


@functools.lru_cache(maxsize=None)
def _plane(method, degree, c, frame, x, y, w, h):
    assert method != "lanczos" or ol.lanczos_rows_defined(degree, h, DH)
    crop = np.ascontiguousarray(frames(4)[frame, y:y + h, x:x + w, c])
    exp = np.array(ol.run_oracle(method, degree, w, h, DW, DH, 1, crop))
    exp.setflags(write=False)
    return exp


def check_reference(method, degree, C):
    """Where the reference's own build exists (ol.ref_available()): its result on every cropped box it runs clean
    equals the oracle's.  CPU tests only (the check runs a sanitizer build).  Returns the boxes compared."""
    n = 0
    for b in boxes(method, degree):
        f, x, y, w, h = b[:5]
        if not _ref_clean(method, degree, w, h):
            continue
        for c in range(C):
            crop = np.ascontiguousarray(frames(4)[f, y:y + h, x:x + w, c])
            assert np.array_equal(_plane(method, degree, c, f, x, y, w, h),
                                  ol.run_ref(method, degree, w, h, DW, DH, 1, crop)), (method, degree, c, b)
        n += 1
    return n


def expected(method, degree, C, box_list=None):
    """uint8 [N, 24, 32] (C = 1) or [N, 24, 32, C]: the oracle per box and channel, flipped where flagged."""
    box_list = boxes(method, degree) if box_list is None else box_list
    out = np.zeros((len(box_list), DH, DW, C), np.uint8)
    for i, b in enumerate(box_list):
        for c in range(C):
            p = _plane(method, degree, c, *b[:5])
            out[i, :, :, c] = p[:, ::-1] if len(b) == 6 and b[5] else p
    return out[..., 0] if C == 1 else out
