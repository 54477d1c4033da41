"""Shapes, inputs and the expected value of the planar "resize to normalised tensors" tests
(tests/test_planes_norm_host.py, tests/test_planes_norm_gpu.py).  Test infrastructure only.

The expected value needs no oracle of its own: by definition (include/iqo_hip.h
iqo_hip_resize_planes_norm_device) output plane p is

    cvt(fl32(fl32(float(u8[f, order[p]]) * scale[p]) + bias[p]))

of the bytes the planar U8 path writes for source plane (f, order[p]), which is oracle_lib.run_oracle
plane by plane.  norm_cases supplies the two-rounding float32 arithmetic and the bit patterns; its
NORM_SCALE / NORM_BIAS are constants at which a fused multiply-add gives other bits
(tests/test_norm_host.py), and the noise frames below hold such bytes after the resize
(tests/test_planes_norm_host.py checks one shape).
"""
import functools

import numpy as np

import norm_cases as nc
import oracle_lib as ol

# (method, degree, srcW, srcH, dstW, dstH), the kernel family of its first pass with a 16-byte aligned
# layout (libiqo_amd.host_kernel_for), and what the second pass meets
SHAPES = [
    (("lanczos", 3, 64, 32, 32, 16), "lanczos_stream"),   # full groups only
    (("area", 0, 96, 24, 32, 8), "area_int"),             # full groups only
    (("linear", 0, 16, 2, 32, 4), "linear_up2"),          # 4 rows
    (("lanczos", 3, 40, 24, 20, 12), "ryx"),              # 8-pixel tail of 4; fp32 exact
    (("lanczos", 3, 40, 24, 27, 17), "ryg"),              # tails of 3 in both forms; odd row length
    (("area", 0, 384, 216, 320, 180), "walk"),            # many blocks
    (("lanczos", 3, 13, 9, 5, 40), "tile"),               # dstW 5: no full 8-group, one full 4-group + 1
    (("lanczos", 3, 7, 100, 3, 50), "general"),           # dstW 3: no full group in either form
]
BY_FAMILY = {family: shape for shape, family in SHAPES}
STREAM, RYX, RYG, TILE = (BY_FAMILY[k] for k in ("lanczos_stream", "ryx", "ryg", "tile"))

N_FRAMES = 2


def sid(shape):
    return "%s%d-%dx%d-%dx%d" % shape


@functools.lru_cache(maxsize=None)
def frames_for(shape, planes=3, frames=N_FRAMES):
    """Inputs [frames, planes, srcH, srcW], read-only: seeded noise, another seed per (frame, plane); frame 1
    has its left third set to 255 in plane 0 only, so a plane mix-up shows."""
    _, _, sw, sh, _, _ = shape
    out = np.stack([np.stack([ol.splitmix_bytes(sw * sh, 700 + 16 * f + c).reshape(sh, sw) for c in range(planes)])
                    for f in range(frames)])
    if frames > 1:
        out[1, 0, :, : max(1, sw // 3)] = 255
    out.setflags(write=False)
    return out


def oracle_planes(shape, src):
    """The U8 path's bytes [F, P, dstH, dstW] of src [F, P, srcH, srcW]: the oracle, plane by plane."""
    m, d, sw, sh, dw, dh = shape
    return np.stack([np.stack([ol.run_oracle(m, d, sw, sh, dw, dh, 1, pl) for pl in fr]) for fr in src])


@functools.lru_cache(maxsize=None)
def expected_u8(shape, planes=3, frames=N_FRAMES):
    """oracle_planes of frames_for(shape, planes, frames), read-only."""
    out = oracle_planes(shape, frames_for(shape, planes, frames))
    out.setflags(write=False)
    return out


def expected_bits(u8, order, scale, bias, dtype):
    """u8 [F, P, H, W] (the U8 path's bytes per source plane) -> bit patterns [F, len(order), H, W] of the float
    output; order[p] is the source plane of output plane p.  norm_cases.expected_bits takes channels last."""
    return nc.expected_bits(np.moveaxis(u8, 1, -1), order, scale, bias, dtype)
