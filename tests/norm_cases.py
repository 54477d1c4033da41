"""Constants and the reference formula shared by the normalised float output tests
(tests/test_norm_host.py, tests/test_norm_gpu.py).  Test infrastructure only.

The reference needs no oracle of its own: plane p of the float output is, by definition
(include/iqo_hip.h iqo_hip_resize_device_norm),

    cvt(fl32(fl32(float(u8[..., order[p]]) * scale[p]) + bias[p]))

of the bytes the packed U8 path produces, which tests/packed_cases.py already pins per channel.  numpy's
float32 arithmetic rounds each operation on its own, which is the pinned two-rounding form.
"""
import numpy as np

MEAN = (0.485, 0.456, 0.406, 0.5)
STD = (0.229, 0.224, 0.225, 0.25)
# (v / 255 - mean) / std as v * scale + bias; rounded to float32 once, here
NORM_SCALE = tuple(np.float32(1.0 / (255.0 * s)) for s in STD)
NORM_BIAS = tuple(np.float32(-m / s) for m, s in zip(MEAN, STD))

OUT_F32, OUT_F16, OUT_BF16 = 1, 2, 3  # IQO_OUT_*
DTYPES = ("float32", "float16", "bfloat16")
CODE = {"float32": OUT_F32, "float16": OUT_F16, "bfloat16": OUT_BF16}
ELEM = {"float32": 4, "float16": 2, "bfloat16": 2}


def affine_f32(u8, scale, bias):
    """float32(u8) * scale + bias with two float32 roundings."""
    return u8.astype(np.float32) * np.float32(scale) + np.float32(bias)


def fma_f32(u8, scale, bias):
    """The same with ONE rounding (what a fused multiply-add gives): float64 holds a byte times a
    float32 plus a float32 of these magnitudes exactly, and float64 -> float32 rounds once."""
    exact = u8.astype(np.float64) * np.float64(np.float32(scale)) + np.float64(np.float32(bias))
    return exact.astype(np.float32)


def bf16_bits(f32):
    """Round-to-nearest-even float32 -> bfloat16 bit patterns (int16), by torch on the CPU."""
    import torch
    t = torch.from_numpy(np.ascontiguousarray(f32)).to(torch.bfloat16)
    return t.view(torch.int16).numpy()


def to_bits(f32, dtype):
    """Bit patterns of cvt(f32): int32 for float32, int16 for the two half types."""
    if dtype == "float32":
        return np.ascontiguousarray(f32).view(np.int32)
    if dtype == "float16":
        return np.ascontiguousarray(f32.astype(np.float16)).view(np.int16)
    return bf16_bits(f32)


def expected_bits(u8, order, scale, bias, dtype):
    """u8 [F, H, W, C] (the U8 path's bytes) -> bit patterns [F, planes, H, W] of the float output."""
    planes = [affine_f32(u8[..., c], s, b) for c, s, b in zip(order, scale, bias)]
    return to_bits(np.stack(planes, axis=1), dtype)
