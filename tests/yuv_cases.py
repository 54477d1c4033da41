"""Shapes of the fused I420 tests (tests/test_yuv_host.py, tests/test_yuv_gpu.py): one row per
(method, degree, srcW, srcH, dstW, dstH, label), the label being the fused instantiation
libiqo_amd.host_yuv420_fused reports for the shape ("none": plane by plane).  Test
infrastructure only.

Every label of libiqo_amd.YUV420_FUSED has at least one row.  Heights are 16 .. 64 source rows:
what selects an instantiation is the row's width and the ratios, so the oracle costs milliseconds.
Every row keeps the tight I420 layout of Yuv420Resizer.resize_frames aligned for its kernels.
"""
import functools

import numpy as np

import oracle_lib as ol

LABELS = ["none", "lz_symb10", "lz_sym10", "lz_symb8", "lz_sym8", "area44", "area22", "area2y", "area4y", "area8y",
          "area33", "area3y", "area6y", "lin_d2", "lin_up2"]

CASES = [
    # Lanczos 2:1, Y block-shared: exactly 4 waves per row and at most 4 DMA chunks
    ("lanczos", 3, 3840, 48, 1920, 24, "lz_symb10"),   # 60 lanes per wave
    ("lanczos", 2, 3840, 48, 1920, 24, "lz_symb8"),
    ("lanczos", 3, 3008, 40, 1504, 20, "lz_symb10"),   # 47 lanes; 3 DMA chunks for 4 waves: one wave has none
    ("lanczos", 2, 3008, 40, 1504, 20, "lz_symb8"),
    ("lanczos", 3, 3968, 40, 1984, 20, "lz_symb10"),   # 62 lanes: the widest 4-wave row
    ("lanczos", 2, 3968, 40, 1984, 20, "lz_symb8"),
    ("lanczos", 3, 3840, 52, 1920, 26, "lz_symb10"),   # odd chroma output height (13)
    ("lanczos", 2, 3840, 52, 1920, 26, "lz_symb8"),
    # Lanczos 2:1, Y per-wave: any other wave count (1 .. 3 waves are block-shared when run alone)
    ("lanczos", 3, 4096, 32, 2048, 16, "lz_sym10"),    # 5 waves per row: a partial last 4-wave block
    ("lanczos", 2, 4096, 32, 2048, 16, "lz_sym8"),
    ("lanczos", 3, 2560, 40, 1280, 20, "lz_sym10"),    # 3 waves
    ("lanczos", 2, 2560, 40, 1280, 20, "lz_sym8"),
    ("lanczos", 3, 1920, 64, 960, 32, "lz_sym10"),     # 2 waves
    ("lanczos", 2, 1920, 64, 960, 32, "lz_sym8"),
    ("lanczos", 3, 640, 48, 320, 24, "lz_sym10"),      # 1 wave
    ("lanczos", 2, 640, 48, 320, 24, "lz_sym8"),
    ("lanczos", 3, 64, 32, 32, 16, "lz_sym10"),        # lanes = dstW / 8
    ("lanczos", 2, 64, 32, 32, 16, "lz_sym8"),
    ("lanczos", 3, 32, 32, 16, 16, "lz_sym10"),
    ("lanczos", 2, 32, 32, 16, 16, "lz_sym8"),
    # Area, integer ratios (area_kind 0 .. 7) and Linear 2:1 (kind 8)
    ("area", 0, 128, 16, 32, 4, "area44"),
    ("area", 0, 1088, 40, 272, 10, "area44"),          # 3 Y workgroups per frame, 1 per chroma plane
    ("area", 0, 128, 16, 64, 8, "area22"),
    ("area", 0, 128, 24, 64, 4, "area2y"),
    ("area", 0, 128, 16, 32, 8, "area4y"),
    ("area", 0, 256, 16, 32, 4, "area8y"),
    ("area", 0, 96, 24, 32, 8, "area33"),
    ("area", 0, 48, 24, 16, 8, "area33"),
    ("area", 0, 1056, 36, 352, 12, "area33"),
    ("area", 0, 96, 16, 32, 8, "area3y"),
    ("area", 0, 192, 24, 32, 4, "area6y"),
    ("area", 0, 2112, 36, 352, 6, "area6y"),
    ("linear", 0, 128, 16, 64, 8, "lin_d2"),
    ("linear", 0, 64, 8, 32, 4, "lin_d2"),
    ("linear", 0, 1088, 40, 544, 20, "lin_d2"),
    # Linear 2x
    ("linear", 0, 16, 2, 32, 4, "lin_up2"),            # chroma 8x1: one source row, one 8-column group
    ("linear", 0, 32, 6, 64, 12, "lin_up2"),
    ("linear", 0, 64, 8, 128, 16, "lin_up2"),
    ("linear", 0, 1008, 14, 2016, 28, "lin_up2"),
    # no fused form
    ("lanczos", 4, 3840, 48, 1920, 24, "none"),        # chroma takes another kernel family than Y
    ("lanczos", 5, 3840, 64, 1920, 32, "none"),
    ("lanczos", 3, 3840, 50, 1920, 25, "none"),        # chroma rows 25 -> 12: not 2:1
    ("lanczos", 3, 3856, 48, 1928, 24, "none"),
    ("linear", 0, 48, 6, 144, 18, "none"),             # Linear 3x
    ("lanczos", 3, 1920, 1080, 1280, 720, "none"),     # exact 3:2 kernel on Y
]


def cid(case):
    return "%s%d-%dx%d-%dx%d-%s" % case


def one_per_label():
    """The first row of every label, "none" included."""
    seen, out = set(), []
    for c in CASES:
        if c[6] not in seen:
            seen.add(c[6])
            out.append(c)
    return out


def chroma_shape(case):
    """(srcW, srcH, dstW, dstH, pxScale) of the U and V planes, as iqo_hip_plan_yuv420 builds them."""
    m, _, sw, sh, dw, dh, _ = case
    return sw // 2, sh // 2, dw // 2, dh // 2, 2 if m == "lanczos" else 1


N_FRAMES = 3
CONST = (16, 128, 235)  # frame 2: the Y, U and V planes are three different constants


@functools.lru_cache(maxsize=None)
def planes_for(case):
    """Inputs (Y [3, sh, sw], U, V [3, sh/2, sw/2]), read-only: frame 0 seeded noise, frame 1 noise with a
    flat band (255 over the upper half of V, 0 over the left third of Y), frame 2 three constants."""
    _, _, sw, sh, _, _, _ = case
    cw, ch = sw // 2, sh // 2
    y = np.stack([ol.gen("noise", sw, sh, 900 + f) for f in range(N_FRAMES)])
    u = np.stack([ol.gen("noise", cw, ch, 910 + f) for f in range(N_FRAMES)])
    v = np.stack([ol.gen("noise", cw, ch, 920 + f) for f in range(N_FRAMES)])
    v[1, : max(1, ch // 2)] = 255
    y[1, :, : max(1, sw // 3)] = 0
    y[2], u[2], v[2] = CONST
    for a in (y, u, v):
        a.setflags(write=False)
    return y, u, v


def oracle_planes(case, y, u, v):
    """Per-plane oracle of one frame."""
    m, d, sw, sh, dw, dh, _ = case
    cw, ch, cdw, cdh, px = chroma_shape(case)
    return (ol.run_oracle(m, d, sw, sh, dw, dh, 1, y), ol.run_oracle(m, d, cw, ch, cdw, cdh, px, u),
            ol.run_oracle(m, d, cw, ch, cdw, cdh, px, v))


@functools.lru_cache(maxsize=None)
def expected_for(case):
    """Oracle outputs (Y [3, dh, dw], U, V [3, dh/2, dw/2]) of planes_for(case), read-only."""
    y, u, v = planes_for(case)
    fr = [oracle_planes(case, y[f], u[f], v[f]) for f in range(N_FRAMES)]
    out = tuple(np.stack([fr[f][p] for f in range(N_FRAMES)]) for p in range(3))
    for a in out:
        a.setflags(write=False)
    return out
