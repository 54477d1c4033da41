"""The expected value and the shapes of the NV12 / I420 "resize to RGB" tests
(tests/test_yuvrgb_host.py, tests/test_yuvrgb_gpu.py).  Test infrastructure only.

The definition (include/iqo_hip.h, IQO_CS_*) is written once here, in numpy int32: with Y, U, V the
bytes of the per-plane oracle (yuv_cases.oracle_planes), chroma replicated to the output grid
(sample (min(y >> 1, ch - 1), min(x >> 1, cw - 1))), y' = Y - yOff, u = U - 128, v = V - 128,

    R = clamp255((cY y' + cRV v         + 8192) >> 14)
    G = clamp255((cY y' - cGU u - cGV v + 8192) >> 14)
    B = clamp255((cY y' + cBU u         + 8192) >> 14)

Float outputs are norm_cases.expected_bits of these bytes.

Inputs: the three frames of yuv_cases.planes_for (noise, noise with flat bands, the constants
16 / 128 / 235) and two clamp frames (clamp_frames below), through which every shape, however small or
however much its method averages, reaches both clamps in every channel.
"""
import functools

import numpy as np

import yuv_cases as yc

SHIFT = 14
# IQO_CS_*: (yOff, cY, cRV, cGU, cGV, cBU)
BT601_LIMITED, BT601_FULL, BT709_LIMITED, BT709_FULL = 0, 1, 2, 3
TABLE = {
    BT601_LIMITED: (16, 19077, 26149, 6419, 13320, 33050),
    BT601_FULL: (0, 16384, 22970, 5638, 11700, 29032),
    BT709_LIMITED: (16, 19077, 29372, 3494, 8731, 34610),
    BT709_FULL: (0, 16384, 25802, 3069, 7670, 30402),
}
STANDARDS = sorted(TABLE)
NAMES = {BT601_LIMITED: "bt601", BT601_FULL: "bt601-full", BT709_LIMITED: "bt709", BT709_FULL: "bt709-full"}
# the real coefficients the table rounds: (Kr, Kb, limited range)
REAL = {BT601_LIMITED: (0.299, 0.114, True), BT601_FULL: (0.299, 0.114, False),
        BT709_LIMITED: (0.2126, 0.0722, True), BT709_FULL: (0.2126, 0.0722, False)}

ORDERS = {"rgb": (0, 1, 2), "bgr": (2, 1, 0), "rgba": (0, 1, 2, 3), "bgra": (2, 1, 0, 3)}


def real_constants(standard):
    """(yOff, round(k 2^14) of cY, cRV, cGU, cGV, cBU) from the standard's Kr / Kb and range."""
    kr, kb, limited = REAL[standard]
    kg = 1.0 - kr - kb
    sy, sc = (255.0 / 219.0, 255.0 / 224.0) if limited else (1.0, 1.0)
    ks = (sy, 2.0 * (1.0 - kr) * sc, 2.0 * kb * (1.0 - kb) / kg * sc, 2.0 * kr * (1.0 - kr) / kg * sc,
          2.0 * (1.0 - kb) * sc)
    return (16 if limited else 0,) + tuple(int(round(k * (1 << SHIFT))) for k in ks)


def raw_rgb(standard, y, u, v):
    """The three shifted sums before the clamp, int32 [..., 3], of uint8 arrays of one shape."""
    yoff, cy, crv, cgu, cgv, cbu = (np.int32(c) for c in TABLE[standard])
    yy = y.astype(np.int32) - yoff
    uu, vv = u.astype(np.int32) - 128, v.astype(np.int32) - 128
    half = np.int32(1 << (SHIFT - 1))
    r = (cy * yy + crv * vv + half) >> SHIFT
    g = (cy * yy - cgu * uu - cgv * vv + half) >> SHIFT
    b = (cy * yy + cbu * uu + half) >> SHIFT
    return np.stack([r, g, b], axis=-1)


def yuv_to_rgb(standard, y, u, v):
    """uint8 [..., 3] (R, G, B)."""
    return np.clip(raw_rgb(standard, y, u, v), 0, 255).astype(np.uint8)


def replicate(c, dw, dh):
    """Chroma [F, ch, cw] on the output grid [F, dh, dw]: nearest, clamped at the last sample."""
    ch, cw = c.shape[-2:]
    rows = np.minimum(np.arange(dh) >> 1, ch - 1)
    cols = np.minimum(np.arange(dw) >> 1, cw - 1)
    return c[..., rows[:, None], cols[None, :]]


def planes_to_rgb(standard, y, u, v, raw=False):
    """Resized planes (Y [F, dh, dw]; U, V [F, dh/2, dw/2]) -> RGB [F, dh, dw, 3]."""
    dh, dw = y.shape[-2:]
    fn = raw_rgb if raw else yuv_to_rgb
    return fn(standard, y, replicate(u, dw, dh), replicate(v, dw, dh))


def reorder(rgb, order):
    """[..., 3] -> [..., len(order)]: byte c is order[c] of (R, G, B, 255)."""
    full = np.concatenate([rgb, np.full(rgb.shape[:-1] + (1,), 255, np.uint8)], axis=-1)
    return np.ascontiguousarray(full[..., list(order)])


# ---- shapes.  I420: yuv_cases.one_per_label() (every fused instantiation and "none"), the four standards
# dealt over the rows in turn (15 rows: each at least three times).
I420_CASES = [(c, STANDARDS[i % 4]) for i, c in enumerate(yc.one_per_label())]

# NV12: (method, degree, srcW, srcH, dstW, dstH), standard.  Small shapes at which yuv_rgb_kernel can go
# wrong: dstW of 2 and 3 (narrower than a thread's 8 pixels), dstW % 8 in {1, 4, 7} (tail stores), odd dstW
# and dstH (the chroma index clamp; dstW = 33: the clamped sample is in another thread's group), dstH = 2,
# several groups per row, an up-scale and a down-scale per method.
NV12_CASES = [
    (("lanczos", 3, 64, 32, 33, 17), BT709_LIMITED),    # odd x odd, dstW % 8 = 1, chroma 16 x 8
    (("lanczos", 2, 24, 16, 52, 36), BT601_FULL),       # up-scale, dstW % 8 = 4
    (("area", 0, 80, 48, 47, 23), BT601_LIMITED),       # odd x odd, dstW % 8 = 7
    (("area", 0, 16, 16, 2, 2), BT709_FULL),            # dstW = 2, dstH = 2: chroma 1 x 1
    (("area", 0, 12, 10, 30, 25), BT709_LIMITED),       # up-scale, odd dstH
    (("linear", 0, 16, 16, 3, 2), BT601_FULL),          # dstW = 3: chroma 1 x 1, the clamp in the first group
    (("linear", 0, 20, 12, 40, 24), BT709_FULL),        # up-scale 2x, whole groups only
    (("linear", 0, 64, 48, 36, 26), BT601_LIMITED),     # down-scale, dstW % 8 = 4
]


def nv12_case(shape):
    """The yuv_cases row of an NV12 shape (its planes and oracle are those of the I420 planes)."""
    return shape + ("nv12",)


def nid(row):
    shape, standard = row
    return "%s%d-%dx%d-%dx%d-%s" % (shape + (NAMES[standard],))


def iid(row):
    case, standard = row
    return "%s-%s" % (yc.cid(case), NAMES[standard])


N_FRAMES = yc.N_FRAMES + 2


def clamp_frames(case):
    """Two frames (Y [2, sh, sw]; U, V [2, sh/2, sw/2]) of flat patches, which survive any resize: Y is 0 on
    the left half and 255 on the right; U = V = 0 in the first frame (R and B fall below 0 at Y = 0, G
    passes 255 at Y = 255, in all four standards) and U = V = 255 in the second (G below 0, R and B above
    255).  Two frames, since a 2 x 2 output has one chroma sample per frame."""
    _, _, sw, sh, _, _, _ = case
    y = np.zeros((2, sh, sw), np.uint8)
    y[:, :, sw // 2:] = 255
    u = np.zeros((2, sh // 2, sw // 2), np.uint8)
    u[1] = 255
    return y, u, u.copy()


@functools.lru_cache(maxsize=None)
def planes_for(case):
    """Inputs (Y [5, sh, sw]; U, V [5, sh/2, sw/2]), read-only: yuv_cases.planes_for, then clamp_frames."""
    out = tuple(np.concatenate([a, b]) for a, b in zip(yc.planes_for(case), clamp_frames(case)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_planes(case):
    """Per-plane oracle outputs (Y [5, dh, dw]; U, V [5, dh/2, dw/2]) of planes_for(case), read-only."""
    y, u, v = clamp_frames(case)
    fr = [yc.oracle_planes(case, y[f], u[f], v[f]) for f in range(2)]
    out = tuple(np.concatenate([a, np.stack([fr[0][p], fr[1][p]])]) for p, a in enumerate(yc.expected_for(case)))
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expected_rgb(case, standard):
    """RGB bytes [5, dh, dw, 3] of planes_for(case) resized by the per-plane oracle; read-only."""
    y, u, v = expected_planes(case)
    out = planes_to_rgb(standard, y, u, v)
    out.setflags(write=False)
    return out


def nv12_frames(case):
    """planes_for(case) in the tight NV12 layout of Nv12Resizer.resize_frames: [5, bytes]."""
    y, u, v = planes_for(case)
    n = y.shape[0]
    uv = np.stack([u, v], axis=3)
    return np.ascontiguousarray(np.concatenate([y.reshape(n, -1), uv.reshape(n, -1)], axis=1))


def i420_frames(case):
    """... and in the tight I420 layout of Yuv420Resizer.resize_frames."""
    y, u, v = planes_for(case)
    n = y.shape[0]
    return np.ascontiguousarray(np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1))
