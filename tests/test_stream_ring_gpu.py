"""Block-shared Lanczos 2:1 streamer: ring refill order and per-row load policy.

The kernel keeps K ring slots, issues DMA(0) .. DMA(K-2) before the first output row and refills the
slot of iteration i-1 in iteration i; the band's first NY-2 walk rows (VGPR loads) and its last NY-2
(DMA iterations j >= n - (NY-2)/2) keep the default cache policy, every other DMA iteration is
nontemporal.  The cases below put the band length n on both sides of every one of those limits, in
both walk directions, at each row geometry, and relaunch a multi-band batch.  Every output is
compared bit for bit with the oracle.  A frame shorter than the Y window is not a streamer shape, so
a band of n rows is cut from the shortest frame of n-row bands that is one (_bands_for).

Which shapes run the block-shared body (prep_lanczos, exact 2:1, srcW % 16 == 0): a row takes
wpr = ceil(dstW / (8 np)) waves, np <= 62, and is block-shared for wpr <= 4, i.e. dstW <= 1984; the
ring row is 32 + 2 dstW bytes, DMA'd in chunks = ceil((16 + 2 dstW) / 1024) pieces, CPW =
ceil(chunks / wpr) per wave.  wpr = 1 .. 4 allows dstW <= 496 w, hence chunks <= w: CPW = 1 is the
only value prep_lanczos can reach (test_only_one_chunk_per_wave_is_reachable walks the arithmetic);
the CPW = 2 instantiations exist but no shape selects them.  Lanczos-5 runs only with the line edge
scheme (dstW >= 256, >= 16 lanes per wave), so its narrow-row case is the nearest line-scheme shape,
512 -> 256.  One-wave rows run with a single frame: two or more narrow frames take the frame-stacked
kernel, which has its own case."""
import numpy as np
import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")

NY = {2: 8, 3: 10, 4: 12, 5: 16}   # Y taps of the 2:1 tables
K = {2: 4, 3: 5, 4: 5, 5: 5}       # ring depth at the default prefetch (prep_lanczos)


def band_lengths(d):
    h = (NY[d] - 2) // 2  # DMA iterations that bring the rows shared with the next band
    return sorted({1, 2, h - 1, h, h + 1, K[d] - 1, K[d], K[d] + 1, 2 * K[d] + 1})


def _bands_for(d, sw, dw, n, parity):
    """Fewest bands of n rows (a multiple of `parity`) whose frame the planner gives to the streamer:
    frames shorter than the Y window run other kernels, so a short band is cut from the shortest
    frame that streams."""
    for b in range(parity, 64, parity):
        try:
            if libiqo_amd.host_kernel_for("lanczos", d, sw, 2 * n * b, dw, n * b) == "lanczos_stream":
                return b
        except libiqo_amd.IqoError:
            pass
    raise AssertionError(("no streamer shape", d, sw, dw, n))


def _check(d, sw, dw, n, parity, frames, seed):
    """`frames` frames of sw -> dw columns in bands of exactly n rows: the fewest bands the streamer
    takes, one band where it can (parity 1) or an even count (parity 2: as many bands walk upwards
    as downwards)."""
    bands = _bands_for(d, sw, dw, n, parity)
    sh, dh = 2 * n * bands, n * bands
    src = np.stack([ol.gen("noise", sw, sh, seed + f) for f in range(frames)])
    src[-1, :, : sw // 5] = 255
    r = libiqo_amd.make_resizer("lanczos", d, sw, sh, dw, dh, 1)
    assert r.describe()["kernel"] == "lanczos_stream", (d, sw, sh)
    r.set_option("bands", bands)
    out = r.resize_tensor(torch.from_numpy(src).to(DEV)).cpu().numpy()
    assert r.describe()["bands"] == bands, (d, sw, sh, bands)
    for f in range(frames):
        exp = ol.run_oracle("lanczos", d, sw, sh, dw, dh, 1, src[f])
        bad = np.argwhere(out[f] != exp)
        assert bad.size == 0, (d, sw, dw, n, bands, f, bad[:4].tolist())


def test_only_one_chunk_per_wave_is_reachable():
    """prep_lanczos's chunks / wpr arithmetic over every block-shared width: CPW is always 1."""
    for dw in range(8, 1985, 8):
        wpr = -(-dw // 496)
        lanes = (dw + 7) // 8
        np_ = min(-(-lanes // wpr), dw // 8)
        wpr = -(-dw // (8 * np_))
        row_need = (max(32 + 2 * dw, 16 + 2 * dw) + 15) & ~15
        chunks = (row_need - 16 + 1023) // 1024
        assert wpr <= 4 and -(-chunks // wpr) == 1, dw


@pytest.mark.parametrize("parity", [1, 2], ids=["fewest_bands", "even_bands"])
@pytest.mark.parametrize("d", [2, 3, 4, 5])
def test_band_length_against_ring_and_halo_depth(d, parity):
    """3840 -> 1920 columns (4 waves, 60 lanes each, line edge scheme; ring depth 5: a masked last
    chunk of 49 lanes) in bands of exactly n rows.  Odd bands walk upwards and share their other end."""
    for n in band_lengths(d):
        _check(d, 3840, 1920, n, parity, 2, 4000 + 100 * d + n)


# (srcW, dstW, frames): one wave; narrow-row edge scheme (Lanczos-5: nearest line-scheme shape);
# two waves for one chunk, so the second one DMAs into the sink (1000 -> 500 is no multiple of 16
# columns and runs the general kernel: 1008 -> 504 is the nearest streamer shape)
GEOMETRY = {"one_wave": (640, 320, 1), "narrow": (256, 128, 1), "sink": (1008, 504, 2)}


@pytest.mark.parametrize("geom", sorted(GEOMETRY))
@pytest.mark.parametrize("d", [2, 3, 4, 5])
def test_row_geometry(d, geom):
    sw, dw, frames = GEOMETRY[geom]
    if geom == "narrow" and d == 5:
        sw, dw = 512, 256
    for n in (K[d] + 1, 2 * K[d] + 1):
        for parity in (1, 2):
            _check(d, sw, dw, n, parity, frames, 5000 + 100 * d + n)


@pytest.mark.parametrize("d", [2, 3])
def test_frame_stacked_ring(d):
    """5 frames of 256 -> 128 columns sit side by side in one 2-wave workgroup (the frame-stacked
    kernel keeps the same ring schedule)."""
    for n in (K[d] + 1, 2 * K[d] + 1):
        _check(d, 256, 128, n, 2, 5, 6000 + 100 * d + n)


def test_fused_i420_shared_body():
    """I420 in one launch whose Y plane runs the block-shared body (4 waves per row)."""
    m, d, sw, sh, dw, dh = "lanczos", 3, 3840, 44, 1920, 22
    assert libiqo_amd.host_yuv420_fused(m, d, sw, sh, dw, dh) == "lz_symb10"
    cw, ch, cdw, cdh = sw // 2, sh // 2, dw // 2, dh // 2
    n = 2
    y = np.stack([ol.gen("noise", sw, sh, 7000 + f) for f in range(n)])
    u = np.stack([ol.gen("noise", cw, ch, 7010 + f) for f in range(n)])
    v = np.stack([ol.gen("noise", cw, ch, 7020 + f) for f in range(n)])
    src = torch.from_numpy(np.concatenate([y.reshape(n, -1), u.reshape(n, -1), v.reshape(n, -1)], axis=1)).to(DEV)
    out, fused = libiqo_amd.Yuv420Resizer(m, d, sw, sh, dw, dh).resize_frames(src)
    out = out.cpu().numpy()
    assert fused
    for f in range(n):
        assert (out[f, : dw * dh].reshape(dh, dw) == ol.run_oracle(m, d, sw, sh, dw, dh, 1, y[f])).all(), (f, "Y")
        assert (out[f, dw * dh: dw * dh + cdw * cdh].reshape(cdh, cdw) ==
                ol.run_oracle(m, d, cw, ch, cdw, cdh, 2, u[f])).all(), (f, "U")
        assert (out[f, dw * dh + cdw * cdh:].reshape(cdh, cdw) ==
                ol.run_oracle(m, d, cw, ch, cdw, cdh, 2, v[f])).all(), (f, "V")


def test_relaunch_fresh_outputs():
    """64 frames of 3840x48 -> 1920x24 in 3 bands, 20 launches into fresh outputs: a slot refilled
    before its last read shows as stray wrong pixels in some launch."""
    d, sw, sh, dw, dh, frames = 3, 3840, 48, 1920, 24, 64
    src = np.stack([ol.gen("noise", sw, sh, 8000 + f) for f in range(frames)])
    exp = torch.from_numpy(np.stack([ol.run_oracle("lanczos", d, sw, sh, dw, dh, 1, src[f]) for f in range(frames)])).to(DEV)
    r = libiqo_amd.make_resizer("lanczos", d, sw, sh, dw, dh, 1)
    assert r.describe()["kernel"] == "lanczos_stream"
    r.set_option("bands", 3)
    dsrc = torch.from_numpy(src).to(DEV)
    outs = [r.resize_tensor(dsrc) for _ in range(20)]
    torch.cuda.synchronize()
    for k, out in enumerate(outs):
        bad = torch.nonzero(out != exp)
        assert bad.numel() == 0, (k, bad[:4].tolist())
