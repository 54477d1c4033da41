"""Block-shared Lanczos 2:1 streamer: folded Y taps, single DMA form, one-round-trip band start.

Where one outer tap of the Y table is twice its neighbour (Lanczos-3: 1 -2 -4 9 28, Lanczos-4:
1 2 -3 -5 9 28) the vertical pass adds the two pair sums as X = P + 2 P' with 32-bit adds on packed
u16 halves and multiplies once.  The frames below drive every tap alone (one frame per window phase:
rows = phase (mod NY) at 255, the rest 0), drive X to its maximum of 1530 (255 exactly on the rows of
the folded pairs of the windows that start every NY rows) and its counterpart (the complement), and
add flat 0, flat 255 and two noise frames.  Lanczos-2 has no such tap pair and runs the same frames
through the unfolded pass as a control.

Shapes are the smallest the planner gives the streamer (found as test_stream_ring_gpu._bands_for
does): 512 -> 256 columns is the smallest line-scheme row, 496 -> 248 the narrow-row edge scheme,
2000 -> 1000 has a last DMA chunk masked to 62 lanes (ring rows packed: Lanczos-3 / -4) and a third
wave without a chunk (DMA sink).  Bands: the fewest bands of 2K+1 rows (no multiple of NY/2: a partial
last trip) and an even count of bands of K-2 rows (shorter than the K-1 prologue DMA iterations, so
some fall past the band end; odd bands walk upwards).  The whole output is compared bit for bit with
the oracle, the top and bottom border rows (divided after the fold) included."""
import numpy as np
import pytest

import oracle_lib as ol

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

if not torch.cuda.is_available():  # pragma: no cover - CPU container
    pytest.skip("needs a GPU", allow_module_level=True)

import libiqo_amd  # noqa: E402

DEV = torch.device("cuda:0")

NY = {2: 8, 3: 10, 4: 12}       # Y taps of the 2:1 tables
K = {2: 4, 3: 5, 4: 5}          # ring depth at the default prefetch (prep_lanczos)
FOLDQ = {2: 1, 3: 1, 4: 0}      # first pair of the fold (Lanczos-2: the same rows as Lanczos-3, unfolded)
WIDTHS = {"line": (512, 256), "narrow": (496, 248), "masked": (2000, 1000)}


def _bands_for(d, sw, dw, n, parity):
    """Fewest bands of n rows (a multiple of `parity`) whose frame the planner gives to the streamer."""
    for b in range(parity, 64, parity):
        try:
            if libiqo_amd.host_kernel_for("lanczos", d, sw, 2 * n * b, dw, n * b) == "lanczos_stream":
                return b
        except libiqo_amd.IqoError:
            pass
    raise AssertionError(("no streamer shape", d, sw, dw, n))


def _off_y(d):
    """First source row of output row 0's trimmed Y window (negative: above the image)."""
    s0, rows = libiqo_amd.host_band_src_rows("lanczos", d, 3840, 2160, 1920, 1080, 1, 100, 1)
    off = s0 - 200 + (rows - NY[d]) // 2  # the untrimmed window has (rows - NY) / 2 zero taps per end
    assert off == 1 - NY[d] // 2, (d, s0, rows)
    return off


def _frames(d, sw, sh):
    ny, q, off = NY[d], FOLDQ[d], _off_y(d)
    tap = (np.arange(sh) - off) % ny  # tap index of each row in the windows that start every NY rows
    out = [ol.gen("flat0", sw, sh), ol.gen("flat255", sw, sh)]
    for phase in range(ny):
        f = np.zeros((sh, sw), dtype=np.uint8)
        f[np.arange(sh) % ny == phase] = 255
        out.append(f)
    pairs = np.isin(tap, [q, q + 1, ny - 2 - q, ny - 1 - q])
    f = np.zeros((sh, sw), dtype=np.uint8)
    f[pairs] = 255
    out += [f, 255 - f]
    out += [ol.gen("noise", sw, sh, 9100 + d), ol.gen("noise", sw, sh, 9200 + d)]
    # (a checkerboard on top keeps the frame count odd: a batch of 16 would put each XCD's last frame
    # in shorter tail bands than the ones this test asks for)
    out.append(ol.gen("checker", sw, sh))
    assert len(out) % 8
    return np.stack(out)


@pytest.mark.parametrize("band", ["one_long", "even_short"])
@pytest.mark.parametrize("width", sorted(WIDTHS))
@pytest.mark.parametrize("d", [2, 3, 4])
def test_fold_frames_bit_exact(d, width, band):
    sw, dw = WIDTHS[width]
    n, parity = (2 * K[d] + 1, 1) if band == "one_long" else (K[d] - 2, 2)
    assert n % (NY[d] // 2) and (band == "one_long" or n < K[d] - 1)
    assert libiqo_amd.host_lanczos_yfold("lanczos", d, 3840, 2160, 1920, 1080) == (d != 2)
    bands = _bands_for(d, sw, dw, n, parity)
    sh, dh = 2 * n * bands, n * bands
    src = _frames(d, sw, sh)
    r = libiqo_amd.make_resizer("lanczos", d, sw, sh, dw, dh, 1)
    assert r.describe()["kernel"] == "lanczos_stream", (d, sw, sh)
    assert libiqo_amd.host_lanczos_yfold("lanczos", d, sw, sh, dw, dh) == (d != 2)
    r.set_option("bands", bands)
    out = r.resize_tensor(torch.from_numpy(src).to(DEV)).cpu().numpy()
    assert r.describe()["bands"] == bands, (d, sw, sh, bands)
    for f in range(src.shape[0]):
        exp = ol.run_oracle("lanczos", d, sw, sh, dw, dh, 1, src[f])
        bad = np.argwhere(out[f] != exp)
        assert bad.size == 0, (d, width, band, bands, f, bad[:4].tolist())
