"""The seeded CPU search that found the rows of tests/instance_cases.py.  Run once, by hand; never at test time:

    IQO_HIP_TUNING=1 python tests/instance_search.py [samples per worker] [workers]  > rows.txt

It draws small shapes and option sets at random, asks the library's host query (libiqo_amd.host_instance_for)
which template instantiation each would run, and keeps for every instantiation the smallest hit by
sw * sh + dw * dh (ties: fewer options, then the first found).  Worker k draws from random.Random(SEED + k), a
fixed number of samples each, so a run is reproducible; the committed table came from the defaults below.
Shapes without a pinned answer are never kept (instance_cases.pinned_answer).  It prints the rows as Python
literals, then the instantiations of the library's enumeration it did not reach.

Three modes share the samples: the ratio kernels with their tuning options (ryx, ryg, ryu), the tile kernel
(walker and ratio kernels switched off) and the walker (ratio kernels switched off).  The exact-ratio
families are not searched: their rows are the smallest shapes of the parity tests' own lists
(instance_cases.EXACT).
"""
import multiprocessing
import random
import sys

import conftest  # noqa: F401  (sys.path, IQO_HIP_TUNING)
import instance_cases as ic
import libiqo_amd

SEED = 20
SAMPLES = 400000   # per worker
WORKERS = 8
# search bounds: source <= 512 x 160, destination <= 512 x 320.  From below: 16 output rows and columns at least, so
# that a frame has rows past the first unrolled trip of every kernel (12 output rows at most), more columns than
# one thread takes, and distinct cuts for the GPU test's 3 bands and row-band windows
SW, SH, DW, DH = (16, 512), (8, 160), (16, 512), (16, 320)
# tile NP 16 of Area / Linear needs columns shrinking by more than 23: the tile mode also draws wider sources, in case
# none within the bound reaches it (one does: every committed row is within the bound, tests/test_instance_host.py)
WIDE_SW = (8, 1024)

RATIO_OFF, TILE_ONLY = ic.RATIO_OFF, ic.TILE_ONLY
# exact row ratios of ryx_kernel (P, Q)
RYX_ROWS = ((9, 4), (4, 1), (2, 1), (4, 9))


def log_int(rng, lo, hi):
    """An integer in lo .. hi, small values as likely as large ones."""
    import math
    return min(hi, max(lo, int(round(math.exp(rng.uniform(math.log(lo), math.log(hi + 1)))))))


def ratio_options(rng):
    o = []
    if rng.random() < 0.35:
        o.append(("ryg_cpt", rng.choice((2, 3, 4))))
    if rng.random() < 0.25:
        o.append(("ryx_split", rng.choice((0, 2, 3, 4))))
    for key in ("ryx_adj", "ryx_uc", "ryx_cpt", "ryu", "ryu_run"):
        if rng.random() < 0.12:
            o.append((key, 0))
    return tuple(o)


def draw(rng):
    """(method, degree, sw, sh, dw, dh, px, options)."""
    mode = rng.choice(("ratio", "ratio", "tile", "walk"))
    method = rng.choice(("lanczos", "lanczos", "lanczos", "area", "area", "linear"))
    degree = rng.randint(1, 9) if method == "lanczos" else 0
    px = rng.choice((1, 1, 2)) if method == "lanczos" else 1
    sw, sh = log_int(rng, *SW), log_int(rng, *SH)
    if mode == "tile" and method != "lanczos" and rng.random() < 0.2:
        sw = log_int(rng, 256, WIDE_SW[1])
    how = rng.random()
    if how < 0.5:       # both axes by about the same ratio (the walker needs that)
        r = 2.0 ** rng.uniform(-1.6, 4.0)
        dw = int(round(sw / (r * rng.uniform(0.8, 1.25))))
        dh = int(round(sh / (r * rng.uniform(0.9, 1.1))))
    else:
        dw, dh = log_int(rng, *DW), log_int(rng, *DH)
    if mode == "ratio" and rng.random() < 0.4:  # an exact row ratio
        p, q = rng.choice(RYX_ROWS)
        k = rng.randint(-(-DH[0] // q), max(-(-DH[0] // q), min(SH[1] // p, DH[1] // q)))
        sh, dh = p * k, q * k
        if rng.random() < 0.4:  # ... and columns at exactly 2:1 (uniform column coefficients)
            sw &= ~1
            dw = sw // 2
    dw, dh = min(max(dw, DW[0]), DW[1]), min(max(dh, DH[0]), DH[1])
    opts = ratio_options(rng) if mode == "ratio" else TILE_ONLY if mode == "tile" else RATIO_OFF
    return method, degree, sw, sh, dw, dh, px, opts


def key_of(inst):
    return tuple(sorted(inst.items()))


def worker(args):
    seed, samples = args
    rng = random.Random(seed)
    best = {}
    for _ in range(samples):
        method, degree, sw, sh, dw, dh, px, opts = draw(rng)
        if method == "linear" and (dw > 2 * sw or dh > 2 * sh):
            continue
        try:
            inst = libiqo_amd.host_instance_for(method, degree, sw, sh, dw, dh, px, opts)
        except libiqo_amd.IqoError:
            continue
        if inst["kernel"] not in ic.SEARCHED_KERNELS:
            continue
        score = (sw * sh + dw * dh, len(opts))
        k = key_of(inst)
        if k in best and best[k][0] <= score:
            continue
        if not ic.pinned_answer(method, degree, sw, sh, dw, dh, px):
            continue
        best[k] = (score, (method, degree, sw, sh, dw, dh, px, opts))
    return best


def main():
    samples = int(sys.argv[1]) if len(sys.argv) > 1 else SAMPLES
    workers = int(sys.argv[2]) if len(sys.argv) > 2 else WORKERS
    with multiprocessing.Pool(workers) as pool:
        parts = pool.map(worker, [(SEED + k, samples) for k in range(workers)])
    best = {}
    for part in parts:  # in worker order: a tie keeps the lower seed's
        for k, v in part.items():
            if k not in best or v[0] < best[k][0]:
                best[k] = v
    missing = []
    for family in ic.SEARCHED_FAMILIES:
        for inst in libiqo_amd.host_instances(family):
            k = key_of(inst)
            if k not in best:
                missing.append(inst)
                continue
            method, degree, sw, sh, dw, dh, px, opts = best[k][1]
            params = {a: b for a, b in inst.items() if a != "kernel"}
            o = "TILE_ONLY" if opts == TILE_ONLY else "RATIO_OFF" if opts == RATIO_OFF else repr(opts)
            print("    (%r, %r, %r, %d, %d, %d, %d, %d, %d, %s)," % (inst["kernel"], params, method, degree, sw, sh, dw, dh,
                                                                    px, o))
    print("# not reached: %d" % len(missing))
    for inst in missing:
        print("#   %r" % (inst,))


if __name__ == "__main__":
    main()
