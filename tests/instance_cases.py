"""One small shape per template instantiation of the 1-channel resize kernels outside the integer-ratio
streamers (tests/test_instance_host.py, tests/test_instance_gpu.py).  Test infrastructure only.

ryx_kernel, ryg_kernel, ryu_kernel, tile_kernel, walk_kernel and the exact-ratio kernels (lanczos_up2 / d32 / d31 /
u23, linear_u23, area_d32) have 230 instantiations between them, each its own unrolled arithmetic.  Which one a
shape runs is decided by the plan (plan.cpp), the column split and options (abi.hip ryx_dev / ryg_dev) and the
families' instantiation tables (kernels.hip, kernels_ratio.hip); libiqo_amd.host_instance_for reports the
result without a GPU and Resizer.instance() for a live plan.  A row here is

    (kernel, parameters, method, degree, sw, sh, dw, dh, pxScale, options)

with `parameters` the instantiation's non-zero template parameters by name, written out as literals: the host
test checks them against the host query, the GPU test against the live plan before it launches anything.

SEARCHED was found once, on the CPU, by tests/instance_search.py (seed 20, 8 workers x 400000 samples; source 16 x 8
.. 512 x 160, destination 16 x 16 .. 512 x 320; the smallest hit by sw * sh + dw * dh), never searched at test time.  It
leaves out shapes without a pinned answer (pinned_answer below).  EXACT holds the exact-ratio kernels at the
smallest shapes the parity tests' own lists use (tests/test_gpu_parity.py *_SHAPES, tests/test_ratio_tables.py,
tests/extreme_cases.py), one row per prefetch depth that abi.hip's ratio_prefetch check lists; EXTRA their second
shapes at every depth again (rows beyond one per instantiation: same tests, not part of the count).
UNREACHABLE lists the instantiations no shape within the bounds runs, each with the plan rule that excludes it.
"""
import functools

import numpy as np

import extreme_cases as ec
import oracle_lib as ol

# options that leave the walker (the exact-ratio and general-row kernels off) / the tile kernel (the walker off too)
RATIO_OFF = tuple((k, 0) for k in ("a32", "d32", "d31", "ryx", "ryg", "up2", "u23", "l23"))
TILE_ONLY = (("walk", 0),) + RATIO_OFF
assert tuple(k for k, _ in TILE_ONLY) == ec.TILE_OPTIONS

# kernels of the search, and the library's families that hold them (ryu_kernel is part of the ryg family)
SEARCHED_KERNELS = ("ryx", "ryg", "ryu", "tile", "walk")
SEARCHED_FAMILIES = ("ryx", "ryg", "tile", "walk")
EXACT_FAMILIES = ("lanczos_up2", "lanczos_d32", "lanczos_d31", "lanczos_u23", "linear_u23", "area_d32")
FAMILIES = SEARCHED_FAMILIES + EXACT_FAMILIES
# instantiations per kernel (ryg family: 60 ryg_kernel + 30 ryu_kernel): 230 in all
COUNTS = {"ryx": 37, "ryg": 60, "ryu": 30, "tile": 22, "walk": 60, "lanczos_up2": 4, "lanczos_d32": 5, "lanczos_d31": 5,
          "lanczos_u23": 2, "linear_u23": 2, "area_d32": 3}

# The alignment (source, destination) each family's vector accesses need of base, row stride and frame stride
# (abi.hip kernel_align, restated: the GPU test asserts the live query at exactly these alignments)
ALIGN = {"walk": (4, 1), "lanczos_up2": (8, 16), "lanczos_d32": (4, 8), "lanczos_d31": (4, 4), "area_d32": (4, 8),
         "lanczos_u23": (8, 4), "linear_u23": (8, 4)}


def align_of(kernel):
    return ALIGN.get(kernel, (1, 1))


def _zero_border(tab, src_len, dst_len):
    """A border output of the axis whose taps inside the image sum to 0 (the reference divides by it)."""
    lo, phase, mb, me = ec.axis_geometry(tab, src_len, dst_len)
    nt = tab.shape[1]
    for d in list(range(0, mb)) + list(range(max(me, mb), dst_len)):
        s = lo[d] + np.arange(nt)
        if int(tab[phase[d]][(s >= 0) & (s < src_len)].sum()) == 0:
            return True
    return False


@functools.lru_cache(maxsize=None)
def pinned_answer(method, d, sw, sh, dw, dh, px):
    """False for the shapes the table leaves out: Lanczos shapes the plans reject (ol.lanczos_rows_defined), shapes
    with a border row or column whose valid taps sum to 0 (the `trap` shapes of tests/extreme_cases.py: the
    reference divides by zero there), and Linear upscales above 2x other than exact 3x (the reference reads
    row / column -1 there)."""
    if method == "linear":
        return (dw <= 2 * sw and dh <= 2 * sh) or (dw == 3 * sw and dh == 3 * sh)
    if method != "lanczos":
        return True
    if not ol.lanczos_rows_defined(d, sh, dh, px):
        return False
    ty = ol.oracle_tables("lanczos", d, sw, sh, dw, dh, px, 1)
    tx = ol.oracle_tables("lanczos", d, sw, sh, dw, dh, px, 0)
    return not (sh != dh and _zero_border(ty, sh, dh)) and not (sw != dw and _zero_border(tx, sw, dw))


SEARCHED = [
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 12, 'NP': 8, 'PD': 2, 'CPT': 2}, 'lanczos', 7, 18, 36, 16, 16, 2, ()),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 12, 'NP': 8, 'PD': 2, 'ADJ': 1, 'CPT': 2}, 'lanczos', 6, 17, 36, 16, 16, 2, ()),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 12, 'NP': 10, 'PD': 2, 'CPT': 2}, 'lanczos', 3, 41, 36, 16, 16, 1, (('ryx_split', 3), ('ryx_adj', 0))),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 12, 'NP': 10, 'PD': 2, 'ADJ': 1, 'CPT': 2}, 'lanczos', 7, 41, 36, 16, 16, 2, (('ryu', 0),)),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 8, 'NP': 6, 'PD': 2, 'CPT': 2}, 'lanczos', 2, 17, 36, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 8, 'NP': 6, 'PD': 2, 'ADJ': 1, 'CPT': 2}, 'lanczos', 2, 28, 36, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 8, 'NP': 7, 'PD': 2, 'CPT': 2}, 'lanczos', 4, 50, 36, 16, 16, 2, (('ryg_cpt', 4), ('ryx_adj', 0))),
    ('ryx', {'LZ': 1, 'P': 9, 'Q': 4, 'T': 8, 'NP': 7, 'PD': 2, 'ADJ': 1, 'CPT': 2}, 'lanczos', 4, 45, 36, 16, 16, 2, (('ryg_cpt', 3), ('ryu_run', 0))),
    ('ryx', {'P': 9, 'Q': 4, 'T': 4, 'NP': 3, 'PD': 2, 'CPT': 2}, 'area', 0, 17, 36, 16, 16, 1, ()),
    ('ryx', {'P': 9, 'Q': 4, 'T': 4, 'NP': 3, 'PD': 2, 'ADJ': 1, 'CPT': 2}, 'area', 0, 32, 36, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 1, 'T': 14, 'NP': 13, 'PD': 4, 'CPT': 2}, 'lanczos', 3, 52, 64, 16, 16, 1, (('ryg_cpt', 4), ('ryx_adj', 0))),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 1, 'T': 14, 'NP': 9, 'PD': 4, 'CPT': 2}, 'lanczos', 3, 17, 64, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 1, 'T': 22, 'NP': 17, 'PD': 3, 'CPT': 2}, 'lanczos', 4, 30, 64, 16, 16, 1, (('ryg_cpt', 2), ('ryu_run', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 4, 'NP': 3, 'PD': 2, 'CPT': 2}, 'lanczos', 1, 17, 32, 16, 16, 1, (('ryg_cpt', 3), ('ryx_adj', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 12, 'NP': 9, 'PD': 3, 'CPT': 2}, 'lanczos', 3, 17, 32, 16, 16, 1, (('ryx_split', 4),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 16, 'NP': 11, 'PD': 4, 'CPT': 2}, 'lanczos', 5, 17, 32, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 18, 'NP': 13, 'PD': 5, 'CPT': 2}, 'lanczos', 6, 17, 32, 16, 16, 1, (('ryg_cpt', 3), ('ryx_uc', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 20, 'NP': 15, 'PD': 5, 'CPT': 2}, 'lanczos', 7, 18, 32, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 22, 'NP': 17, 'PD': 2, 'CPT': 2}, 'lanczos', 8, 19, 34, 16, 17, 1, (('ryg_cpt', 4), ('ryu', 0), ('ryu_run', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 24, 'NP': 19, 'PD': 2, 'CPT': 2}, 'lanczos', 9, 20, 38, 16, 19, 1, (('ryu_run', 0),)),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 9, 'T': 6, 'NP': 4, 'PD': 2, 'CPT': 2}, 'lanczos', 3, 28, 8, 16, 18, 2, (('ryx_cpt', 0), ('ryu_run', 0))),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 9, 'T': 4, 'NP': 3, 'PD': 2, 'CPT': 2}, 'lanczos', 2, 17, 8, 16, 18, 1, (('ryg_cpt', 4),)),
    ('ryx', {'LZ': 1, 'P': 4, 'Q': 9, 'T': 6, 'NP': 4, 'PD': 2, 'CPT': 4}, 'lanczos', 3, 17, 8, 16, 18, 2, (('ryx_uc', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 4, 'NP': 3, 'PD': 2, 'CPT': 2, 'UC': 1}, 'lanczos', 1, 32, 36, 16, 18, 1, (('ryg_cpt', 4), ('ryx_adj', 0), ('ryu_run', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 4, 'NP': 3, 'PD': 2, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 1, 32, 32, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 12, 'NP': 9, 'PD': 3, 'CPT': 2, 'UC': 1}, 'lanczos', 3, 36, 32, 18, 16, 1, (('ryx_adj', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 12, 'NP': 9, 'PD': 3, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 4, 34, 32, 17, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 16, 'NP': 11, 'PD': 4, 'CPT': 2, 'UC': 1}, 'lanczos', 5, 36, 32, 18, 16, 1, (('ryg_cpt', 2), ('ryx_adj', 0), ('ryx_cpt', 0), ('ryu', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 16, 'NP': 11, 'PD': 4, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 5, 32, 32, 16, 16, 1, (('ryx_split', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 18, 'NP': 13, 'PD': 5, 'CPT': 2, 'UC': 1}, 'lanczos', 6, 34, 36, 17, 18, 1, (('ryx_adj', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 18, 'NP': 13, 'PD': 5, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 6, 32, 32, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 20, 'NP': 15, 'PD': 5, 'CPT': 2, 'UC': 1}, 'lanczos', 7, 34, 32, 17, 16, 1, (('ryx_adj', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 20, 'NP': 15, 'PD': 5, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 7, 32, 32, 16, 16, 1, ()),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 22, 'NP': 17, 'PD': 2, 'CPT': 2, 'UC': 1}, 'lanczos', 8, 32, 38, 16, 19, 1, (('ryx_adj', 0),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 22, 'NP': 17, 'PD': 2, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 8, 32, 36, 16, 18, 1, (('ryg_cpt', 4),)),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 24, 'NP': 19, 'PD': 2, 'CPT': 2, 'UC': 1}, 'lanczos', 9, 32, 40, 16, 20, 1, (('ryx_split', 0), ('ryx_adj', 0), ('ryu', 0))),
    ('ryx', {'LZ': 1, 'P': 2, 'Q': 1, 'T': 24, 'NP': 19, 'PD': 2, 'ADJ': 1, 'CPT': 2, 'UC': 1}, 'lanczos', 9, 32, 38, 16, 19, 1, (('ryu_run', 0),)),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 1, 17, 17, 16, 16, 2, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 2, 17, 17, 16, 16, 2, (('ryg_cpt', 3), ('ryx_uc', 0))),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 2, 17, 17, 16, 16, 2, ()),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 4, 17, 17, 16, 16, 2, (('ryg_cpt', 2), ('ryx_split', 0))),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 2, 17, 17, 16, 16, 1, (('ryg_cpt', 3), ('ryx_adj', 0))),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 4, 17, 17, 16, 16, 2, ()),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 3, 18, 17, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 6, 17, 17, 16, 16, 2, (('ryg_cpt', 3),)),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 6, 17, 17, 16, 16, 2, ()),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 5, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 4, 17, 18, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 5, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 4, 17, 19, 16, 16, 1, (('ryg_cpt', 3), ('ryx_uc', 0))),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 5, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 4, 17, 17, 16, 16, 1, (('ryx_uc', 0),)),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 6, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 9, 19, 17, 16, 16, 2, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 6, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 9, 17, 17, 16, 16, 2, (('ryx_cpt', 0), ('ryu_run', 0))),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 6, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 8, 19, 18, 16, 16, 2, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 7, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 5, 17, 17, 16, 16, 1, (('ryg_cpt', 2), ('ryx_cpt', 0))),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 7, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 5, 17, 17, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 7, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 6, 17, 17, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 8, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 6, 18, 17, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 8, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 6, 18, 17, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 8, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 6, 18, 17, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 10, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 7, 17, 17, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 10, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 7, 17, 19, 16, 16, 1, (('ryg_cpt', 3),)),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 10, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 7, 17, 19, 16, 16, 1, (('ryg_cpt', 4), ('ryx_adj', 0), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 12, 'PD': 4, 'CPT': 2, 'NL': 2}, 'lanczos', 7, 22, 17, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 12, 'PD': 4, 'CPT': 3, 'NL': 2}, 'lanczos', 7, 23, 17, 16, 16, 1, (('ryg_cpt', 3),)),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 12, 'PD': 4, 'CPT': 4, 'NL': 2}, 'lanczos', 7, 22, 20, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 2, 'NL': 1}, 'lanczos', 2, 20, 8, 16, 16, 1, (('ryg_cpt', 2), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 3, 'NL': 1}, 'lanczos', 2, 19, 8, 16, 16, 1, (('ryx_split', 0), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'NL': 1}, 'lanczos', 2, 18, 8, 16, 16, 1, (('ryg_cpt', 4), ('ryx_uc', 0), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 2, 'NL': 1}, 'lanczos', 3, 17, 9, 16, 16, 2, (('ryg_cpt', 2), ('ryx_split', 4), ('ryx_adj', 0), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 3, 'NL': 1}, 'lanczos', 3, 17, 8, 16, 16, 2, (('ryg_cpt', 3), ('ryu', 0))),
    ('ryg', {'LZ': 1, 'T': 6, 'NP': 4, 'PD': 4, 'CPT': 4, 'NL': 1}, 'lanczos', 3, 17, 8, 16, 16, 2, (('ryu', 0), ('ryu_run', 0))),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 2, 'NL': 1}, 'lanczos', 4, 17, 8, 16, 16, 1, (('ryg_cpt', 2), ('ryu', 0), ('ryu_run', 0))),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 3, 'NL': 1}, 'lanczos', 4, 19, 8, 16, 16, 2, (('ryu', 0),)),
    ('ryg', {'LZ': 1, 'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'NL': 1}, 'lanczos', 4, 17, 8, 16, 16, 1, (('ryg_cpt', 4), ('ryu', 0))),
    ('ryg', {'T': 3, 'NP': 2, 'PD': 4, 'CPT': 2, 'NL': 2}, 'linear', 0, 17, 17, 16, 16, 1, (('ryg_cpt', 2),)),
    ('ryg', {'T': 3, 'NP': 2, 'PD': 4, 'CPT': 3, 'NL': 2}, 'linear', 0, 17, 17, 16, 16, 1, (('ryg_cpt', 3),)),
    ('ryg', {'T': 3, 'NP': 2, 'PD': 4, 'CPT': 4, 'NL': 2}, 'linear', 0, 17, 17, 16, 16, 1, (('ryx_uc', 0),)),
    ('ryg', {'T': 3, 'NP': 3, 'PD': 4, 'CPT': 2, 'NL': 2}, 'area', 0, 35, 18, 16, 16, 1, ()),
    ('ryg', {'T': 3, 'NP': 3, 'PD': 4, 'CPT': 3, 'NL': 2}, 'area', 0, 35, 19, 16, 16, 1, (('ryg_cpt', 3),)),
    ('ryg', {'T': 3, 'NP': 3, 'PD': 4, 'CPT': 4, 'NL': 2}, 'area', 0, 35, 18, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 10, 'NP': 6, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 5, 17, 33, 16, 16, 2, ()),
    ('ryg', {'LZ': 1, 'T': 12, 'NP': 7, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 3, 17, 33, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 14, 'NP': 8, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 7, 17, 33, 16, 16, 2, (('ryg_cpt', 2),)),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 9, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 5, 17, 33, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 18, 'NP': 10, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 5, 17, 35, 16, 16, 1, ()),
    ('ryg', {'LZ': 1, 'T': 18, 'NP': 12, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 5, 32, 33, 16, 16, 1, (('ryx_split', 3), ('ryx_uc', 0))),
    ('ryg', {'LZ': 1, 'T': 22, 'NP': 16, 'PD': 4, 'CPT': 2, 'NL': 3}, 'lanczos', 7, 17, 33, 16, 16, 1, (('ryx_adj', 0),)),
    ('ryg', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 2, 'NL': 3}, 'area', 0, 17, 33, 16, 16, 1, ()),
    ('ryg', {'T': 4, 'NP': 4, 'PD': 4, 'CPT': 2, 'NL': 3}, 'area', 0, 67, 33, 16, 16, 1, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 14, 'NP': 8, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 4, 17, 49, 16, 16, 2, (('ryg_cpt', 4),)),
    ('ryg', {'LZ': 1, 'T': 16, 'NP': 9, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 6, 17, 51, 16, 16, 2, ()),
    ('ryg', {'LZ': 1, 'T': 18, 'NP': 10, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 7, 17, 49, 16, 16, 2, (('ryx_adj', 0),)),
    ('ryg', {'LZ': 1, 'T': 20, 'NP': 11, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 8, 17, 50, 16, 16, 2, (('ryg_cpt', 3),)),
    ('ryg', {'LZ': 1, 'T': 22, 'NP': 12, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 9, 17, 51, 16, 16, 2, (('ryx_cpt', 0),)),
    ('ryg', {'LZ': 1, 'T': 24, 'NP': 13, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 6, 17, 49, 16, 16, 1, (('ryg_cpt', 2), ('ryx_cpt', 0))),
    ('ryg', {'LZ': 1, 'T': 22, 'NP': 16, 'PD': 4, 'CPT': 2, 'NL': 4}, 'lanczos', 8, 50, 49, 16, 16, 2, (('ryx_cpt', 0), ('ryu', 0), ('ryu_run', 0))),
    ('ryg', {'T': 5, 'NP': 3, 'PD': 4, 'CPT': 2, 'NL': 4}, 'area', 0, 17, 49, 16, 16, 1, ()),
    ('ryg', {'T': 5, 'NP': 4, 'PD': 4, 'CPT': 2, 'NL': 4}, 'area', 0, 67, 50, 16, 16, 1, (('ryg_cpt', 4), ('ryx_split', 4))),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 2, 'KM': 2}, 'lanczos', 2, 17, 8, 16, 16, 2, (('ryg_cpt', 2), ('ryu_run', 0))),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 3, 'KM': 2}, 'lanczos', 2, 18, 8, 16, 16, 2, (('ryg_cpt', 3), ('ryx_cpt', 0))),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'KM': 2}, 'lanczos', 2, 18, 9, 16, 16, 1, (('ryu_run', 0),)),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'RUN': 4, 'KM': 2}, 'lanczos', 2, 17, 8, 16, 16, 1, ()),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'RUN': 5, 'KM': 2}, 'lanczos', 2, 18, 8, 16, 16, 1, ()),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 2, 'KM': 3}, 'lanczos', 2, 39, 12, 19, 25, 2, (('ryx_split', 0), ('ryx_cpt', 0))),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 3, 'KM': 3}, 'lanczos', 2, 22, 11, 17, 29, 2, (('ryg_cpt', 3), ('ryx_split', 3), ('ryu_run', 0))),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'KM': 3}, 'lanczos', 2, 18, 9, 23, 20, 1, (('ryu_run', 0),)),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'RUN': 4, 'KM': 3}, 'lanczos', 2, 16, 10, 23, 21, 1, (('ryx_cpt', 0),)),
    ('ryu', {'T': 4, 'NP': 3, 'PD': 4, 'CPT': 4, 'RUN': 5, 'KM': 3}, 'lanczos', 2, 35, 10, 32, 23, 1, (('ryx_adj', 0),)),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 2, 'KM': 2}, 'lanczos', 3, 17, 8, 16, 16, 2, (('ryg_cpt', 2),)),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 3, 'KM': 2}, 'lanczos', 3, 17, 8, 16, 16, 1, (('ryg_cpt', 3), ('ryx_uc', 0))),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'KM': 2}, 'lanczos', 3, 17, 10, 16, 16, 1, (('ryu_run', 0),)),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'RUN': 5, 'KM': 2}, 'lanczos', 3, 18, 8, 16, 16, 2, ()),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'RUN': 6, 'KM': 2}, 'lanczos', 3, 17, 8, 16, 16, 1, ()),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 2, 'KM': 3}, 'lanczos', 3, 16, 9, 17, 24, 1, (('ryg_cpt', 2),)),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 3, 'KM': 3}, 'lanczos', 3, 20, 8, 25, 22, 2, (('ryg_cpt', 3),)),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'KM': 3}, 'lanczos', 3, 20, 9, 18, 20, 2, (('ryx_split', 0), ('ryx_cpt', 0), ('ryu_run', 0))),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'RUN': 5, 'KM': 3}, 'lanczos', 3, 21, 8, 28, 20, 1, (('ryx_split', 3), ('ryx_adj', 0), ('ryx_uc', 0))),
    ('ryu', {'T': 6, 'NP': 4, 'PD': 3, 'CPT': 4, 'RUN': 6, 'KM': 3}, 'lanczos', 3, 20, 9, 19, 26, 1, (('ryx_split', 2),)),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 2, 'KM': 2}, 'lanczos', 4, 19, 8, 16, 16, 2, (('ryg_cpt', 2),)),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 3, 'KM': 2}, 'lanczos', 4, 17, 8, 16, 16, 1, (('ryg_cpt', 3), ('ryu_run', 0))),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'KM': 2}, 'lanczos', 4, 17, 8, 16, 16, 1, (('ryg_cpt', 4), ('ryu_run', 0))),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'RUN': 6, 'KM': 2}, 'lanczos', 4, 17, 8, 16, 16, 2, ()),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'RUN': 7, 'KM': 2}, 'lanczos', 4, 18, 8, 16, 16, 1, ()),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 2, 'KM': 3}, 'lanczos', 4, 17, 8, 16, 18, 2, (('ryg_cpt', 2), ('ryx_split', 2))),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 3, 'KM': 3}, 'lanczos', 4, 22, 8, 16, 18, 2, (('ryg_cpt', 3),)),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'KM': 3}, 'lanczos', 4, 20, 8, 16, 18, 2, (('ryg_cpt', 4), ('ryx_split', 4), ('ryu_run', 0))),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'RUN': 6, 'KM': 3}, 'lanczos', 4, 18, 8, 16, 18, 2, (('ryx_split', 0),)),
    ('ryu', {'T': 8, 'NP': 5, 'PD': 4, 'CPT': 4, 'RUN': 7, 'KM': 3}, 'lanczos', 4, 18, 8, 16, 18, 1, (('ryx_cpt', 0),)),
    ('tile', {'LZ': 1, 'NP': 1}, 'lanczos', 4, 16, 8, 16, 16, 1, ()),
    ('tile', {'NP': 1}, 'linear', 0, 16, 8, 16, 16, 1, TILE_ONLY),
    ('tile', {'LZ': 1, 'NP': 2}, 'lanczos', 1, 18, 9, 19, 16, 1, TILE_ONLY),
    ('tile', {'NP': 2}, 'area', 0, 17, 8, 16, 16, 1, TILE_ONLY),
    ('tile', {'LZ': 1, 'NP': 3}, 'lanczos', 1, 17, 8, 16, 16, 2, (('ryg_cpt', 4),)),
    ('tile', {'NP': 3}, 'area', 0, 34, 8, 16, 16, 1, ()),
    ('tile', {'LZ': 1, 'NP': 4}, 'lanczos', 5, 17, 8, 16, 16, 2, ()),
    ('tile', {'NP': 4}, 'area', 0, 66, 8, 16, 16, 1, ()),
    ('tile', {'LZ': 1, 'NP': 5}, 'lanczos', 6, 17, 8, 16, 16, 2, ()),
    ('tile', {'NP': 5}, 'area', 0, 98, 8, 16, 16, 1, (('ryg_cpt', 3), ('ryx_split', 3), ('ryu', 0))),
    ('tile', {'LZ': 1, 'NP': 6}, 'lanczos', 8, 17, 8, 16, 16, 2, (('ryg_cpt', 4), ('ryx_cpt', 0))),
    ('tile', {'NP': 6}, 'area', 0, 130, 8, 16, 16, 1, (('ryg_cpt', 4),)),
    ('tile', {'LZ': 1, 'NP': 7}, 'lanczos', 5, 17, 8, 16, 16, 1, ()),
    ('tile', {'NP': 7}, 'area', 0, 162, 8, 16, 16, 1, ()),
    ('tile', {'LZ': 1, 'NP': 8}, 'lanczos', 6, 17, 8, 16, 16, 1, ()),
    ('tile', {'NP': 8}, 'area', 0, 194, 8, 16, 16, 1, RATIO_OFF),
    ('tile', {'LZ': 1, 'NP': 10}, 'lanczos', 8, 17, 8, 16, 16, 1, ()),
    ('tile', {'NP': 10}, 'area', 0, 226, 8, 16, 16, 1, RATIO_OFF),
    ('tile', {'LZ': 1, 'NP': 12}, 'lanczos', 9, 17, 8, 16, 16, 1, ()),
    ('tile', {'NP': 12}, 'area', 0, 324, 8, 17, 16, 1, ()),
    ('tile', {'LZ': 1, 'NP': 16}, 'lanczos', 9, 20, 8, 16, 16, 1, ()),
    ('tile', {'NP': 16}, 'area', 0, 378, 9, 16, 21, 1, TILE_ONLY),
    ('walk', {'LZ': 1, 'NP': 1, 'VY': 2, 'NV': 1}, 'lanczos', 1, 16, 8, 16, 16, 1, ()),
    ('walk', {'NP': 1, 'VY': 2, 'NV': 1}, 'linear', 0, 16, 8, 16, 16, 1, ()),
    ('walk', {'NP': 1, 'VY': 2, 'NV': 2}, 'linear', 0, 252, 9, 21, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 2, 'VY': 4, 'NV': 1}, 'lanczos', 1, 16, 17, 17, 16, 1, RATIO_OFF),
    ('walk', {'NP': 2, 'VY': 4, 'NV': 1}, 'area', 0, 17, 17, 16, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 2, 'VY': 4, 'NV': 2}, 'lanczos', 1, 507, 24, 512, 21, 1, RATIO_OFF),
    ('walk', {'NP': 2, 'VY': 4, 'NV': 2}, 'area', 0, 267, 18, 89, 16, 1, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 2, 'VY': 2, 'NV': 1}, 'lanczos', 1, 16, 8, 19, 16, 1, RATIO_OFF),
    ('walk', {'NP': 2, 'VY': 2, 'NV': 1}, 'area', 0, 17, 8, 16, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 2, 'VY': 2, 'NV': 2}, 'lanczos', 1, 345, 9, 346, 16, 1, RATIO_OFF),
    ('walk', {'NP': 2, 'VY': 2, 'NV': 2}, 'linear', 0, 211, 8, 16, 16, 1, (('ryg_cpt', 2), ('ryx_split', 0))),
    ('walk', {'LZ': 1, 'NP': 3, 'VY': 6, 'NV': 1}, 'lanczos', 3, 17, 8, 16, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 3, 'VY': 6, 'NV': 2}, 'lanczos', 3, 253, 8, 151, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 3, 'VY': 4, 'NV': 1}, 'lanczos', 2, 17, 8, 16, 16, 2, RATIO_OFF),
    ('walk', {'NP': 3, 'VY': 4, 'NV': 1}, 'area', 0, 34, 17, 16, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 3, 'VY': 4, 'NV': 2}, 'lanczos', 2, 272, 9, 141, 16, 2, RATIO_OFF),
    ('walk', {'NP': 3, 'VY': 4, 'NV': 2}, 'area', 0, 258, 17, 67, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 4, 'VY': 8, 'NV': 1}, 'lanczos', 4, 19, 8, 16, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 4, 'VY': 8, 'NV': 2}, 'lanczos', 4, 252, 9, 204, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 4, 'VY': 6, 'NV': 1}, 'lanczos', 3, 17, 9, 20, 16, 1, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 4, 'VY': 6, 'NV': 2}, 'lanczos', 3, 286, 8, 109, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 5, 'VY': 10, 'NV': 1}, 'lanczos', 5, 25, 8, 16, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 5, 'VY': 10, 'NV': 2}, 'lanczos', 5, 247, 9, 126, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 5, 'VY': 8, 'NV': 1}, 'lanczos', 4, 16, 9, 19, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 5, 'VY': 8, 'NV': 2}, 'lanczos', 4, 279, 8, 139, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 6, 'VY': 12, 'NV': 1}, 'lanczos', 6, 22, 8, 16, 16, 2, (('ryg_cpt', 4), ('ryx_uc', 0))),
    ('walk', {'LZ': 1, 'NP': 6, 'VY': 12, 'NV': 2}, 'lanczos', 6, 247, 11, 149, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 6, 'VY': 10, 'NV': 1}, 'lanczos', 5, 16, 8, 18, 16, 2, (('ryg_cpt', 3),)),
    ('walk', {'LZ': 1, 'NP': 6, 'VY': 10, 'NV': 2}, 'lanczos', 5, 249, 9, 101, 16, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 7, 'VY': 14, 'NV': 1}, 'lanczos', 7, 27, 8, 16, 16, 2, (('ryx_adj', 0),)),
    ('walk', {'LZ': 1, 'NP': 7, 'VY': 14, 'NV': 2}, 'lanczos', 7, 250, 8, 125, 18, 2, (('ryg_cpt', 4), ('ryu', 0))),
    ('walk', {'LZ': 1, 'NP': 7, 'VY': 12, 'NV': 1}, 'lanczos', 6, 16, 8, 17, 16, 1, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 7, 'VY': 12, 'NV': 2}, 'lanczos', 6, 248, 9, 132, 16, 2, (('ryg_cpt', 2),)),
    ('walk', {'LZ': 1, 'NP': 8, 'VY': 16, 'NV': 1}, 'lanczos', 8, 25, 8, 16, 16, 2, ()),
    ('walk', {'LZ': 1, 'NP': 8, 'VY': 16, 'NV': 2}, 'lanczos', 8, 252, 9, 158, 17, 2, RATIO_OFF),
    ('walk', {'LZ': 1, 'NP': 8, 'VY': 14, 'NV': 1}, 'lanczos', 7, 16, 8, 17, 16, 1, ()),
    ('walk', {'LZ': 1, 'NP': 8, 'VY': 14, 'NV': 2}, 'lanczos', 7, 245, 9, 108, 16, 2, RATIO_OFF),
]


def _pd(kernel, params, method, degree, sw, sh, dw, dh, pd=None):
    return (kernel, params, method, degree, sw, sh, dw, dh, 1, (("ratio_prefetch", pd),) if pd else ())


# up2: 2x and 3x at degrees 2 and 3.  d32 / d31: the Lanczos-3 tap structure (VARIANT 0) and the Lanczos-2 one, each
# at its default depth (no option) and at every other depth.  u23 / l23: dstW 24, one lane per row.  a32: one
# lane per row.
EXACT = [
    _pd("lanczos_up2", {"NT": 4, "F": 2}, "lanczos", 2, 200, 60, 400, 120),
    _pd("lanczos_up2", {"NT": 6, "F": 2}, "lanczos", 3, 192, 108, 384, 216),
    _pd("lanczos_up2", {"NT": 4, "F": 3}, "lanczos", 2, 16, 5, 48, 15),
    _pd("lanczos_up2", {"NT": 6, "F": 3}, "lanczos", 3, 136, 40, 408, 120),
    _pd("lanczos_d32", {"PD": 1}, "lanczos", 3, 504, 300, 336, 200),
    _pd("lanczos_d32", {"PD": 2}, "lanczos", 3, 504, 300, 336, 200, 2),
    _pd("lanczos_d32", {"PD": 4}, "lanczos", 3, 504, 300, 336, 200, 4),
    _pd("lanczos_d32", {"PD": 1, "VARIANT": 1}, "lanczos", 2, 240, 150, 160, 100),
    _pd("lanczos_d32", {"PD": 3, "VARIANT": 1}, "lanczos", 2, 240, 150, 160, 100, 3),
    _pd("lanczos_d31", {"PD": 1}, "lanczos", 3, 336, 204, 112, 68),
    _pd("lanczos_d31", {"PD": 5}, "lanczos", 3, 336, 204, 112, 68, 5),
    _pd("lanczos_d31", {"PD": 1, "VARIANT": 1}, "lanczos", 2, 192, 96, 64, 32),
    _pd("lanczos_d31", {"PD": 2, "VARIANT": 1}, "lanczos", 2, 192, 96, 64, 32, 2),
    _pd("lanczos_d31", {"PD": 4, "VARIANT": 1}, "lanczos", 2, 192, 96, 64, 32, 4),
    _pd("lanczos_u23", {"PD": 1}, "lanczos", 3, 16, 16, 24, 24),
    _pd("lanczos_u23", {"PD": 2}, "lanczos", 3, 16, 16, 24, 24, 2),
    _pd("linear_u23", {"PD": 2}, "linear", 0, 16, 16, 24, 24),
    _pd("linear_u23", {"PD": 1}, "linear", 0, 16, 16, 24, 24, 1),
    _pd("area_d32", {"PD": 4}, "area", 0, 12, 6, 8, 4),
    _pd("area_d32", {"PD": 2}, "area", 0, 12, 6, 8, 4, 2),
    _pd("area_d32", {"PD": 8}, "area", 0, 12, 6, 8, 4, 8),
]

# the second shapes: u23 / l23 at a two-wave width (64 lanes of 12 columns), a32 at four lanes per row
EXTRA = [
    _pd("lanczos_u23", {"PD": 1}, "lanczos", 3, 512, 16, 768, 24),
    _pd("lanczos_u23", {"PD": 2}, "lanczos", 3, 512, 16, 768, 24, 2),
    _pd("linear_u23", {"PD": 2}, "linear", 0, 512, 16, 768, 24),
    _pd("linear_u23", {"PD": 1}, "linear", 0, 512, 16, 768, 24, 1),
    _pd("area_d32", {"PD": 4}, "area", 0, 48, 30, 32, 20),
    _pd("area_d32", {"PD": 2}, "area", 0, 48, 30, 32, 20, 2),
    _pd("area_d32", {"PD": 8}, "area", 0, 48, 30, 32, 20, 8),
]

INSTANTIATIONS = SEARCHED + EXACT   # one row per instantiation
ALL_ROWS = INSTANTIATIONS + EXTRA

# One forced depth per exact-ratio family that its kernel does not instantiate: the resize call must fail
# (abi.hip run_band), not fall back to the default depth.  (kernel, method, degree, sw, sh, dw, dh, depth)
BAD_PREFETCH = [
    ("lanczos_d32", "lanczos", 3, 504, 300, 336, 200, 3),
    ("lanczos_d31", "lanczos", 3, 336, 204, 112, 68, 2),
    ("lanczos_u23", "lanczos", 3, 16, 16, 24, 24, 4),
    ("linear_u23", "linear", 0, 16, 16, 24, 24, 4),
    ("area_d32", "area", 0, 12, 6, 8, 4, 3),
]

# walk_kernel instantiations no shape runs.  The walker takes a plan only when (plan.cpp build_walk_tables)
#   :997   the row taps unroll as VY = 2 NP or 2 NP - 2 of the column pairs NP, i.e. rows and columns have about
#          the same number of taps;
#   :1017  a 256-output strip reads at most 512 source columns: NV = 1 up to 256 of them, NV = 2 above;
#   :1027  consecutive output rows bring in at most NV (<= 2) new source rows.
_AL_DEEP = ("plan.cpp:997 with plan.cpp:1027: VY >= 6 needs Area / Linear row windows of 5 or more source rows, which only "
            "rows shrinking by more than 3:1 have; their windows advance by 3 or more rows per output row, above "
            "NV <= 2.  Also not found within the bounds")
UNREACHABLE = [
    ("walk", {"LZ": 1, "NP": 1, "VY": 2, "NV": 2},
     "plan.cpp:1017: NP 1 holds two column taps at an even window start, which Lanczos columns have only where "
     "dstW == srcW (one tap each; every Lanczos-1 upscale has odd window starts and takes NP 2); a 256-output strip "
     "of such an axis reads exactly 256 source columns, 64 units, so NV is 1.  Also not found within the bounds"),
] + [("walk", {"NP": 3, "VY": 6, "NV": nv}, _AL_DEEP) for nv in (1, 2)] + [
    ("walk", {"NP": np_, "VY": vy, "NV": nv}, _AL_DEEP)
    for np_ in (4, 5, 6, 7, 8) for vy in (2 * np_, 2 * np_ - 2) for nv in (1, 2)]


def key_of(kernel, params):
    return (kernel,) + tuple(sorted(params.items()))


def instance_of(row):
    """The row's instantiation in the form of libiqo_amd.host_instance_for."""
    return dict(row[1], kernel=row[0])


def rid(row):
    kernel, params, method, degree, sw, sh, dw, dh, px, options = row
    return "%s-%s-%s%d-%dx%d-%dx%d-px%d" % (kernel, "".join("%s%d" % kv for kv in params.items()), method, degree, sw, sh,
                                          dw, dh, px)


@functools.lru_cache(maxsize=None)
def _al_frames(sw, sh):
    half = ol.gen("flat255", sw, sh)
    half[:, : max(1, sw // 2)] = 0
    out = np.stack([ol.gen("noise", sw, sh, 77), ol.gen("flat255", sw, sh), ol.gen("checker", sw, sh), half])
    out.setflags(write=False)
    return ("noise", "flat255", "checker", "halfflat"), out


@functools.lru_cache(maxsize=None)
def _al_expected(method, sw, sh, dw, dh):
    out = np.stack([ol.run_oracle(method, 0, sw, sh, dw, dh, 1, f) for f in _al_frames(sw, sh)[1]])
    out.setflags(write=False)
    return out


def frames_of(row):
    """(names, frames [n, sh, sw]), read-only and shared: Lanczos rows take the tap-sign and border-stress set of
    tests/extreme_cases.py; Area and Linear rows noise, all-255, a checkerboard and a half-flat frame."""
    _, _, method, degree, sw, sh, dw, dh, px, _ = row
    if method == "lanczos":
        return ec.plane_frames(degree, sw, sh, dw, dh, px, True)
    return _al_frames(sw, sh)


def expected_of(row):
    """ol.run_oracle of every frame of frames_of(row), computed once per shape and read-only."""
    _, _, method, degree, sw, sh, dw, dh, px, _ = row
    if method == "lanczos":
        return ec.plane_expected(degree, sw, sh, dw, dh, px, True)
    return _al_expected(method, sw, sh, dw, dh)
