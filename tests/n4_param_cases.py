"""The N4 parameter cases off the defaults, their volumes and the C oracle's results for them
(test_n4_oracle_params.py on the host, test_gpu_n4_params.py on the device).  Not a test module.

Every case is a keyword set of oracle.native.n4 / _lib.n4_params.  The oracle's result of a
(shape, case, conv_mode) is computed once and returned read-only."""
import functools

import numpy as np

from oracle import native
from vent_analysis_amd.synth import synth_volume

# (R, C, Z, seed).  12x70x9: a column range (C * Z = 630) over one 64-column tile and one row slot.
SHAPES = {"37x45x7": (37, 45, 7, 11), "24x20x6": (24, 20, 6, 31), "12x70x9": (12, 70, 9, 12)}
MAIN_SHAPES = ("37x45x7", "24x20x6")

FOUR = (50, 50, 50, 50)
CASES = {
    "ncp-x": dict(ncp=(5, 4, 4)),
    "ncp-y": dict(ncp=(4, 6, 4)),   # ncy alone the largest
    "ncp-z": dict(ncp=(4, 4, 5)),
    "ncp-564": dict(ncp=(5, 6, 4), max_iters=(50, 50, 50)),
    "ncp-456": dict(ncp=(4, 5, 6), max_iters=(50, 50, 50)),
    "ncp-645": dict(ncp=(6, 4, 5), max_iters=(50, 50, 50)),
    "levels-1": dict(max_iters=(50,)),
    "levels-2": dict(max_iters=(50, 50)),
    "levels-3": dict(max_iters=(20, 10, 5)),
    "cap": dict(max_iters=(7, 1, 3, 2)),
    "thr-hi": dict(conv_threshold=0.003),
    "thr-lo": dict(conv_threshold=3e-4),
    "fwhm-hi": dict(fwhm=0.3),
    "fwhm-lo": dict(fwhm=0.05),
    "wiener-hi": dict(wiener_noise=0.1),
    "wiener-lo": dict(wiener_noise=0.001),
    "bins-37": dict(n_bins=37),
    "bins-256": dict(n_bins=256),
    "combo": dict(ncp=(5, 6, 4), n_bins=128, fwhm=0.2, wiener_noise=0.02, conv_threshold=0.003,
                  max_iters=(12, 9, 6)),
}
# not in the table: the defaults (what a case must differ from; the middle of the threshold chain)
# and the three-level prefix of the default schedule
EXTRA = {"default": {}, "prefix-3": dict(max_iters=FOUR[:3])}
ALL = {**CASES, **EXTRA}
PREFIX = {1: "levels-1", 2: "levels-2", 3: "prefix-3", 4: "default"}   # max_iters = FOUR[:k]
THRESHOLDS = ("thr-hi", "default", "thr-lo")                           # 0.003, 0.001, 3e-4

# the cases the volume-resident kernels may refuse (their state has to fit in LDS)
LARGE = {
    "ncp-777": dict(ncp=(7, 7, 7)),                         # final lattice 35^3
    "levels-5": dict(max_iters=(8, 8, 8, 8, 8)),            # final lattice 19^3
    "levels-8": dict(max_iters=(3, 3, 3, 3, 2, 2, 2, 2)),   # VH_MAX_LEVELS; final lattice 131^3
}


def shapes_of(case):
    return tuple(SHAPES) if case.startswith("ncp-") else MAIN_SHAPES


def table():
    """[(case, shape)] of the case table."""
    return [(c, s) for c in CASES for s in shapes_of(c)]


def n_levels(kw):
    return len(kw.get("max_iters", FOUR))


@functools.lru_cache(maxsize=None)
def volume(shape):
    X, M = synth_volume(*SHAPES[shape])
    M = M.astype(np.uint8)
    X.setflags(write=False)
    M.setflags(write=False)
    return X, M


def params(case):
    return {**ALL, **LARGE}[case]


@functools.lru_cache(maxsize=None)
def oracle(shape, case, conv_mode=0):
    """(field float32, iterations int32 [levels], convergence float32 [levels]), read-only."""
    X, M = volume(shape)
    out = native.n4(X, M, conv_mode=conv_mode, **params(case))
    for a in out:
        a.setflags(write=False)
    return out
