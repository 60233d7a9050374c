"""The seeded cases of the scribble tests: image, stroke labels and score grid per (h, w, k), and the
float64 / float32 restatement of each (tests/_scribble_ref.py), computed once and shared.  The shapes are the smallest at
which the kernels can go wrong: the smallest images, one row or column below / on / above the blocked form's 64 x 32 tile,
two sizes with several tiles.  test_scribble_cpu.py asserts the conditions on the cases (the float32 yardstick Y and the label
margins); test_hip_scribble.py holds the kernels against them."""
import numpy as np

import _scribble_ref as R

SMALL = [(1, 2), (2, 2), (2, 300), (300, 2), (3, 5)]
TILE_ROWS = [(31, 67), (32, 67), (33, 67)]                  # one below / on / above the tile's 32 rows
TILE_COLS = [(45, 63), (45, 64), (45, 65)]                  # one below / on / above the tile's 64 columns
GENERAL = [(42, 63), (97, 130)]
SHAPES = SMALL + TILE_ROWS + TILE_COLS + GENERAL
KS = (2, 3, 7)
SWEEPS = (1, 3, 8, 24)                                      # one; an odd number of swaps; one blocked launch at T = 8; several
DEFAULT_AT = (42, 63)                                       # the default 128 sweeps, at this shape only
Y_CAP = 5e-6                                                # the yardstick of a case must lie in (0, Y_CAP)
MARGIN_FACTOR, MARGIN_SHARE = 8.0, 0.01                     # at most 1 % of a case's pixels with a margin below 8 Y

_made, _run = {}, {}


def sweeps_of(shape):
    return SWEEPS + ((R.ITERS,) if tuple(shape) == DEFAULT_AT else ())


def region_map(h, w, k):
    """k slanted bands"""
    ys, xs = np.mgrid[0:h, 0:w]
    t = (xs + 0.5) / w + 0.3 * (ys + 0.5) / h
    return np.minimum((t * k / 1.3).astype(np.int64), k - 1)


def make(h, w, k):
    """(img (h, w, 3) float32 in [0, 1]: k slanted bands of one colour each plus noise; stroke (h, w) int32: about one pixel
    in 16 carries the label of its band, pixel 0 always, the others -1; scores (gh, gw, k) float32: 0.3, + 0.4 for the band
    of the cell's centre, + noise)"""
    if (h, w, k) not in _made:
        rng = np.random.default_rng(7000 + 131 * h + 17 * w + k)
        region = region_map(h, w, k)
        colours = rng.uniform(0.1, 0.9, size=(k, 3))
        img = np.clip(colours[region] + 0.02 * rng.standard_normal((h, w, 3)), 0.0, 1.0).astype(np.float32)
        drawn = rng.random((h, w)) < 1.0 / 16.0
        drawn[0, 0] = True
        drawn[-1, -1] = False                                # at least one free pixel
        stroke = np.where(drawn, region, -1).astype(np.int32)
        gh, gw = max(1, -(-h // 4)), max(1, -(-w // 4))
        cell = region_map(gh, gw, k)
        scores = (0.3 + 0.4 * (cell[..., None] == np.arange(k)) + 0.05 * rng.standard_normal((gh, gw, k))).astype(np.float32)
        _made[(h, w, k)] = (img, stroke, scores)
    return _made[(h, w, k)]


def run(h, w, k, dtype=np.float64):
    """the restatement of case (h, w, k) at the defaults, with a snapshot after each of sweeps_of((h, w)); computed once"""
    key = (h, w, k, np.dtype(dtype).name)
    if key not in _run:
        img, stroke, scores = make(h, w, k)
        _run[key] = R.diffuse(img, stroke, scores, iters=sweeps_of((h, w)), dtype=dtype)
    return _run[key]


def yardstick(h, w, k, n):
    """Y = max |x_f32ref - x_f64ref| after n sweeps"""
    return float(np.abs(run(h, w, k, np.float32)[n]["x"].astype(np.float64) - run(h, w, k)[n]["x"]).max())
