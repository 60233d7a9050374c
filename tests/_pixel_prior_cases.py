"""The cases of the pixel-space priors that tests/test_pixel_prior_cpu.py holds the float64 restatement
to (against torch.autograd) and tests/test_hip_pixel_prior.py the library (against the restatement).

Detail term: (h, w, pools, cell weights).  x and c are drawn independently in [0, 1], so D_p does not rest on cancellation.
    degenerate      1 x 1 (L = 0), one row, one partial cell (3 x 3 at p = 4), two pool sizes on 2 x 3
    ragged cells    partial cells on the last row, the last column or both; 17 x 16 at p = 16: a full and a 1-row cell
    workgroups      257 x 300 at p = 1, 2, 8: 9 x 10, 5 x 5 and 2 x 2 tiles; 33 x 33 at p = 1, 2, 4 and 65 x 65 at p = 8, 16:
                    one pixel more than a tile (32 pixels up to p = 8, 64 at p = 16) in both axes
    ticket wrap     3 x 8193 at p = 1, 4 (and for TV): 257 tiles in one row, so the block that takes the last ticket makes a
                    second trip over the 256-strided partials; three rows keep the vertical neighbours
    cell weights    absent | random | random with a block of zeros (so that some cell and its neighbours weigh 0) | all zero
TV: (h, w); 42 x 63 and 257 x 300 span several 32 x 32 tiles both ways, 3 x 8193 is the ticket wrap."""
import functools

import numpy as np

import _pixel_prior_ref as PR

WEIGHTS = ("absent", "random", "zeros_block", "all_zero")

# (h, w, pools, weights)
DETAIL = [
    (1, 1, (1,), "absent"),
    (1, 5, (1,), "absent"),
    (3, 3, (4,), "absent"),
    (2, 3, (1, 2), "random"),
    (5, 7, (2,), "absent"),
    (5, 7, (2,), "random"),
    (42, 63, (1, 4), "absent"),
    (42, 63, (1, 4), "random"),
    (42, 63, (1, 4), "zeros_block"),
    (42, 63, (1, 4), "all_zero"),
    (33, 65, (2, 16), "absent"),
    (33, 65, (2, 16), "zeros_block"),
    (17, 16, (16,), "random"),
    (257, 300, (1, 2, 8), "absent"),
    (257, 300, (1, 2, 8), "random"),
    (33, 33, (1, 2, 4), "random"),
    (65, 65, (8, 16), "zeros_block"),
    (3, 8193, (1, 4), "random"),
]
TV = [(1, 1), (1, 5), (5, 1), (2, 2), (42, 63), (257, 300), (3, 8193)]


def detail_label(case):
    h, w, pools, wk = case
    return f"{h}x{w}-p{'_'.join(str(p) for p in pools)}-{wk}"


def tv_label(case):
    return f"{case[0]}x{case[1]}"


DETAIL_LABELS = [detail_label(c) for c in DETAIL]
TV_LABELS = [tv_label(c) for c in TV]
assert len(set(DETAIL_LABELS)) == len(DETAIL)


def cell_weights(h, w, p, kind, rng):
    """the (hp, wp) float32 cell weights of one pool size, or None"""
    hp, wp = PR.grid(h, w, p)
    if kind == "absent":
        return None
    if kind == "all_zero":
        return np.zeros((hp, wp), dtype=np.float32)
    m = (0.25 + 1.25 * rng.random((hp, wp))).astype(np.float32)
    if kind == "zeros_block":           # the upper left 60 % of the grid (at least 3 x 3 cells where the grid has them)
        m[: max(3, (3 * hp) // 5), : max(3, (3 * wp) // 5)] = 0.0
    return m


@functools.lru_cache(maxsize=None)
def detail_inputs(label):
    """{x, c (h, w, 3) float32, weights [per pool size], g0 (h, w, 3) float32: a pre-filled gradient}; cached, read-only"""
    h, w, pools, wk = DETAIL[DETAIL_LABELS.index(label)]
    rng = np.random.default_rng(1000 * h + w + sum(pools))
    x = rng.random((h, w, 3)).astype(np.float32)
    c = rng.random((h, w, 3)).astype(np.float32)
    weights = [cell_weights(h, w, p, wk, rng) for p in pools]
    g0 = (rng.standard_normal((h, w, 3)) * 1e-3).astype(np.float32)
    return dict(h=h, w=w, pools=list(pools), kind=wk, x=x, c=c, weights=weights, g0=g0)


@functools.lru_cache(maxsize=None)
def tv_inputs(label):
    h, w = TV[TV_LABELS.index(label)]
    rng = np.random.default_rng(77 * h + w)
    return dict(h=h, w=w, x=rng.random((h, w, 3)).astype(np.float32),
                g0=(rng.standard_normal((h, w, 3)) * 1e-3).astype(np.float32))


def dead_pixels(h, w, p, m):
    """(h, w) bool: the pixels of cells whose own weight and whose in-grid neighbours' weights are all 0"""
    z = np.pad(m == 0, 1, constant_values=True)
    dead = z[1:-1, 1:-1] & z[:-2, 1:-1] & z[2:, 1:-1] & z[1:-1, :-2] & z[1:-1, 2:]
    return np.repeat(np.repeat(dead, p, axis=0), p, axis=1)[:h, :w]


# ------------------------------------------------------------------ steps with the two terms (the engine's tests)
# rows in the format of tests/_step_cases.py: (transport, side, map, targets, (h, w), seed), seeds those of _transport_cases
STEP_TABLE = [
    ("remd", "one", False, 0, (64, 64), 0),
    ("remd", "one", False, 1, (42, 64), 4),
    ("remd", "regions", False, 0, (64, 64), 5),
    ("remd", "blend", True, 1, (64, 64), 8),
]
STEP_POOLS = (1, 4)                 # the command line's default
