"""Float64 / integer NumPy restatement of region tracking: strotss_label_warp (the prior label of a grid
cell along the backward flow) and strotss_kmeans_assign_prior (the assignment biased toward that prior), with the cases the
CPU and GPU tests share.  The scores, the error bound and the planted rows are those of tests/_cluster_ref.py.  Pure host
code: the CPU tests check it against itself, the GPU tests check the kernels against it."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as R  # noqa: E402


# ------------------------------------------------------------------ A. the prior along the flow
def cell_starts(g: int, n: int) -> np.ndarray:
    """(g + 1,): the first pixel row (column) of cells 0..g of g cells over n pixels -- the smallest y with y g // n >= i"""
    return (np.arange(g + 1, dtype=np.int64) * n + g - 1) // g


def probes(g: int, n: int) -> np.ndarray:
    """(g,): the probe row (column) of every cell, the integer mean of its first and last owned row (column)"""
    s = cell_starts(g, n)
    return (s[:-1] + s[1:] - 1) // 2


def label_warp(prev_grid, k, flow, certainty, dtype=np.float32):
    """(gh, gw) int32 priors.  dtype: the arithmetic of the source pixel, sy = floor((y_c + dy) + 0.5): float32 is what the
    kernel does, float64 the exact statement (they agree wherever no sum lands within a float32 rounding of k + 0.5)"""
    prev_grid = np.asarray(prev_grid)
    gh, gw = prev_grid.shape
    h, w = flow.shape[:2]
    yc, xc = probes(gh, h), probes(gw, w)
    out = np.full((gh, gw), -1, dtype=np.int32)
    half = dtype(0.5)
    for i in range(gh):
        for j in range(gw):
            dx, dy = flow[yc[i], xc[j]]
            if not (np.isfinite(dx) and np.isfinite(dy)):
                continue
            if certainty is not None and certainty[yc[i], xc[j]] < 0.5:
                continue
            sy = np.floor((dtype(yc[i]) + dtype(dy)) + half)
            sx = np.floor((dtype(xc[j]) + dtype(dx)) + half)
            if not (0 <= sy < h and 0 <= sx < w):
                continue
            lab = int(prev_grid[int(sy) * gh // h, int(sx) * gw // w])
            if 0 <= lab < k:
                out[i, j] = lab
    return out


WARP_SHAPES = [(21, 32, 5, 7), (64, 48, 64, 48), (7, 5, 1, 1)]        # (h, w, gh, gw); gh == h in the second
WARP_K = 3


def _push_flows(h, w, gh, gw, rng):
    """flows whose border cells' probes leave the image through every edge; every component a multiple of 1/4"""
    yc, xc = probes(gh, h), probes(gw, w)
    base = (rng.integers(-12, 13, size=(h, w, 2)) / 4.0).astype(np.float32)
    ups = {"up": (0.0, -(float(yc[0]) + 1.25)), "down": (0.0, float(h - yc[-1]) + 0.25),
           "left": (-(float(xc[0]) + 1.25), 0.0), "right": (float(w - xc[-1]) + 0.25, 0.0)}
    if gh * gw == 1:                                                 # one cell: one flow per edge
        flows = []
        for v in ups.values():
            f = base.copy()
            f[yc[0], xc[0]] = v
            flows.append(f)
        return flows
    f = base.copy()
    f[yc[0], xc] = ups["up"]
    f[yc[-1], xc] = ups["down"]
    f[yc[1:-1], xc[0]] = ups["left"]
    f[yc[1:-1], xc[-1]] = ups["right"]
    if gh < 3:                                                       # no inner rows: the two corners of row 0 go sideways
        f[yc[0], xc[0]] = ups["left"]
        f[yc[0], xc[-1]] = ups["right"]
    return [f]


def warp_cases(h, w, gh, gw, k=WARP_K):
    """[(name, prev_grid, flow, certainty)]: previous grids over -1..k (both ends out of range), flows zero, constant
    (+2.25, -1.75), pushing probes through every edge, and one with a NaN and an inf at probe pixels; certainty None, all ones
    or a checkerboard of 0 / 1"""
    rng = np.random.default_rng(1000 * h + w + gh + gw)
    yc, xc = probes(gh, h), probes(gw, w)
    grids = [("random", rng.integers(-1, k + 1, size=(gh, gw)).astype(np.int32))]
    if gh * gw == 1:
        grids = [(f"const{v}", np.full((1, 1), v, dtype=np.int32)) for v in (-1, 1, k)]
    else:
        grids[0][1][0, 0], grids[0][1][-1, -1] = -1, k
    push = _push_flows(h, w, gh, gw, rng)
    bad = push[0].copy()
    bad[yc[0], xc[0], 0] = np.nan
    bad[yc[-1], xc[-1], 1] = np.inf
    flows = [("zero", np.zeros((h, w, 2), np.float32)),
             ("const", np.broadcast_to(np.float32([2.25, -1.75]), (h, w, 2)).copy())]
    flows += [(f"push{i}", f) for i, f in enumerate(push)] + [("nonfinite", bad)]
    yy, xx = np.mgrid[0:h, 0:w]
    certs = [("none", None), ("ones", np.ones((h, w), np.float32)), ("checker", ((yy + xx) % 2).astype(np.float32))]
    return [(f"{gn}-{fn}-{cn}", g, f, c) for gn, g in grids for fn, f in flows for cn, c in certs]


# ------------------------------------------------------------------ B. the biased assignment
def assign_prior(x, inv, n, d, centres, prior, beta):
    """(label int32, best, second, s, score): score_ij = s_ij + (prior_i == j ? beta : 0) in float64 (beta at its float32
    value); label = the first arg-max of the scores, best = the raw s of that j, second = the largest raw s of the others
    (-inf for one centre).  A row with inv == 0 has every s = 0: it takes its valid prior when beta > 0, else label 0, and
    best = second = 0 (as strotss_kmeans_assign has it)."""
    s = R.scores(x, inv, n, d, centres)
    k = s.shape[1]
    prior = np.asarray(prior[:n])
    score = s + (prior[:, None] == np.arange(k)[None, :]) * float(np.float32(beta))
    label = np.argmax(score, axis=1).astype(np.int32)
    best = s[np.arange(n), label]
    rest = s.copy()
    rest[np.arange(n), label] = -np.inf
    second = rest.max(axis=1) if k > 1 else np.full(n, -np.inf)
    zero = inv[:n] == 0
    best[zero], second[zero] = 0.0, 0.0
    return label, best, second, s, score


def biased_margin(score) -> np.ndarray:
    """per row: the top biased score minus the runner-up's (inf for one centre)"""
    if score.shape[1] == 1:
        return np.full(score.shape[0], np.inf)
    part = np.sort(score, axis=1)
    return part[:, -1] - part[:, -2]


def exact_rows(x, inv, n, d) -> np.ndarray:
    """rows whose scores are exactly 0 in float32 and in float64 alike (a zero row, inv_norm == 0): their labels are
    compared exactly whatever their margin"""
    return (inv[:n] == 0) | ~x[:n, :d].any(axis=1)


ASSIGN_SHAPES = [(1, 3, 1), (33, 35, 2), (1000, 35, 16), (4096, 2179, 5)]     # (n, d, k)
BETAS = (0.0, 0.05, 2.0)
_cases = {}


def assign_case(n, d, k):
    """(x, inv, c32, prior): planted non-negative rows with a zero row (1) and a row of inverse norm 0 (2) for n >= 3, float32
    centres one update after farthest-first, priors uniform in -1..k (none, every label, one value out of range); rows 1 and
    2 get a valid prior.  Computed once."""
    if (n, d, k) not in _cases:
        x, _ = R.planted_rows(n, d, k, 1.0, 2000 + n % 997 + d + k)
        inv = R.inv_norm(x, n)
        centres, _ = R.farthest_first(x, inv, n, d, k)
        label, _, _, _ = R.assign(x, inv, n, d, centres)
        centres, _ = R.update(x, inv, label, n, d, k, centres)
        c32 = np.zeros((k, x.shape[1]), dtype=np.float32)
        c32[:, :d] = centres
        prior = np.random.default_rng(n + d + k).integers(-1, k + 1, size=x.shape[0]).astype(np.int32)
        if n >= 3:
            x[1] = 0.0
            inv[1] = R.inv_norm(x, n)[1]
            inv[2] = 0.0
            prior[1], prior[2] = k - 1, k - 1
        _cases[(n, d, k)] = (x, inv, c32, prior)
    return _cases[(n, d, k)]
