"""The Sinkhorn and pairwise-distance problems of tests/test_hip_sinkhorn.py, as seeded cases built on the CPU.  A plain
module (not a conftest): tests/test_sinkhorn_cases_cpu.py checks every case's conditioning, the float32 yardstick and the
negative controls; the GPU test runs the HIP entries at the same cases against tests/_sinkhorn_ref.py.

Rows come from _loss_cases.hyper_rows (RGB in columns 0..2; narrower cases keep the first d of three columns), each case
seeded by its label.  x = style rows (ns), y = prediction rows (n).

Conditioning of a Sinkhorn case (asserted on the CPU, _sinkhorn_ref.clamp_arguments): in float64 every argument of the two
clamp(., 1e-12) calls of every iteration is >= CLAMP_CLEAR = 1e-9 -- the clamps are inactive and three orders of magnitude
from acting, so f32 rounding cannot flip one.  l is 10 for 'cosine'; for 'l2' / 'both' the largest of L_CHOICES for which
the case is conditioned.  The ALL-CLAMPED case is the opposite: 'cosine' with l the first of L_CLAMPED for which every K v
argument is <= CLAMPED_BELOW (clamped by a factor of 4) and every K^T u argument is <= CLAMPED_BELOW or >= CLAMPED_ABOVE."""
import functools
import zlib

import numpy as np

import _loss_cases as LC

CLAMP_EPS = 1e-12
CLAMP_CLEAR = 1e-9
CLAMPED_BELOW, CLAMPED_ABOVE = 2.5e-13, 4e-12
L_COSINE = 10.0
L_CHOICES = (10.0, 5.0, 2.0)
L_CLAMPED = (100.0, 200.0, 400.0)
METRICS = ("cosine", "l2", "both")

# (label, n, ns, d, T, kind, metrics)
#   "dup": prediction rows 5 and 2 identical;  "clamp_pair": prediction row 7 and style row 11 are the same row of
#   _loss_cases.exact_rows (m = 1 + 1 - 2 = 0 exactly in f32 and f64: the l2 clamp acts, but y - x = 0 there, so whether it
#   passes gradient cannot show), and prediction row 9 is style row 13 (such a row / 32) plus 2^-12 in one of its four
#   columns: m = 2^-24 = 6e-8 exactly on every arithmetic (all terms are dyadic and fit f32), clamped by a factor of 16 with
#   y - x != 0 -- the pair on which a gradient let through the clamp shows.  The l2 clamp acts on no other pair;
#   "all_clamped": see above;  "far_row": see far_row_case
SPECS = [
    ("n1_ns33", 1, 33, 35, 30, "plain", METRICS),
    ("n15_ns300_below_col_chunks", 15, 300, 67, 30, "plain", METRICS),
    ("n17_ns1", 17, 1, 35, 5, "plain", METRICS),
    ("n37_ns65", 37, 65, 131, 30, "plain", METRICS),
    ("n64_ns64_d2179", 64, 64, 2179, 30, "plain", METRICS),
    ("n65_ns31_T2", 65, 31, 35, 2, "plain", METRICS),
    ("n100_ns31_rgb", 100, 31, 3, 30, "plain", METRICS),
    ("n50_ns40_d1", 50, 40, 1, 3, "plain", METRICS),
    ("n257_ns130_T1", 257, 130, 515, 1, "plain", METRICS),
    ("n130_ns257_T64", 130, 257, 131, 64, "plain", METRICS),
    ("n200_ns200_dup_rows", 200, 200, 35, 3, "dup", METRICS),
    ("n48_ns40_clamp_pair", 48, 40, 35, 3, "clamp_pair", ("l2", "both")),
    ("n37_ns65_all_clamped", 37, 65, 131, 3, "all_clamped", ("cosine",)),
    ("n4096_ns2_far_row", 4096, 2, 3, 2, "far_row", ("l2",)),
]
LABELS = [s[0] for s in SPECS]
DUP_ROWS = (5, 2)
CLAMP_PAIR = (7, 11)          # (prediction row, style row): identical rows
NEAR_PAIR = (9, 13)           # (prediction row, style row): 2^-12 apart in one column
FAR_ROW_SUM = 2e-9            # K v_0 of the far style row: clear of the clamp by 2000, below n * 1e-12 = 4.1e-9 by 2
PUBLIC_LABELS = ("n37_ns65", "n65_ns31_T2", "n200_ns200_dup_rows")      # also run through losses.sinkhorn_knopp


class Case:
    def __init__(self, label, n, ns, d, T, kind, metrics, x, y):
        self.label, self.n, self.ns, self.d, self.T, self.kind, self.metrics = label, n, ns, d, T, kind, metrics
        self.x, self.y = x, y

    @property
    def family_d(self):
        return "narrow" if self.d <= 3 else "wide"


def _rows(rng, m, d):
    return LC.hyper_rows(rng, m, max(d, 3))[:, :d].copy()


def _far_row(x, y, l):
    """Style row 0 becomes c * (1, 1, 1) with c such that sum_j exp(-l * l2(x_0, y_j)) = FAR_ROW_SUM (bisection in float64):
    K v_0 of that row is conditioned (>= 1e-9) only because v_0 = 1 -- from v_0 = 1 / n it would be 4.9e-13 and clamp.  The
    alternating scalings are otherwise invariant under v_0 -> c v_0, so this is the one case where the start value shows."""
    d = x.shape[1]

    def total(c):
        m = ((c - y) ** 2).sum(1)
        return np.exp(-l * np.sqrt(np.maximum(m, 1e-6) / d)).sum()
    lo, hi = 1.0, 20.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if total(mid) > FAR_ROW_SUM else (lo, mid)
    x[0] = 0.5 * (lo + hi)
    return x


U = 2.0 ** -24


def l2_margin(x, y, kind):
    """(ns, n) float64: m - (1e-6 + 2 dm), m = |x_i|^2 + |y_j|^2 - 2 x_i.y_j the argument of l2_distance's clamp(., 1e-6) and
    dm = (4 + sqrt(d)) U (|x_i|^2 + |y_j|^2 + 2 |x_i.y_j|) the f32 error of m (_loss_ref.remd): >= 0 where f32 rounding cannot
    make that clamp act.  The two planted pairs of a "clamp_pair" case (m exact on every arithmetic) count as clear.  Prediction
    rows that offend are redrawn from a derived seed."""
    G = x @ y.T
    nx, ny = (x * x).sum(1)[:, None], (y * y).sum(1)[None, :]
    margin = (nx + ny - 2.0 * G) - (1e-6 + 2.0 * (4.0 + np.sqrt(x.shape[1])) * U * (nx + ny + 2.0 * np.abs(G)))
    if kind == "clamp_pair":
        margin[CLAMP_PAIR[1], CLAMP_PAIR[0]] = margin[NEAR_PAIR[1], NEAR_PAIR[0]] = 0.0
    return margin


@functools.lru_cache(maxsize=None)
def make_case(label):
    spec = [s for s in SPECS if s[0] == label]
    assert spec, label
    _, n, ns, d, T, kind, metrics = spec[0]
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    x, y = _rows(rng, ns, d), _rows(rng, n, d)
    if kind == "clamp_pair":
        y[CLAMP_PAIR[0]] = x[CLAMP_PAIR[1]] = LC.exact_rows(rng, 1, d)[0]
        x[NEAR_PAIR[1]] = LC.exact_rows(rng, 1, d)[0] / 32.0
        y[NEAR_PAIR[0]] = x[NEAR_PAIR[1]]
        y[NEAR_PAIR[0], np.flatnonzero(x[NEAR_PAIR[1]])[0]] += 2.0 ** -12
    for attempt in range(50):
        if kind == "dup":
            y[DUP_ROWS[0]] = y[DUP_ROWS[1]]
        bad = np.flatnonzero((l2_margin(x, y, kind) < 0).any(0))
        if not len(bad):
            break
        r2 = np.random.default_rng([zlib.crc32(label.encode()), attempt + 1])
        for j in bad:
            y[j] = _rows(r2, 1, d)[0]
    else:
        raise AssertionError(f"case {label}: an l2 clamp stays within f32 rounding after 50 redraws")
    if kind == "far_row":
        x = _far_row(x, y, L_CHOICES[0])
    return Case(label, n, ns, d, T, kind, metrics, x, y)


def runs():
    """every (label, metric) the tests run"""
    return [(s[0], m) for s in SPECS for m in s[6]]


# ------------------------------------------------------------------ pairwise distances with gradients to both sides
# (label, nx, ny, d)
PAIR_SPECS = [
    ("pair_1x1", 1, 1, 35),
    ("pair_31x33_rgb", 31, 33, 3),
    ("pair_33x31", 33, 31, 131),
    ("pair_65x257", 65, 257, 67),
    ("pair_200x130", 200, 130, 515),
]
PAIR_LABELS = [s[0] for s in PAIR_SPECS]
PAIR_KINDS = ("cosine", "l2", "both")


@functools.lru_cache(maxsize=None)
def make_pair(label):
    """(x, y, G): the two row sets and the upstream gradient of their distance matrix"""
    _, nx, ny, d = [s for s in PAIR_SPECS if s[0] == label][0]
    rng = np.random.default_rng(zlib.crc32(label.encode()))
    return _rows(rng, nx, d), _rows(rng, ny, d), rng.standard_normal((nx, ny))


# ------------------------------------------------------------------ strotss_rows_gemm_bwd
ROWS_GEMM_N = (1, 31, 33, 64, 65, 200)
ROWS_GEMM_K = (1, 32, 33, 100, 257)
ROWS_GEMM_LD = (32, 64, 2208)
ROWS_GEMM_G = (1.0, -0.5)


def rows_gemm_problem(n, k, ld, seed, beyond_k=False):
    """Operands of dx += g r (W B - x r q): W (n, pad32(k)) with columns >= k zero (beyond_k: random too), B (pad32(k), ld),
    x (n, ld), r > 0, q."""
    rng = np.random.default_rng([seed, n, k, ld])
    kp = (k + 31) // 32 * 32
    W = rng.standard_normal((n, kp))
    B = rng.standard_normal((kp, ld))
    if not beyond_k:
        W[:, k:] = 0.0
    ops = (W, B, rng.standard_normal((n, ld)), rng.uniform(0.1, 2.0, n), rng.standard_normal(n))
    return tuple(a.astype(np.float32).astype(np.float64) for a in ops)      # exactly what the f32 entry is given
