"""The loss problems the loss tests run, as seeded cases: (label, n, ns, d) plus the feature matrices, built on the CPU.
A plain module (not a conftest): tests/test_loss_cases_cpu.py checks on the CPU that every case meets its conditioning,
tests/test_hip_loss_terms.py runs every loss entry at every case against the float64 restatement of tests/_loss_ref.py.

Rows look like hypercolumns: ReLU-like non-negative columns at a level of their own per row, RGB in [0, 1] in columns 0..2.  `x` holds the style rows, `y`
the prediction rows, `c` the content rows; `gx` / `gy` name each row's duplicate group (rows made identical share one id).
Ties are identified by group, never by float64 equality: a BLAS may round identical rows differently at block edges.

Conditioning (what makes a relaxed-EMD gradient a function of the data and not of f32 rounding): for every cost matrix a
case is checked on (cosine, l2 and 'both' at the case's width, the palette's with and without the YUV conversion), every row
and column minimum is either an exact tie inside a duplicate group or lies more than TAU_C below the next distinct value,
and |R_X - R_Y| > TAU_C.  Rows that offend are redrawn from a derived seed until both hold."""
import functools

import numpy as np

import _regime
from _loss_ref import RGB2YUV, TAU_C

# (label, n, ns, d, kind): kind "plain" | "flat_style" | "flat_pred" | "exact_rows" | "public" | "regime" (rows of
# tests/_regime.py loss_rows: mostly zero, heavy-tailed, block scales 1 .. 100, dead columns)
CASES = [
    ("step", 1024, 1024, 2179, "plain"),
    ("ragged_n1000_ns777", 1000, 777, 2179, "plain"),
    ("ragged_n777_ns1000", 777, 1000, 2179, "plain"),
    ("tie_list_limit_ns2048", 1024, 2048, 2179, "plain"),
    ("small_region_n37", 37, 1500, 2179, "plain"),
    ("n1_clamp", 1, 64, 2179, "exact_rows"),
    ("n2_content_clamp", 2, 64, 2179, "exact_rows"),
    ("flat_style_1500_of_2048", 1024, 2048, 2179, "flat_style"),
    ("flat_pred_600_of_1024", 1024, 2048, 2179, "flat_pred"),
    ("second_column_trip_d3100", 200, 300, 3100, "public"),
    ("regime_n1000_ns777", 1000, 777, 2179, "regime"),
    ("regime_small_n37", 37, 300, 2179, "regime"),
]
LABELS = [c[0] for c in CASES]
FLAT_STYLE_ROWS = 1500
FLAT_PRED_ROWS = 600


def hyper_rows(rng, m, d):
    """ReLU rows with a level of their own (sparse dark rows to dense bright ones), as hypercolumns of an image's flat and
    textured regions: their cosine distances spread over most of [0, 1]"""
    level = rng.uniform(-2.0, 2.0, (m, 1))
    x = np.maximum(rng.standard_normal((m, d)) + level, 0) + 0.01 * rng.random((m, d))
    x[:, :3] = rng.random((m, 3))
    return x


def exact_rows(rng, m, d):
    """Rows of unit norm whose normalisation and self dot product are exact in f32 and bf16 (four entries of 0.5: one to
    three of them in RGB, the rest in random feature columns): their cosine self-distance is exactly 0, so a column of
    them meets the self-similarity's column-sum clamp the same way on every arithmetic."""
    x = np.zeros((m, d))
    for i in range(m):
        rgb = rng.permutation(3)[:int(rng.integers(1, 4))]
        x[i, rgb] = 0.5
        x[i, 3 + rng.permutation(d - 3)[:4 - len(rgb)]] = 0.5
    return x


def cost_matrices(x, y, d):
    """The float64 cost matrices (style rows x prediction rows) the relaxed-EMD entries minimise over, by name."""
    G = x @ y.T
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    rx, ry = 1.0 / np.sqrt(np.maximum(nx, 1e-12)), 1.0 / np.sqrt(np.maximum(ny, 1e-12))
    cos = 1.0 - G * rx[:, None] * ry[None, :]
    l2 = np.sqrt(np.maximum(nx[:, None] + ny[None, :] - 2.0 * G, 1e-6) / d)
    out = {"cos": cos, "l2": l2, "both": cos + l2}
    for name, a, b in (("palette_yuv", x[:, :3] @ RGB2YUV, y[:, :3] @ RGB2YUV), ("palette_rgb", x[:, :3], y[:, :3])):
        g3 = a @ b.T
        na, nb = (a * a).sum(1), (b * b).sum(1)
        ca = 1.0 - g3 / np.sqrt(np.maximum(na, 1e-12))[:, None] / np.sqrt(np.maximum(nb, 1e-12))[None, :]
        out[name] = ca + np.sqrt(np.maximum(na[:, None] + nb[None, :] - 2.0 * g3, 1e-6) / 3.0)
    return out


def min_gaps(C, gx, gy):
    """Per row and per column of C: (position of the minimum, gap to the next value outside the minimum's duplicate group,
    position of that value)."""
    out = []
    for M, g_other in ((C, gy), (C.T, gx)):
        j = M.argmin(1)
        same = g_other[None, :] == g_other[j][:, None]
        rest = np.where(same, np.inf, M)
        j2 = rest.argmin(1)
        out.append((j, rest[np.arange(M.shape[0]), j2] - M[np.arange(M.shape[0]), j], j2))
    return out


def offending(C, gx, gy, tau=TAU_C, fixed_y=False):
    """(style rows, prediction rows) to redraw so that every minimum of C is well separated; empty when conditioned.
    fixed_y: redraw style rows only (the prediction rows are shared with other style sets)."""
    (jr, gap_r, j2r), (ic, gap_c, i2c) = min_gaps(C, gx, gy)
    single_x = np.bincount(gx)[gx] == 1
    single_y = np.bincount(gy)[gy] == 1
    bx, by = set(), set()
    for i in np.nonzero(gap_r <= tau)[0]:
        if gap_r[i] == 0 and single_y[j2r[i]] and not fixed_y:     # two prediction rows alike in this cost: move one
            by.add(int(j2r[i]))
        elif single_x[i]:
            bx.add(int(i))
        elif single_y[j2r[i]] and not fixed_y:
            by.add(int(j2r[i]))
        else:
            raise AssertionError("a near tie between two duplicate groups cannot be redrawn")
    for j in np.nonzero(gap_c <= tau)[0]:
        if single_y[j] and not fixed_y:
            by.add(int(j))
        elif single_x[i2c[j]]:
            bx.add(int(i2c[j]))
        else:
            raise AssertionError("a near tie between two duplicate groups cannot be redrawn")
    return sorted(bx), sorted(by)


def branch_gap(C):
    return float(C.min(1).mean() - C.min(0).mean())


def conditioned(C, gx, gy, tau=TAU_C):
    bx, by = offending(C, gx, gy, tau)
    return not bx and not by and abs(branch_gap(C)) > tau


METRICS = ("cos", "l2", "both", "palette_yuv", "palette_rgb")


class Case:
    def __init__(self, label, n, ns, d, kind, x, y, c, gx, gy, redrawn):
        self.label, self.n, self.ns, self.d, self.kind = label, n, ns, d, kind
        self.x, self.y, self.c, self.gx, self.gy, self.redrawn = x, y, c, gx, gy, redrawn

    @property
    def dup_groups_y(self):
        return [np.nonzero(self.gy == g)[0] for g in np.unique(self.gy) if (self.gy == g).sum() > 1]


@functools.lru_cache(maxsize=None)
def make_case(label):
    spec = [c for c in CASES if c[0] == label]
    assert spec, label
    _, n, ns, d, kind = spec[0]
    seed = 1000 + LABELS.index(label)
    rng = np.random.default_rng(seed)
    rows = _regime.loss_rows if kind == "regime" else hyper_rows
    x, y, c = rows(rng, ns, d), rows(rng, n, d), rows(rng, n, d)
    gx, gy = np.arange(ns), np.arange(n)
    if kind == "exact_rows":
        y = exact_rows(rng, n, d)
        c = exact_rows(rng, 1, d).repeat(n, 0)               # identical content rows: every content column clamps
    if kind == "flat_style":
        grp = rng.permutation(ns)[:FLAT_STYLE_ROWS]
        x[grp] = x[grp[0]]
        gx[grp] = grp[0]
    if kind == "flat_pred":
        grp = rng.permutation(n)[:FLAT_PRED_ROWS]
        y[grp] = y[grp[0]]
        gy[grp] = grp[0]
    redrawn = 0
    for attempt in range(50):
        costs = cost_matrices(x, y, d)
        bad_x, bad_y = set(), set()
        for name in METRICS:
            bx, by = offending(costs[name], gx, gy)
            bad_x.update(bx); bad_y.update(by)
        if not bad_x and not bad_y:
            gaps = [abs(branch_gap(costs[m])) for m in METRICS]
            if min(gaps) > TAU_C:
                return Case(label, n, ns, d, kind, x, y, c, gx, gy, redrawn)
            bad_y = {int(np.flatnonzero(np.bincount(gy)[gy] == 1)[0])}     # R_X == R_Y within TAU_C: move one prediction row
        r2 = np.random.default_rng([seed, attempt + 1])
        for i in sorted(bad_x):
            x[i] = rows(r2, 1, d)[0]
        for j in sorted(bad_y):
            y[j] = (exact_rows if kind == "exact_rows" else rows)(r2, 1, d)[0]
        redrawn += len(bad_x) + len(bad_y)
    raise AssertionError(f"case {label}: not conditioned after 50 redraws")


def all_cases():
    return [make_case(lbl) for lbl in LABELS]


BLEND_NS = (1024, 777, 2048, 1500)
BLEND_WEIGHTS = (0.4, 0.3, 0.2, 0.1)


@functools.lru_cache(maxsize=None)
def blend_styles(k):
    """k style row sets (ns from BLEND_NS, the last one with a 300-row duplicate group) against the prediction rows of the
    "step" case, each conditioned against them by redrawing its own rows only."""
    base = make_case("step")
    out = []
    for s, ns in enumerate(BLEND_NS[:k]):
        seed = 2000 + s
        x = hyper_rows(np.random.default_rng(seed), ns, base.d)
        gx = np.arange(ns)
        if s == 3:
            x[100:400] = x[100]
            gx[100:400] = 100
        for attempt in range(50):
            costs = cost_matrices(x, base.y, base.d)
            bad = set()
            for name in ("cos", "palette_yuv"):
                bad.update(offending(costs[name], gx, base.gy, fixed_y=True)[0])
            if not bad:
                if min(abs(branch_gap(costs[m])) for m in ("cos", "palette_yuv")) > TAU_C:
                    break
                bad = {0}
            r2 = np.random.default_rng([seed, attempt + 1])
            for i in sorted(bad):
                x[i] = hyper_rows(r2, 1, base.d)[0]
        else:
            raise AssertionError(f"blend style {s}: not conditioned after 50 redraws")
        out.append((x, gx))
    return out
