"""Cases of the sliced palette term (strotss_palette_sliced_fwd_bwd).  A plain module, built on the CPU:
colours uniform in [0, 1], x = style rows (ns, 3), y = prediction rows (n, 3), directions nn.rand.palette_directions(P).
`ld` is the row stride the GPU test gives the rows (32 or 2208: the columns past the third hold values the entry must neither
read nor write), `rgb_to_yuv` the entry's flag.

TIE-FREE cases are compared element by element: float32 must decide no rank and no sign.  The builder searches row seeds (the
label's crc + try, at most TRIES) and keeps the first whose smallest float64 gap -- between neighbours within a sorted set and
between any a and any b of a direction -- is at least MIN_GAP = 2e-5.  With colours in [0, 1] that is only reachable at small
sizes: (n, ns) are one atom against one, two against one, one against a full wave, unequal sizes on both sides, exactly one
wave and the first cross-wave stage with unequal sizes, each with P = 1 and with P = 8.

The DUPLICATE case holds two identical prediction rows and two identical style rows: their ties are exact in every arithmetic
and the row index breaks them; every other gap is held to MIN_GAP, and the seed is one at which the two tied prediction rows
take different coefficients in some direction (so that the order of the tie shows in the gradient).

LINE cases are tie-free BY CONSTRUCTION, at the widths the product runs (S = 256, which no searched case reaches, 512 and 1024).
A search cannot reach them: 2048 colours in [0, 1] leave a direction's smallest neighbour gap near 1e-7, and every a-versus-b
gap counts as well.  Instead the m = n + ns points 0.5 + t_k u lie on ONE line through the cube's centre, t_k = 0.98 ((k + 0.5 +
U(-0.25, 0.25)) / m - 0.5), u of max-norm 1, so every colour stays in [0.01, 0.99]; the points are dealt at random to the two
sides and each side is permuted.  A direction's projections are 0.5 <dir, M 1> + t_k <dir, M u> (M the RGB->YUV matrix where the
flag is set): one grid for both sides, neighbours at least half a step apart, the step being 0.98 |<dir, M u>| / m.  u is the
best of LINE_TRIES seeded candidates by min_p |<dir_p, M u>| over the case's directions: 0.49 raw and 0.29 YUV at P = 8.  With
P = 1 u lies along the direction itself.  Measured gaps (float64, gap_of): 1.2e-4 raw and 7.2e-5 YUV at 1024 x 1024, 2.5e-4 and
1.5e-4 at 512 x 512; all at least 3.4 times MIN_GAP.  A random deal makes rank r of one side lead or trail rank r of the other by
a random walk, so the signs, and with them the coefficients, come in long runs: exchanging two neighbouring ranks changes the
gradient at only 14 of the 510 upper slots of 1024 x 1024 (tests/test_palette_sliced_cpu.py counts them).  The LINE_PAIRS case
deals points 2k and 2k + 1 one to each side by a coin: the sign of a_(r) - b_(r) is that coin, and every second exchange shows.

FULL-SHAPE cases (the step's own sizes) are not tie-free and are compared in norm (tests/_palette_sliced_ref.py)."""
import functools
import zlib

import numpy as np

import _palette_sliced_ref as PR

MIN_GAP = 2e-5
TRIES = 64


class Case:
    def __init__(self, label, n, ns, n_proj, ld, rgb_to_yuv, kind, x, y, seed, row_seed):
        self.label, self.n, self.ns, self.n_proj, self.ld, self.rgb_to_yuv, self.kind = label, n, ns, n_proj, ld, rgb_to_yuv, kind
        self.x, self.y, self.seed, self.row_seed = x, y, seed, row_seed

    @property
    def dirs(self):
        from nn import rand
        return rand.palette_directions(self.n_proj)


# (label, n, ns, P, ld, rgb_to_yuv, kind)
SPECS = [
    ("n1_ns1_p1", 1, 1, 1, 32, 1, "plain"),
    ("n1_ns1_p8", 1, 1, 8, 2208, 0, "plain"),
    ("n2_ns1_p1", 2, 1, 1, 2208, 1, "plain"),
    ("n2_ns1_p8", 2, 1, 8, 32, 0, "plain"),
    ("n1_ns64_p1", 1, 64, 1, 32, 0, "plain"),
    ("n1_ns64_p8", 1, 64, 8, 2208, 1, "plain"),
    ("n37_ns64_p1", 37, 64, 1, 2208, 1, "plain"),
    ("n37_ns64_p8", 37, 64, 8, 32, 0, "plain"),
    ("n64_ns37_p1", 64, 37, 1, 32, 0, "plain"),
    ("n64_ns37_p8", 64, 37, 8, 2208, 1, "plain"),
    ("n64_ns64_p1", 64, 64, 1, 2208, 0, "plain"),
    ("n64_ns64_p8", 64, 64, 8, 32, 1, "plain"),
    ("n65_ns33_p1", 65, 33, 1, 32, 1, "plain"),
    ("n65_ns33_p8", 65, 33, 8, 2208, 0, "plain"),
    ("n65_ns33_p4_dup", 65, 33, 4, 32, 1, "dup"),
    # constructed, no seed search: S = 256 ...
    ("line_n130_ns130_p8", 130, 130, 8, 32, 1, "line"),
    ("line_n256_ns200_p8", 256, 200, 8, 2208, 0, "line"),
    # ... S = 512 ...
    ("line_n257_ns512_p8", 257, 512, 8, 32, 0, "line"),
    ("line_n512_ns512_p8", 512, 512, 8, 2208, 1, "line"),
    # ... and S = 1024
    ("line_n513_ns300_p8", 513, 300, 8, 2208, 0, "line"),
    ("line_n1024_ns1024_p8", 1024, 1024, 8, 32, 1, "line"),
    ("line_n1024_ns1024_p1", 1024, 1024, 1, 2208, 0, "line"),     # u along the one direction: whole-number coefficients
    ("line_n1023_ns1024_p8", 1023, 1024, 8, 2208, 1, "line"),
    ("line_n1024_ns513_p8", 1024, 513, 8, 32, 0, "line"),
    ("line_n1024_ns1024_p8_pairs", 1024, 1024, 8, 2208, 0, "line_pairs"),
]
CONSTRUCTED = [s[0] for s in SPECS if s[6].startswith("line")]
LINE_TRIES = 4096
SWAP_LABEL, INTEGER_LABEL = "line_n1024_ns1024_p8", "line_n1024_ns1024_p1"


def width(n, ns):
    """the sort's width: the power of two >= max(n, ns), clamped to [64, 1024]"""
    S = 64
    while S < min(max(n, ns), 1024):
        S *= 2
    return S
ELEMENTWISE = [s[0] for s in SPECS]
TIE_FREE = [s[0] for s in SPECS if s[6] == "plain"]
DUP_LABEL = "n65_ns33_p4_dup"
DUP_PRED, DUP_STYLE = (5, 9), (3, 7)

# (label, n, ns, P, ld, rgb_to_yuv): seeded by the label, compared in norm
FULL = [
    ("full_n1024_ns1024_p64", 1024, 1024, 64, 2208, 1),
    ("full_n1024_ns1024_p1024", 1024, 1024, 1024, 32, 1),
    ("full_n1000_ns1024_p33", 1000, 1024, 33, 32, 0),
    ("full_n768_ns600_p64", 768, 600, 64, 32, 1),
    ("full_n1024_ns1_p64", 1024, 1, 64, 32, 1),
    ("full_n1_ns1024_p64", 1, 1024, 64, 32, 1),
]
FULL_LABELS = [s[0] for s in FULL]


def gap_of(case):
    """the smallest float64 gap of the case, the exact ties of the duplicate case left out"""
    return PR.min_gap(case.x, case.y, case.dirs, case.rgb_to_yuv, skip_exact=case.kind == "dup")


def tie_shows(case):
    """the duplicate case: the two tied prediction rows take different coefficients in some direction"""
    _, g = PR.palette_sliced(case.x, case.y, case.dirs, case.rgb_to_yuv)
    _, gm = PR.palette_sliced(case.x, case.y, case.dirs, case.rgb_to_yuv, descending_ties=True)
    return bool(np.abs(g - gm).max() > 1e-3 * np.abs(g).max())


def line_margin(u, n_proj, convert):
    """min_p |<dir_p, M u>|: what a step of t is worth in the direction that separates the points least"""
    from nn import rand
    mu = PR.yuv(np.asarray(u, np.float64)[None, :], convert)[0]
    return float(np.abs(rand.palette_directions(n_proj).astype(np.float64) @ mu).min())


@functools.lru_cache(maxsize=None)
def line_direction(n_proj, convert, seed):
    """u of max-norm 1: along the direction at P = 1, else the best of LINE_TRIES seeded candidates by line_margin"""
    from nn import rand
    if n_proj == 1:
        u = rand.palette_directions(1)[0].astype(np.float64)
        return u / np.abs(u).max()
    cand = np.random.default_rng(seed).standard_normal((LINE_TRIES, 3))
    cand /= np.abs(cand).max(1, keepdims=True)
    dirs = rand.palette_directions(n_proj).astype(np.float64)
    margins = np.abs(PR.yuv(cand, convert) @ dirs.T).min(1)
    return cand[int(np.argmax(margins))]


@functools.lru_cache(maxsize=None)
def make_case(label):
    spec = [s for s in SPECS if s[0] == label]
    assert spec, label
    _, n, ns, P, ld, convert, kind = spec[0]
    base = zlib.crc32(label.encode())
    if kind.startswith("line"):
        rng = np.random.default_rng(base)
        m = n + ns
        t = 0.98 * ((np.arange(m) + 0.5 + rng.uniform(-0.25, 0.25, m)) / m - 0.5)
        pts = 0.5 + t[:, None] * line_direction(P, convert, base)[None, :]
        deal = rng.permutation(m)
        if kind == "line_pairs":
            coin = rng.integers(0, 2, n)
            deal = np.concatenate([rng.permutation(2 * np.arange(n) + coin), rng.permutation(2 * np.arange(n) + 1 - coin)])
        c = Case(label, n, ns, P, ld, convert, kind, pts[deal[n:]], pts[deal[:n]], base, base)
        assert gap_of(c) >= MIN_GAP, (label, gap_of(c))
        return c
    for k in range(TRIES):
        rng = np.random.default_rng(base + k)
        x, y = rng.random((ns, 3)), rng.random((n, 3))
        if kind == "dup":
            x[DUP_STYLE[1]] = x[DUP_STYLE[0]]
            y[DUP_PRED[1]] = y[DUP_PRED[0]]
        c = Case(label, n, ns, P, ld, convert, kind, x, y, base, base + k)
        if gap_of(c) >= MIN_GAP and (kind != "dup" or tie_shows(c)):
            return c
    raise AssertionError(f"{label}: no seed in {TRIES} tries holds a gap of {MIN_GAP}")


@functools.lru_cache(maxsize=None)
def make_full(label):
    spec = [s for s in FULL if s[0] == label]
    assert spec, label
    _, n, ns, P, ld, convert = spec[0]
    base = zlib.crc32(label.encode())
    rng = np.random.default_rng(base)
    return Case(label, n, ns, P, ld, convert, "full", rng.random((ns, 3)), rng.random((n, 3)), base, base)


def case_of(label):
    return make_full(label) if label in FULL_LABELS else make_case(label)


def equal_case():
    """a prediction equal to the style set, row for row: loss 0, every coefficient 0 (sign(0) = 0)"""
    x = np.random.default_rng(77).random((64, 3))
    return Case("equal_n64_ns64_p8", 64, 64, 8, 32, 1, "equal", x, x.copy(), 77, 77)


def two_colour_case():
    """mass conservation: a style of 32 rows of one colour and 32 of another, a prediction of 64 rows of the first"""
    red, blue = np.array([0.9, 0.1, 0.1]), np.array([0.1, 0.1, 0.9])
    x = np.concatenate([np.tile(red, (32, 1)), np.tile(blue, (32, 1))])
    return Case("two_colours", 64, 64, 64, 32, 1, "mass", x, np.tile(red, (64, 1)), 0, 0), red, blue
