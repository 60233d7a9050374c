"""Cases of the sliced Wasserstein style term (strotss_sliced_cos_fwd_bwd).  A plain module, built on
the CPU: rows from _loss_cases.hyper_rows, x = style rows (ns), y = prediction rows (n), directions the draw `t` of the Philox
stream with key `seed` (nn.rand.sliced_signs).

TIE-FREE cases are compared element by element: float32 must not decide a rank.  The builder searches row seeds (the label's
crc + try, at most TRIES) and keeps the first whose smallest gap between sorted neighbours, over all directions and both
sides and computed in float64, is at least MIN_GAP = 2e-5: about ten times the float32 error of an O(1) dot product of at most
35 terms.  (n, ns, P) are the sizes at which the kernels take another path: one atom against several, exactly one wave, the
first cross-wave stage, unequal sizes on both sides, a single sign word (d = 3), long overlap loops.

The DUPLICATE case holds two identical prediction rows and two identical style rows: their ties are exact in every arithmetic
and the row index breaks them, as the stable sort of the restatement does; every other gap is held to MIN_GAP.  The SIGN case
holds projections of both signs and an exact zero: prediction row 0 is made orthogonal to direction 0.

ARC cases are tie-free BY CONSTRUCTION, at the widths the product runs (max(n, ns) in 257 .. 1024, where the sort has six or ten
cross-wave stages).  A search cannot reach them: among 1024 random rows the smallest of the ~1023 neighbour gaps of ONE direction
is about 1e-6, and a seed whose every direction and side holds 2e-5 turns up with a probability of about 1e-9 per try.  Instead
row i is s_i (cos th_i, sin th_i, 0.5), th_i = lo + (hi - lo)(i + 0.5 + U(-0.25, 0.25)) / m on lo = pi/4 + 0.3, hi = 3 pi/4 - 0.3,
s_i uniform in [0.5, 2] (so the reciprocal norms differ), the rows then permuted at random.  On that range sin th > |cos th|, so
the projection on every direction (+-1, +-1, +-1) is strictly monotone in th -- descending where the first sign is +1, ascending
where it is -1: the case tables give each case P >= 4 and tests/test_sliced_cpu.py asserts that both occur -- and neighbours
are at least half a grid step apart: (hi - lo) / (2 m) * sqrt(2) sin(0.3) / sqrt(1.25) = 1.8e-4 at m = 1024.  The wide form
(d = 35) holds (cos th, sin th) in columns 0 and 1 and ONE fixed non-zero tail of norm 0.5 in columns 2 .. 34 of every row of both
sides: the tail adds a constant to a direction's projections and leaves the gaps alone.  Measured gaps (float64, gap_of):
1.99e-4 at 1024 x 1024 (d = 3 and d = 35), 2.28e-4 at 1024 x 513, 4.3e-4 at 257 x 512; all at least nine times MIN_GAP.  The ARC
DUPLICATE case copies row 5 to row 900 on both sides: the tied pair starts in two different waves, so the row index has to
break the tie across cross-wave stages.

FULL-SHAPE cases (the step's own sizes, d = 2179) are not tie-free -- a smallest float64 gap of 8e-9 was seen at 1024 x 1024
with 256 directions -- and are compared in norm (tests/_sliced_ref.py)."""
import functools
import zlib

import numpy as np

import _loss_cases as LC
import _sliced_ref as SR

MIN_GAP = 2e-5
TRIES = 64
DRAW_T = 3            # the draw number of every operator case: not 0, so that the counter's value shows


class Case:
    def __init__(self, label, n, ns, d, n_proj, kind, seed, x, y, row_seed):
        self.label, self.n, self.ns, self.d, self.n_proj, self.kind, self.seed = label, n, ns, d, n_proj, kind, seed
        self.x, self.y, self.row_seed, self.t = x, y, row_seed, DRAW_T

    @property
    def signs(self):
        from nn import rand
        return rand.sliced_signs(self.seed, self.t, self.n_proj, self.d)


# (label, n, ns, d, P, kind)
SPECS = [
    ("n1_ns1_p1", 1, 1, 35, 1, "plain"),
    ("n1_ns5_p2", 1, 5, 35, 2, "plain"),
    ("n5_ns1_p2", 5, 1, 35, 2, "plain"),
    ("n64_ns64_p8", 64, 64, 35, 8, "plain"),
    ("n65_ns40_p4", 65, 40, 35, 4, "plain"),
    ("n96_ns33_p2_rgb", 96, 33, 3, 2, "plain"),
    ("n130_ns130_p4", 130, 130, 35, 4, "plain"),
    ("n256_ns200_p2", 256, 200, 35, 2, "plain"),
    ("n3_ns200_p2", 3, 200, 35, 2, "plain"),
    ("n200_ns3_p2", 200, 3, 35, 2, "plain"),
    ("n64_ns64_p4_dup", 64, 64, 35, 4, "dup"),
    ("n64_ns64_p2_sign", 64, 64, 35, 2, "sign"),
    # constructed, no seed search: S = 512 ...
    ("arc_n257_ns512_p8", 257, 512, 3, 8, "arc"),              # the first slot past 256
    ("arc_n512_ns512_p4", 512, 512, 35, 4, "arc"),
    # ... and S = 1024
    ("arc_n513_ns300_p4", 513, 300, 35, 4, "arc"),             # the smallest
    ("arc_n1024_ns1024_p4", 1024, 1024, 3, 4, "arc"),
    ("arc_n1024_ns1024_p4_wide", 1024, 1024, 35, 4, "arc"),
    ("arc_n1023_ns1024_p4", 1023, 1024, 3, 4, "arc"),          # coprime: every cell overlaps two
    ("arc_n1024_ns513_p4", 1024, 513, 35, 4, "arc"),
    ("arc_n1024_ns1_p4", 1024, 1, 3, 4, "arc"),                # the one-atom limits of the cell walk at full width
    ("arc_n1_ns1024_p4", 1, 1024, 35, 4, "arc"),
    ("arc_n1024_ns1024_p4_dup", 1024, 1024, 35, 4, "arc_dup"),
]
TIE_FREE = [s[0] for s in SPECS if s[5] == "plain"]
ELEMENTWISE = [s[0] for s in SPECS]
CONSTRUCTED = [s[0] for s in SPECS if s[5].startswith("arc")]
DUP_LABEL, SIGN_LABEL = "n64_ns64_p4_dup", "n64_ns64_p2_sign"
DUP_PRED, DUP_STYLE = (5, 9), (3, 7)
ARC_DUP_LABEL = "arc_n1024_ns1024_p4_dup"
ARC_DUP = (5, 900)                                             # on both sides: wave 0 and wave 14
ARC_LO, ARC_HI = np.pi / 4 + 0.3, 3 * np.pi / 4 - 0.3
SWAP_LABEL = "arc_n1024_ns1024_p4_wide"                        # the planted rank swap of tests/test_sliced_cpu.py


def width(n, ns):
    """the sort's width: the power of two >= max(n, ns), clamped to [64, 1024]"""
    S = 64
    while S < min(max(n, ns), 1024):
        S *= 2
    return S

# (label, n, ns, d, P): seeded by the label, compared in norm
FULL = [
    ("full_n1024_ns1024_p256", 1024, 1024, 2179, 256),
    ("full_n768_ns600_p64", 768, 600, 2179, 64),
    ("full_n1000_ns1024_p33", 1000, 1024, 2179, 33),
    ("full_n1024_ns1024_p1024", 1024, 1024, 2179, 1024),
]
FULL_LABELS = [s[0] for s in FULL]


def _rows(rng, m, d):
    return LC.hyper_rows(rng, m, max(d, 3))[:, :d].copy()


def _arc_tail(rng, d):
    """columns 2 .. d - 1 of every arc row before its scale: 0.5 at d = 3, else d - 2 non-zero entries of norm 0.5"""
    tail = rng.uniform(0.5, 1.0, d - 2) * rng.choice([-1.0, 1.0], d - 2)
    return 0.5 * tail / np.linalg.norm(tail)


def _arc_rows(rng, m, tail):
    theta = ARC_LO + (ARC_HI - ARC_LO) * (np.arange(m) + 0.5 + rng.uniform(-0.25, 0.25, m)) / m
    rows = np.empty((m, 2 + len(tail)))
    rows[:, 0], rows[:, 1], rows[:, 2:] = np.cos(theta), np.sin(theta), tail[None, :]
    rows *= rng.uniform(0.5, 2.0, m)[:, None]
    return rows[rng.permutation(m)]


def gap_of(case):
    """the smallest gap between sorted neighbours (float64), the exact ties of the duplicate case left out"""
    import torch
    s = torch.as_tensor(case.signs, dtype=torch.float64)
    worst = float("inf")
    for rows, dup in ((case.x, DUP_STYLE), (case.y, DUP_PRED)):
        v = torch.sort(SR.projections(torch.as_tensor(rows, dtype=torch.float64), s), dim=1)[0]
        if v.shape[1] < 2:
            continue
        gaps = (v[:, 1:] - v[:, :-1]).numpy()
        if case.kind.endswith("dup"):
            zero = gaps == 0.0
            assert (zero.sum(1) == 1).all(), "the duplicate case holds one exact tie per direction and side"
            gaps = np.where(zero, np.inf, gaps)
        worst = min(worst, float(gaps.min()))
    return worst


@functools.lru_cache(maxsize=None)
def make_case(label):
    spec = [s for s in SPECS if s[0] == label]
    assert spec, label
    _, n, ns, d, P, kind = spec[0]
    base = zlib.crc32(label.encode())
    from nn import rand
    if kind.startswith("arc"):
        rng = np.random.default_rng(base)
        tail = _arc_tail(rng, d)
        x, y = _arc_rows(rng, ns, tail), _arc_rows(rng, n, tail)
        if kind == "arc_dup":
            x[ARC_DUP[1]] = x[ARC_DUP[0]]
            y[ARC_DUP[1]] = y[ARC_DUP[0]]
        c = Case(label, n, ns, d, P, kind, base, x, y, base)
        assert gap_of(c) >= MIN_GAP, (label, gap_of(c))
        return c
    for k in range(TRIES):
        rng = np.random.default_rng(base + k)
        x, y = _rows(rng, ns, d), _rows(rng, n, d)
        if kind == "dup":
            x[DUP_STYLE[1]] = x[DUP_STYLE[0]]
            y[DUP_PRED[1]] = y[DUP_PRED[0]]
        if kind == "sign":
            # prediction row 0: two equal entries where direction 0 holds +1 and -1, zeros elsewhere
            e0 = rand.sliced_signs(base, DRAW_T, P, d)[0]
            y[0] = 0.0
            y[0, int(np.flatnonzero(e0 > 0)[0])] = 0.75
            y[0, int(np.flatnonzero(e0 < 0)[0])] = 0.75
        c = Case(label, n, ns, d, P, kind, base, x, y, base + k)
        if gap_of(c) >= MIN_GAP:
            if kind == "sign":
                import torch
                a = SR.projections(torch.as_tensor(y, dtype=torch.float64), torch.as_tensor(c.signs, dtype=torch.float64))
                assert float(a[0, 0]) == 0.0 and bool((a[0] < 0).any()) and bool((a[0] > 0).any())
            return c
    raise AssertionError(f"{label}: no seed in {TRIES} tries holds a gap of {MIN_GAP}")


@functools.lru_cache(maxsize=None)
def make_full(label):
    spec = [s for s in FULL if s[0] == label]
    assert spec, label
    _, n, ns, d, P = spec[0]
    base = zlib.crc32(label.encode())
    rng = np.random.default_rng(base)
    return Case(label, n, ns, d, P, "full", base, _rows(rng, ns, d), _rows(rng, n, d), base)


# ------------------------------------------------------------------ the step-level problems
# (label, h, w, samples, seed, masked): tests/_transport_cases.STEPS' sizes.  The seeds are those of that table where the
# restatement's own float32 run stays within a quarter of the step's bounds (tests/test_sliced_cpu.py asserts it); a seed
# that had to change is noted beside it.
STEPS = [
    ("step_64x64", 64, 64, 384, 0, False),
    ("step_42x64", 42, 64, 300, 4, False),
    ("step_64x64_two_regions", 64, 64, 1024, 5, True),      # (n, ns) = (768, 600) and (1024, 1024)
]
BLEND_WEIGHTS = (0.7, 0.3)
BLEND_STEP = ("step_64x64_blend", 64, 64, 256, 8, False)       # two styles, BLEND_WEIGHTS
STEP_PROJECTIONS = 32
STEP_SEED = 0
