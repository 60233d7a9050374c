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
]
TIE_FREE = [s[0] for s in SPECS if s[5] == "plain"]
ELEMENTWISE = [s[0] for s in SPECS]
DUP_LABEL, SIGN_LABEL = "n64_ns64_p4_dup", "n64_ns64_p2_sign"
DUP_PRED, DUP_STYLE = (5, 9), (3, 7)

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
        if case.kind == "dup":
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
