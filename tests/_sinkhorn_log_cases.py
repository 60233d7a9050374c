"""Cases of the log-domain Sinkhorn term (strotss_sinkhorn_log_cos_fwd_bwd_panels), built on the CPU: a
plain module like tests/_sinkhorn_cases.py.  x = style rows (ns), y = prediction rows (n), rows from
_loss_cases.hyper_rows, cosine cost only.

Sizes: the smallest problem; n below the column pass's 16 row chunks (empty chunks) and n = 17 (a short last chunk); the
64-column block edge and the 256-thread reduction edge on either side; the shortest and the longest sweep; the range of L on
one shape; rows the linear form clamps (the far-row construction of _transport_cases at L = 100, once with empty chunks);
and the step's own shapes at d = 2179.

Seeds: a case's rows are seeded by (crc32 of its label, try), and its try is the first of TRIES for which the float32 run
of the restatement lies within CAP / MARGIN of its float64 run (_sinkhorn_log_ref) -- `search` does it, the table pins what
it found, tests/test_sinkhorn_log_cpu.py asserts the pin for the cases below FULL_FROM elements and the bound for all.
L_MAX is the largest L of the L range: 500, the first value tried, met the cap at the first seed."""
import functools
import zlib

import numpy as np

import _sinkhorn_cases as SC
import _transport_cases as TC

TRIES = 64
L_MAX = 500.0
FULL_FROM = 300000           # n * ns from which a case counts as a full shape (searched once, pinned; not searched in the suite)

# (label, ns, n, d, T, L, kind, try)
SPECS = [
    ("ns1_n1", 1, 1, 35, 30, 10.0, "plain", 0),
    ("ns5_n3_empty_chunks", 5, 3, 35, 30, 10.0, "plain", 0),
    ("ns40_n15_empty_chunks", 40, 15, 35, 30, 10.0, "plain", 0),
    ("ns33_n17_short_chunk", 33, 17, 35, 30, 10.0, "plain", 0),
    ("ns63_n65", 63, 65, 35, 30, 10.0, "plain", 0),
    ("ns65_n63", 65, 63, 35, 30, 10.0, "plain", 0),
    ("ns257_n256", 257, 256, 35, 30, 10.0, "plain", 0),
    ("ns256_n257", 256, 257, 35, 30, 10.0, "plain", 0),
    ("ns200_n256_T1", 200, 256, 35, 1, 10.0, "plain", 0),
    ("ns200_n256_T64", 200, 256, 35, 64, 10.0, "plain", 0),
    ("ns200_n256_L1", 200, 256, 35, 30, 1.0, "plain", 0),
    ("ns200_n256_L10", 200, 256, 35, 30, 10.0, "plain", 0),
    ("ns200_n256_L100", 200, 256, 35, 30, 100.0, "plain", 0),
    ("ns200_n256_Lmax", 200, 256, 35, 30, L_MAX, "plain", 0),
    ("ns40_n300_far_row_L100", 40, 300, 35, 30, 100.0, "far_row", 0),
    ("ns40_n15_far_row_L100_empty_chunks", 40, 15, 35, 30, 100.0, "far_row", 0),
    ("ns1024_n1024_d2179_L10", 1024, 1024, 2179, 30, 10.0, "plain", 0),
    ("ns1024_n1024_d2179_L100", 1024, 1024, 2179, 30, 100.0, "plain", 0),
    ("ns600_n768_d2179_L10", 600, 768, 2179, 30, 10.0, "plain", 0),
    ("ns600_n768_d2179_L100", 600, 768, 2179, 30, 100.0, "plain", 0),
]
LABELS = [s[0] for s in SPECS]
FAR_ROW_LABEL = "ns40_n300_far_row_L100"
FAR_ROW_EMPTY_LABEL = "ns40_n15_far_row_L100_empty_chunks"


class Case(SC.Case):
    def __init__(self, label, n, ns, d, T, kind, x, y, l, seed_try):
        super().__init__(label, n, ns, d, T, kind, ("cosine",), x, y)
        self.l, self.seed_try = l, seed_try

    @property
    def full(self):
        return self.n * self.ns >= FULL_FROM


def build(label, seed_try):
    spec = [s for s in SPECS if s[0] == label]
    assert spec, label
    _, ns, n, d, T, l, kind, _ = spec[0]
    rng = np.random.default_rng([zlib.crc32(label.encode()), seed_try])
    x, y = SC._rows(rng, ns, d), SC._rows(rng, n, d)
    if kind == "far_row":
        # style row 0 opposite to the prediction rows' mean direction (_transport_cases._far_row; the l it finds is for the
        # linear form's v_0 control and is not used): every cost of that row is near 2, and at L = 100 its K v is exp(-200) n
        x, _ = TC._far_row(x, y)
    return Case(label, n, ns, d, T, kind, x, y, l, seed_try)


@functools.lru_cache(maxsize=None)
def make_case(label):
    return build(label, [s for s in SPECS if s[0] == label][0][7])


def err32(case):
    """(gradient, loss) distance of the restatement's float32 run from its float64 run"""
    import torch
    import _sinkhorn_log_ref as LR
    l64, g64 = LR.run(case.x, case.y, case.l, case.T)
    l32, g32 = LR.run(case.x, case.y, case.l, case.T, torch.float32)
    return LR.err_over_max(g32, g64), abs(l32 - l64) / abs(l64)


def search(label):
    """the first try whose float32 yardstick meets the cap, with both distances"""
    import _sinkhorn_log_ref as LR
    for k in range(TRIES):
        eg, el = err32(build(label, k))
        if LR.MARGIN * max(eg, el) <= LR.CAP:
            return k, eg, el
    raise AssertionError(f"{label}: no seed in {TRIES} tries meets the cap")


def all_cases():
    return [make_case(lb) for lb in LABELS]


def conditioned_linear_cases():
    """the conditioned cosine cases of _sinkhorn_cases.py (every one but the all-clamped case), where the linear statement
    engages no clamp at L = 10"""
    return [SC.make_case(s[0]) for s in SC.SPECS if "cosine" in s[6] and s[5] != "all_clamped"]
