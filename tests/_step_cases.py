"""The steps that combine the transport of the style term, the style side, a content-weight map and temporal targets
("Combined steps"): a table, not the product of the factors.  tests/test_step_cases_cpu.py computes
from it what it claims to cover and holds every case to the conditioning and the float32 yardstick below;
tests/test_hip_step_combos.py runs the engine on every case against tests/_step_ref.py.

Factors:  transport  remd | sinkhorn | sliced
          side       one style | blend of K = 2 | two regions (_transport_cases.step_masks)
          map        content-weight map off | on (the ramp_map of tests/test_hip_content_weight.py)
          targets    0 | 1 | 3 temporal targets (_long_targets and LAMS of tests/test_hip_temporal_long.py)
          size       64 x 64 | 42 x 64
The table holds (1) every pair of values of two factors at least once (the engine accepts them all), (2) every (sinkhorn or
sliced) x map on x side -- the path where the content term is the separate weighted entry and the transport term borrows
norms and panels from its workspace -- and (3) every (sinkhorn or sliced) x three targets.

Sample counts are those of _transport_cases.STEPS: 384 at 64 x 64, 300 at 42 x 64, 1024 with masks, 256 for the blend.
Sinkhorn: l = 10, T = 30.  Sliced: _sliced_cases.STEP_PROJECTIONS directions, key _sliced_cases.STEP_SEED, first draw 0.

Seeds are chosen on the CPU as the comment above _transport_cases.STEPS describes: the float64 step must hold no near-tie
that float32 rounding decides, and the condition is the yardstick of tests/test_step_cases_cpu.py (the restatement's own
float32 run within a quarter of TOL_SCALAR and GRAD_TOL, with one thread and with the machine's count).  Every row starts
from the seed _transport_cases gives its size and style side (0, 4, 5, 8); REJECTED lists what was tried and did not hold."""
import functools

import _sliced_cases as SLC
import _transport_cases as TC

TRANSPORTS = ("remd", "sinkhorn", "sliced")
SIDES = ("one", "blend", "regions")
MAPS = (False, True)
TARGETS = (0, 1, 3)
SIZES = ((64, 64), (42, 64))
FACTORS = (TRANSPORTS, SIDES, MAPS, TARGETS, SIZES)

SINKHORN_L, SINKHORN_T = 10.0, 30
BLEND_WEIGHTS = TC.BLEND_WEIGHTS

# (transport, side, map, targets, (h, w), seed)
TABLE = [
    ("remd", "one", True, 1, (64, 64), 0),
    ("remd", "regions", True, 3, (64, 64), 5),
    ("remd", "blend", False, 0, (42, 64), 8),
    ("sinkhorn", "one", True, 0, (64, 64), 0),
    ("sinkhorn", "one", False, 1, (42, 64), 4),
    ("sinkhorn", "blend", True, 3, (64, 64), 8),
    ("sinkhorn", "regions", True, 1, (64, 64), 5),
    ("sinkhorn", "regions", False, 3, (42, 64), 5),
    ("sliced", "one", True, 0, (42, 64), 4),
    ("sliced", "one", False, 3, (64, 64), 0),
    ("sliced", "blend", True, 1, (64, 64), 8),
    ("sliced", "regions", True, 3, (64, 64), 5),
    ("sliced", "regions", False, 0, (64, 64), 5),
]
# (transport, side, map, targets, (h, w), seed): what it measured in float32 (threads, scalar, gradient)
REJECTED = [
]


def label(row):
    t, side, cmap, n_t, (h, w), _ = row
    return f"{t}-{side}-{'map' if cmap else 'nomap'}-t{n_t}-{h}x{w}"


LABELS = [label(r) for r in TABLE]
ROWS = dict(zip(LABELS, TABLE))
assert len(ROWS) == len(TABLE)


def required(row):
    """the rows conditions (2) and (3) ask for"""
    return row[0] != "remd" and (row[2] or row[3] == 3)


def borrowing(row):
    """condition (2): the transport term borrows from the separate weighted content entry"""
    return row[0] != "remd" and row[2]


def n_samples(row):
    _, side, _, _, (h, w), _ = row
    return {"regions": 1024, "blend": 256}.get(side, 384 if (h, w) == (64, 64) else 300)


def transport_of(row):
    return {"remd": ("remd",), "sinkhorn": ("sinkhorn", SINKHORN_L, SINKHORN_T),
            "sliced": ("sliced", SLC.STEP_PROJECTIONS, SLC.STEP_SEED, 0)}[row[0]]


def blend_of(row):
    return BLEND_WEIGHTS if row[1] == "blend" else None


def masks_of(row):
    h, w = row[4]
    return TC.step_masks(h, w) if row[1] == "regions" else None


@functools.lru_cache(maxsize=None)
def problem(lb):
    """the inputs of case `lb` (_step_ref.step_problem); cached, treat as read-only"""
    import _step_ref as R
    row = ROWS[lb]
    (h, w) = row[4]
    return R.step_problem(h, w, n_samples(row), row[5], masks=masks_of(row), n_styles=2 if row[1] == "blend" else 1,
                          weight_map=row[2], n_targets=row[3])
