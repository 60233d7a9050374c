"""The seeded cases of the patch-matching stage's tests, shared by test_flow_match_cpu.py (which
proves that the cases meet their conditions) and test_hip_flow_match.py (which runs them on the device).  Every float64 /
float32 restatement is computed once per case and cached here, read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
import _flow_match_ref as M  # noqa: E402

# ------------------------------------------------------------------------------------------------ the stage alone
# flow_match.hip's tile is flow.hip's: 64 wide, 32 high
STAGE_SHAPES = [
    (1, 1), (2, 2), (3, 5), (2, 300), (300, 2),         # one pixel (every tap clamps to it), thinner than the window each way
    (31, 67), (32, 67), (33, 67),                       # one below, on and above the tile's 32 rows
    (45, 63), (45, 64), (45, 65),                       # ... and its 64 columns
    (37, 75),                                           # odd by odd, two tiles each way
]
STAGE_RADII = (1, 2, 4)
MAX_UNDECIDED = 0.05            # of a case's pixels
FLOW_AMPLITUDE = 6.0            # px: sample windows leave the frame


def stage_cases():
    """[(id, h, w, radius, seed)]"""
    return [(f"{h}x{w}-R{r}", h, w, r, 5000 + 11 * h + w + r) for h, w in STAGE_SHAPES for r in STAGE_RADII]


@functools.lru_cache(maxsize=None)
def stage_inputs(h, w, seed):
    """(a, b, u, v) float32 (h, w): the greys of a smooth random pair and a smooth random flow of up to 6 px"""
    fa, fb = R.smooth_pair(h, w, seed)
    a, b = R.grey(fa, np.float32), R.grey(fb, np.float32)
    u, v = M.smooth_flow(h, w, seed + 1, FLOW_AMPLITUDE)
    for x in (a, b, u, v):
        x.setflags(write=False)
    return a, b, u, v


@functools.lru_cache(maxsize=None)
def stage_reference(h, w, radius, seed):
    """dict of the float64 statement of a stage case: costs c (n, h, w), pick, margin, allowed (n, h, w), e, decided"""
    a, b, u, v = (x.astype(np.float64) for x in stage_inputs(h, w, seed))
    c = M.costs(a, b, u, v, radius)
    e = M.cost_error(a, b)
    pick, margin, allowed = M.conditioning(c, radius, e)
    ref = dict(c=c, pick=pick, margin=margin, allowed=allowed, e=e, decided=margin > e)
    for x in ref.values():
        if isinstance(x, np.ndarray):
            x.setflags(write=False)
    return ref


def check_stage(name, ref, radius, u, v, u_out, v_out):
    """the assertions of a stage result (float32 arrays) against a case's reference: -> (n undecided, n undecided that
    chose otherwise than float64).  The offset is recovered exactly: u_out - u is a whole number in [-R, R] or the pixel
    fails; u_out, v_out must be u + dx, v + dy bit for bit (u, v themselves for d = 0)."""
    off = np.array(M.offsets(radius))
    dx = np.rint(u_out.astype(np.float64) - u).astype(np.int64)
    dy = np.rint(v_out.astype(np.float64) - v).astype(np.int64)
    assert (np.abs(dx) <= radius).all() and (np.abs(dy) <= radius).all(), name
    got = (dy + radius) * (2 * radius + 1) + (dx + radius)
    zero = M.offsets(radius).index((0, 0))
    want_u = np.where(got == zero, u, u + off[got, 0].astype(np.float32))
    want_v = np.where(got == zero, v, v + off[got, 1].astype(np.float32))
    assert want_u.dtype == np.float32
    assert np.array_equal(u_out.view(np.int32), want_u.view(np.int32)), name
    assert np.array_equal(v_out.view(np.int32), want_v.view(np.int32)), name
    decided = ref["decided"]
    wrong = decided & (got != ref["pick"])
    assert not wrong.any(), (name, int(wrong.sum()), np.argwhere(wrong)[:5].tolist())
    ok = np.take_along_axis(ref["allowed"], got[None], axis=0)[0]
    assert ok[~decided].all(), (name, np.argwhere(~ok & ~decided)[:5].tolist())
    return int((~decided).sum()), int((~decided & (got != ref["pick"])).sum())


# ------------------------------------------------------------------------------------------------ the whole flow
FLOW_RADIUS = 2
FLOW_CASES = [(48, 64, 48 * 64), (42, 63, 42 * 63)]     # (h, w, seed of _flow_ref.smooth_pair): test_hip_flow.py's pairs
YARDSTICK_CAP = 5e-5            # _flow_cases.YARDSTICK_CAP: the device test allows 4 x a case's yardstick


@functools.lru_cache(maxsize=None)
def flow_reference(h, w, seed, radius=FLOW_RADIUS):
    """(F_f64 matched, yardstick = max |F_f32ref - F_f64ref|) of smooth_pair(h, w, seed)"""
    a, b = R.smooth_pair(h, w, seed)
    f64 = M.optical_flow(a, b, np.float64, radius)
    f32 = M.optical_flow(a, b, np.float32, radius)
    f64.setflags(write=False)
    return f64, float(np.abs(f32.astype(np.float64) - f64).max())


# ------------------------------------------------------------------------------------------------ the two-layer pair
PAIR_SHAPE = (96, 128)
PAIR_SEEDS = (0, 1)
PAIR_RADIUS = 2
# Measured on the float64 statement: interior mean EPE 0.4025 -> 0.3891 (seed 0) and 0.3593 -> 0.3531
# (seed 1), ratios 0.967 and 0.983.  1.5 x headroom over the larger ratio would put the bound ABOVE the unmatched value
# (1.47 x), so the bound is the unmatched value itself: PAIR_FACTOR = min(1, 1.5 x 0.983) = 1.
PAIR_FACTOR = 1.0


@functools.lru_cache(maxsize=None)
def pair(seed, shape=PAIR_SHAPE, block=(32, 40), at=(32, 40)):
    a, b, truth = M.two_layer_pair(shape[0], shape[1], seed, block, at)
    for x in (a, b, truth):
        x.setflags(write=False)
    return a, b, truth


@functools.lru_cache(maxsize=None)
def pair_unmatched_epe(seed):
    """interior mean EPE (margin 8) of the float64 statement WITHOUT the stage on the two-layer pair"""
    a, b, truth = pair(seed)
    return R.interior_epe(R.optical_flow(a, b), truth)[0]
