"""The seeded cases of strotss_optical_flow's stage, parameter and edge tests, shared by
test_flow_cpu.py (which proves that the cases meet their conditions) and test_hip_flow.py (which runs them on the device).
Frames come from _flow_ref.smooth_pair and translated_pair; every float64 / float32 restatement is computed once per case
and cached here, read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402

# ------------------------------------------------------------------------------------------------ stage sets
# Parameter sets that make the flow a short, non-contractive function of one or two kernels: no later sweep forgets an
# early error.  All with min_side = 1 (the level count is max_levels wherever a side can still be halved) and one sweep
# per launch.
STAGE_SETS = {
    # grey, blur and coefficients: from u = v = 0 the one sweep gives (-Ix c inv, -Iy c inv)
    "first_sweep": dict(max_levels=1, warps=1, iters=1, min_side=1, iters_per_launch=1),
    # also the stride-2 blur and the upsample (of the coarse level's one sweep)
    "two_levels": dict(max_levels=2, warps=1, iters=1, min_side=1, iters_per_launch=1),
    # the bilinear warp at a non-zero flow (the second warp's coefficients)
    "second_warp": dict(max_levels=1, warps=2, iters=1, min_side=1, iters_per_launch=1),
    # the neighbour average with clamped borders, and an odd number of (u, v) ping-pong swaps
    "odd_sweeps": dict(max_levels=1, warps=1, iters=3, min_side=1, iters_per_launch=1),
    # an odd launch count on the blocked kernel: 1 launch per warp, 3 warps, 2 levels
    "one_blocked_launch": dict(max_levels=2, warps=3, iters=8, min_side=1, iters_per_launch=8),
}

# flow.hip: #define FLOW_TW 64, #define FLOW_TH 32 (the blocked solver's tile: 64 wide, 32 high)
FLOW_TW, FLOW_TH = 64, 32
STAGE_SHAPES = [
    (2, 2), (2, 300), (300, 2), (3, 5), (42, 63),       # the entry's minimum, thinner than a tile each way, the old smallest
    (31, 67), (32, 67), (33, 67),                       # FLOW_TH - 1, FLOW_TH, FLOW_TH + 1 rows, an odd width
    (45, 63), (45, 64), (45, 65),                       # FLOW_TW - 1, FLOW_TW, FLOW_TW + 1 columns, an odd height
    (37, 75), (37, 73),                                 # odd by odd; second level (19, 38) and (19, 37): odd by odd again
]


def stage_cases():
    """[(id, h, w, seed, params)]"""
    return [(f"{name}-{h}x{w}", h, w, 1000 + 7 * h + w, dict(p)) for name, p in STAGE_SETS.items() for h, w in STAGE_SHAPES]


# ------------------------------------------------------------------------------------------------ parameter grid
GRID_SHAPES = [(42, 63), (97, 130)]
GRID_MOVES = ([dict(alpha2=a) for a in (1e-3, 0.1)] + [dict(warps=n) for n in (1, 3)] + [dict(iters=n) for n in (8, 24)]
              + [dict(max_levels=n) for n in (1, 2, 8)] + [dict(min_side=n) for n in (1, 6, 20)])


def _move_id(move):
    return "-".join(f"{k}={v:g}" for k, v in move.items())


# alpha2 = 1e-3 weakens the smoothness term tenfold, and on most smooth pairs the full solve is then ill-conditioned in
# the statement itself: with the grid's own seeds max |F_f32ref - F_f64ref| is 1.5e-4 px at 42 x 63 and 4.6 px at
# 97 x 130, far above YARDSTICK_CAP.  Those two cases keep their size and parameter and draw other frames: the first
# seeds found whose yardstick is below the cap (1.0e-5 and 7.9e-6).
GRID_SEEDS = {(42, 63, "alpha2=0.001"): 2111, (97, 130, "alpha2=0.001"): 29}


def grid_cases():
    """[(id, h, w, seed, params)]: the full solve, the defaults with one parameter moved"""
    return [(f"{_move_id(m)}-{h}x{w}", h, w, GRID_SEEDS.get((h, w, _move_id(m)), 2000 + h + w), dict(m))
            for h, w in GRID_SHAPES for m in GRID_MOVES]


# The level rule on its threshold, min_side = 12: halve while min(h_k, w_k) // 2 >= min_side.
#   (24, 40): 24 // 2 = 12: a second level;  (23, 40): 11: none.
#   (48, 50) -> (24, 25) -> (12, 13): three levels;  (47, 50) -> ceil(47 / 2) = 24, so (24, 25) -> (12, 13): three levels as
#   well (the rounded-UP half keeps the third level: a floor there would give 23 and stop at two);  (46, 50) -> (23, 25):
#   two levels, the size just below that threshold.
# `other`: parameters that force the other level count on the same frames (one level more or fewer).
THRESHOLDS = [
    dict(h=24, w=40, levels=2, other=dict(max_levels=1), other_levels=1),
    dict(h=23, w=40, levels=1, other=dict(min_side=11), other_levels=2),
    dict(h=48, w=50, levels=3, other=dict(max_levels=2), other_levels=2),
    dict(h=47, w=50, levels=3, other=dict(max_levels=2), other_levels=2),
    dict(h=46, w=50, levels=2, other=dict(min_side=11), other_levels=3),
]
THRESHOLD_PARAMS = dict(min_side=12)


def threshold_cases():
    """[(id, h, w, seed, params, levels, other params, other levels)]"""
    return [(f"{t['h']}x{t['w']}", t["h"], t["w"], 3000 + t["h"] + t["w"], dict(THRESHOLD_PARAMS), t["levels"],
             dict(THRESHOLD_PARAMS, **t["other"]), t["other_levels"]) for t in THRESHOLDS]


# ------------------------------------------------------------------------------------------------ degenerate frames
DEGENERATE_SHAPE = (42, 63)
ZERO_FLOW = ("identical", "constants")                  # the flow is exactly 0 everywhere
FINITE_FLOW = ("blocks", "far_translation")             # finite, and within the yardstick of float64


def degenerate_pair(name, h=DEGENERATE_SHAPE[0], w=DEGENERATE_SHAPE[1]):
    """(frame_a, frame_b) float32 (h, w, 3); for "identical" frame_b IS frame_a"""
    if name == "identical":
        a = R.smooth_pair(h, w, 11)[0]
        return a, a
    if name == "constants":
        return np.full((h, w, 3), 0.25, np.float32), np.full((h, w, 3), 0.75, np.float32)
    if name == "blocks":            # exact 0s and 1s in 11 x 16 blocks, moved by (1, 1) from the first frame to the second
        ys, xs = np.mgrid[0:h + 1, 0:w + 1]             # (7 x 9 blocks moved by (2, 1) have a yardstick of 8.9e-3: replaced)
        board = (((ys // 11) + (xs // 16)) % 2).astype(np.float32)
        board = np.repeat(board[..., None], 3, axis=-1)
        return np.ascontiguousarray(board[1:, 1:]), np.ascontiguousarray(board[:h, :w])
    if name == "far_translation":                       # 0.4 x the width: the warp's samples land outside the frame
        return R.translated_pair(h, w, (int(round(0.4 * w)), 0), seed=5)
    raise KeyError(name)


# ------------------------------------------------------------------------------------------------ cached restatements
def _key(params):
    return tuple(sorted(params.items()))


@functools.lru_cache(maxsize=None)
def _frames(h, w, seed):
    a, b = R.smooth_pair(h, w, seed)
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b


def frames(h, w, seed):
    return _frames(h, w, seed)


def ref_params(params):
    """the restatement's keyword arguments of a parameter set (it has no iters_per_launch: the sweeps are the same)"""
    return {k: v for k, v in params.items() if k != "iters_per_launch"}


@functools.lru_cache(maxsize=None)
def _reference(h, w, seed, key):
    a, b = _frames(h, w, seed)
    kw = ref_params(dict(key))
    f64 = R.optical_flow(a, b, np.float64, **kw)
    f32 = R.optical_flow(a, b, np.float32, **kw)
    f64.setflags(write=False)
    return f64, float(np.abs(f32.astype(np.float64) - f64).max())


def reference(h, w, seed, params):
    """(F_f64, yardstick = max |F_f32ref - F_f64ref|) of smooth_pair(h, w, seed) under params, computed once"""
    return _reference(h, w, seed, _key(params))


@functools.lru_cache(maxsize=None)
def degenerate_reference(name):
    a, b = degenerate_pair(name)
    f64 = R.optical_flow(a, b, np.float64)
    f32 = R.optical_flow(a, b, np.float32)
    f64.setflags(write=False)
    f32.setflags(write=False)
    return f64, f32


def n_levels(h, w, params):
    full = dict(R.DEFAULTS, **ref_params(params))
    return len(R.level_sizes(h, w, full["min_side"], full["max_levels"]))


# The cap on every case's yardstick (test_flow_cpu.py asserts it): the device test allows F32_YARDSTICK x yardstick, so no
# case may bring a yardstick so large that a wrong kernel hides behind it.  The largest of all the cases here is 2.1e-5 px
# (one_blocked_launch at 2 x 300, max |F| = 10 px; the next are 1.8e-5 at 300 x 2 and 1.2e-5 for the far translation);
# the cap is about 2.4 x that.  A case above it is replaced, not excused.
YARDSTICK_CAP = 5e-5


def workspace_bytes(h, w, params):
    """strotss_flow_workspace_bytes as level_sizes implies it: two pyramids (a float plane per level each), u and v twice
    (four full-size float planes) and one f32x4 plane, each rounded up to 256 bytes as Workspace::take rounds"""
    full = dict(R.DEFAULTS, **ref_params(params))

    def take(nbytes):
        return (nbytes + 255) & ~255
    total = sum(2 * take(4 * hk * wk) for hk, wk in R.level_sizes(h, w, full["min_side"], full["max_levels"]))
    return total + 4 * take(4 * h * w) + take(16 * h * w)
