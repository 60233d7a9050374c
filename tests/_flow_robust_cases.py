"""The seeded cases of the robust optical flow's tests, shared by test_flow_robust_cpu.py (which
proves that the cases meet their conditions) and test_hip_flow_robust.py (which runs them on the device).  Every float64 /
float32 restatement is computed once per case and cached here, read-only."""
import functools
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
import _flow_match_ref as M  # noqa: E402
import _flow_robust_ref as RB  # noqa: E402

# ------------------------------------------------------------------------------------------------ one weight update
# flow_robust.hip's tile is flow.hip's: 64 wide, 32 high, with a halo of K
STAGE_SHAPES = [
    (2, 2), (3, 5), (2, 300), (300, 2),                 # thinner than any halo each way
    (31, 67), (32, 67), (33, 67),                       # one below, on and above the tile's 32 rows
    (45, 63), (45, 64), (45, 65),                       # ... and its 64 columns
    (37, 75),                                           # odd by odd, two tiles each way
]
STAGE_KS = (1, 2, 4, 8)         # sweeps per launch: the plain kernel and the three blocked ones
STAGE_SWEEPS = 8                # iters / outer of the defaults: 8, 4, 2 launches or 1
STAGE_FLOW_AMPLITUDE = 2.0      # px: a flow with gradients, so that s varies


def stage_cases():
    """[(id, h, w, k, seed)]"""
    return [(f"{h}x{w}-K{k}", h, w, k, 7000 + 13 * h + w) for h, w in STAGE_SHAPES for k in STAGE_KS]


@functools.lru_cache(maxsize=None)
def stage_inputs(h, w, seed):
    """(coef (h, w, 4) = {Ix, Iy, c, 0}, u, v) float32: the float32 statement's coefficients of a smooth random pair warped
    along a smooth random flow of up to 2 px, and that flow"""
    fa, fb = R.smooth_pair(h, w, seed)
    a, b = R.grey(fa, np.float32), R.grey(fb, np.float32)
    u, v = M.smooth_flow(h, w, seed + 1, STAGE_FLOW_AMPLITUDE)
    ix, iy, c, _ = R.coefficients(a, b, u, v, 1.0)
    coef = np.stack([ix, iy, c, np.zeros_like(c)], axis=-1)
    assert coef.dtype == np.float32
    for x in (coef, u, v):
        x.setflags(write=False)
    return coef, u, v


@functools.lru_cache(maxsize=None)
def stage_reference(h, w, seed, dtype=np.float32):
    """(u', v', s, rG, k) of the statement in `dtype`: one weight update and STAGE_SWEEPS sweeps at the defaults"""
    coef, u, v = (x.astype(dtype) for x in stage_inputs(h, w, seed))
    out = RB.update(u, v, coef[..., 0], coef[..., 1], coef[..., 2], STAGE_SWEEPS, **{k: RB.DEFAULTS[k] for k in
                                                                                  ("alpha", "eps_d", "eps_s")})
    for x in out:
        assert x.dtype == dtype
        x.setflags(write=False)
    return out


# ------------------------------------------------------------------------------------------------ the whole flow
FLOW_CASES = [(48, 64, 48 * 64, 0), (42, 63, 42 * 63, 0), (48, 64, 48 * 64, 2), (42, 63, 42 * 63, 2)]   # (h, w, seed, R)
YARDSTICK_CAP = 5e-5            # section 14's: the device test allows 4 x a case's yardstick
F32_YARDSTICK = 4.0


@functools.lru_cache(maxsize=None)
def flow_reference(h, w, seed, radius):
    """(F_f64, yardstick = max |F_f32ref - F_f64ref|) of the robust statement on smooth_pair(h, w, seed)"""
    a, b = R.smooth_pair(h, w, seed)
    f64 = RB.optical_flow(a, b, np.float64, radius)
    f32 = RB.optical_flow(a, b, np.float32, radius)
    f64.setflags(write=False)
    return f64, float(np.abs(f32.astype(np.float64) - f64).max())


# ------------------------------------------------------------------------------------------------ the two-layer pair
PAIR_SHAPE = (96, 128)
PAIR_SEEDS = (0, 1)
PAIR_RADIUS = 2
# Measured on the float64 statement: interior mean EPE 0.4025 -> 0.1660 (seed 0) and 0.3593 -> 0.1403
# (seed 1), ratios 0.4124 and 0.3905.  1.5 x headroom over the larger ratio: 0.619, below the cap of 0.75.
PAIR_FACTOR = 0.619
PAIR_MEASURED = {0: (0.4025, 0.1660, 0.1686), 1: (0.3593, 0.1403, 0.1410)}   # seed: (Horn-Schunck, robust, robust + R = 2)
PAIR_YARDSTICK_CAP = 1e-3       # px: what float32 may cost on the pair (test_flow_robust_cpu.py says why not section 14's)


@functools.lru_cache(maxsize=None)
def pair(seed):
    a, b, truth = M.two_layer_pair(PAIR_SHAPE[0], PAIR_SHAPE[1], seed)
    for x in (a, b, truth):
        x.setflags(write=False)
    return a, b, truth


@functools.lru_cache(maxsize=None)
def pair_horn_schunck_epe(seed):
    """the reference of the pair's bound: interior mean EPE (margin 8) of _flow_ref.optical_flow in float64"""
    a, b, truth = pair(seed)
    return R.interior_epe(R.optical_flow(a, b), truth)[0]


def two_layer_frames(h=48, w=64, n=3):
    """(n frames in [0, 1] as _temporal_ref.texture makes them, truth of the last frame's backward flow): test_hip_flow_match.py's two-layer
    sequence: the background moves by (+1, 0) per frame and a 16 x 20 block by (-4, +2) per frame against the frame, so the
    backward flow of frame t against t-1 is (-1, 0) and (4, -2)"""
    import _temporal_ref as T
    big = T.texture(h + 32, w + 32, 0)
    fg = T.texture(h + 32, w + 32, 7)[16:32, 16:36]
    frames, truth = [], None
    for t in range(n):
        f = big[16:16 + h, 16 + (n - 1 - t):16 + (n - 1 - t) + w].copy()
        r, c = 22 - 2 * (n - 1 - t), 14 + 4 * (n - 1 - t)
        f[r:r + 16, c:c + 20] = fg
        frames.append(f)
        if t == n - 1:
            truth = np.empty((h, w, 2))
            truth[...] = (-1, 0)
            truth[r:r + 16, c:c + 20] = (4, -2)
    return frames, truth
