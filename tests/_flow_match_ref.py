"""numpy restatement of the optical flow's patch-matching stage, dtype-parametrised like
_flow_ref.py (float64: the statement; float32: the yardstick), shared by test_flow_match_cpu.py and test_hip_flow_match.py.

The stage, at one pyramid level with grey planes A, B (h, w), the level's flow (u, v) and a radius R in 1..4: for each
pixel p = (x, y) and each whole offset d = (dx, dy) in [-R, R]^2

    C(p, d) = sum over the 25 taps t = (tx, ty) in [-2, 2]^2, row-major (ty outer), of
              | A(qy, qx) - bilinear(B, qx + dx + u(p), qy + dy + v(p)) |,   qx = clamp(x + tx), qy = clamp(y + ty)

with _flow_ref.bilinear's rule.  The coordinate is never formed: u(p) = floor(u) + fu is split once per pixel, the taps are
the whole numbers qx + dx + floor(u) and one further (clamped), the weight is fu -- the same value in exact arithmetic
(test_flow_match_cpu.py compares the two in float64), and in float32 without the coordinate's rounding, which at x = 300
moves a sample by up to 1.5e-5 px: more than all the roundings of the lerp together.  d* is the first
minimiser in scan order (dy outer ascending, dx inner ascending) and replaces d = 0 only if C(p, d*) < C(p, 0) strictly;
F'(p) = F(p) + d*.  The flow of the centre pixel moves all 25 taps.

Plus the whole flow with the stage in (after the upsample / the zero start of every level, before its warps), the
conditioning of a stage case (which pixels float32 may decide otherwise) and the two-layer pair of frames."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
import _temporal_ref as T  # noqa: E402

WINDOW = 2                      # the 5 x 5 window's half width
MAX_RADIUS = 4


def offsets(radius):
    """[(dx, dy)] in scan order: dy outer ascending, dx inner ascending"""
    return [(dx, dy) for dy in range(-radius, radius + 1) for dx in range(-radius, radius + 1)]


FLOW_LIMIT = 1.0e6                # |F| is clamped there before it is split (every tap is the edge pixel long before)


def split(f):
    """(whole part as int64, fraction in [0, 1]) of a flow component: floor and f - floor (exact in float32 but for a
    negative f above -2^-25, whose fraction rounds to 1: the tap one further, the same value)"""
    dt = f.dtype.type
    fc = np.clip(f, dt(-FLOW_LIMIT), dt(FLOW_LIMIT))
    fl = np.floor(fc)
    return fl.astype(np.int64), fc - fl


def sample(b, ix, fx, iy, fy):
    """_flow_ref.bilinear's rule at (ix + fx, iy + fy), whole part and fraction given apart: the 4 neighbours clamped to
    the edge, the same lerp expression"""
    h, w = b.shape
    one = b.dtype.type(1)
    x0, x1 = np.clip(ix, 0, w - 1), np.clip(ix + 1, 0, w - 1)
    y0, y1 = np.clip(iy, 0, h - 1), np.clip(iy + 1, 0, h - 1)
    return ((one - fy) * ((one - fx) * b[y0, x0] + fx * b[y0, x1])
            + fy * ((one - fx) * b[y1, x0] + fx * b[y1, x1]))


def costs(a, b, u, v, radius):
    """C (n_offsets, h, w) of a's dtype, offsets in scan order"""
    dt = a.dtype.type
    assert b.dtype == a.dtype and u.dtype == a.dtype and v.dtype == a.dtype
    h, w = a.shape
    ys, xs = np.mgrid[0:h, 0:w]
    taps = [(tx, ty) for ty in range(-WINDOW, WINDOW + 1) for tx in range(-WINDOW, WINDOW + 1)]
    qx = np.stack([np.clip(xs + tx, 0, w - 1) for tx, _ in taps])            # (25, h, w)
    qy = np.stack([np.clip(ys + ty, 0, h - 1) for _, ty in taps])
    aq = a[qy, qx]
    (iu, fu), (iv, fv) = split(u), split(v)
    out = np.empty((len(offsets(radius)), h, w), dtype=a.dtype)
    for i, (dx, dy) in enumerate(offsets(radius)):
        term = np.abs(aq - sample(b, qx + dx + iu[None], fu[None], qy + dy + iv[None], fv[None]))
        c = term[0]
        for t in range(1, len(taps)):                                       # row-major, one rounding per addition
            c = c + term[t]
        out[i] = c
    assert out.dtype.type is dt
    return out


def choose(c, radius):
    """index (h, w) into offsets(radius) of d*: the first minimiser in scan order, and d = 0 unless d* is strictly better"""
    zero = offsets(radius).index((0, 0))
    best = np.argmin(c, axis=0)                                              # numpy: the first of equal minima
    cbest = np.take_along_axis(c, best[None], axis=0)[0]
    return np.where(cbest < c[zero], best, zero)


def stage(a, b, u, v, radius):
    """(u', v', chosen index) of the stage"""
    pick = choose(costs(a, b, u, v, radius), radius)
    off = np.array(offsets(radius))
    keep = pick == offsets(radius).index((0, 0))                             # d = 0: F itself, not F + 0 (-0.0 stays -0.0)
    return (np.where(keep, u, u + off[pick, 0].astype(a.dtype)), np.where(keep, v, v + off[pick, 1].astype(a.dtype)),
            pick)


def optical_flow(frame_a, frame_b, dtype=np.float64, match_radius=0, alpha2=0.01, warps=5, iters=32, min_side=12,
                 max_levels=8):
    """_flow_ref.optical_flow with the stage at every level; match_radius = 0: that function's arithmetic exactly"""
    pa = R.pyramid(frame_a, dtype, min_side, max_levels)
    pb = R.pyramid(frame_b, dtype, min_side, max_levels)
    u = v = np.zeros(pa[-1].shape, dtype=dtype)
    for k in range(len(pa) - 1, -1, -1):
        a, b = pa[k], pb[k]
        if u.shape != a.shape:
            u, v = R.upsample(u, *a.shape), R.upsample(v, *a.shape)
        if match_radius:
            u, v, _ = stage(a, b, u, v, match_radius)
        for _ in range(warps):
            ix, iy, c, inv = R.coefficients(a, b, u, v, alpha2)
            u, v = R.jacobi(u, v, ix, iy, c, inv, iters)
    assert u.dtype == dtype and v.dtype == dtype
    return np.stack([u, v], axis=-1)


# ------------------------------------------------------------------------------------------------ conditioning
def gamma32(k):
    """the float32 constant gamma_k = k u / (1 - k u), u = 2^-24 (Higham, Accuracy and Stability, section 3.1)"""
    u = 2.0 ** -24
    return k * u / (1 - k * u)


def cost_error(a, b):
    """E = 2 * 25 * gamma_8 * m, m = max |A, B|: the budget within which two float32 costs may change their order.
    One term |A(q) - s|: the fraction is exact (split), the weights 1 - f are one rounding each, s = wy0 * (wx0 * b00 +
    fx * b01) + fy * (...) puts at most 5 more on any path (*, +, *, +, with the outer weight's own) and the subtraction
    one: 7 roundings on values of at most m, so a term is within gamma_8 m of exact and 25 terms within 25 gamma_8 m.  Two
    costs: twice that.  The 24 additions of the sum come on top, at most gamma_24 C for a cost C; the budget covers them
    for C up to about 8 m only in the worst case -- they are rounding errors of random sign, and test_flow_match_cpu.py
    checks on every case that the float32 statement does decide each decided pixel as the float64 one does."""
    m = float(max(np.abs(a).max(), np.abs(b).max()))
    return 2 * 25 * gamma32(8) * m


def conditioning(c64, radius, e):
    """per pixel of a float64 cost volume: (pick, margin, allowed) -- the statement's choice, margin = second best - best
    with d = 0's rule included, and the (n_offsets, h, w) mask of the choices a float32 twin may make: every offset within
    e of the best cost, d = 0 among them.  A pixel is decided when margin > e: then allowed holds the pick alone.

    The rule for d = 0 makes one order of all offsets: the smallest cost wins, equal costs go to d = 0 and then to the
    first in scan order.  So the pick changes only if another VALUE comes to lie below the best one: second best = the
    smallest cost strictly above the minimum.  Offsets whose cost equals the minimum bit for bit are no rivals: where
    windows are clamped to the edge (always so in a 1 x 1 image), several offsets read the same 100 pixels with the same
    weights and get the same cost in any arithmetic, so the tie rule decides them alike in float32 and float64."""
    pick = choose(c64, radius)
    cmin = c64.min(axis=0)
    second = np.where(c64 > cmin[None], c64, np.inf).min(axis=0)
    margin = second - cmin
    allowed = c64 <= cmin[None] + e
    return pick, margin, allowed


# ------------------------------------------------------------------------------------------------ inputs
def smooth_flow(h, w, seed, amplitude=6.0):
    """a smooth random flow field (u, v) float32 with |u|, |v| up to `amplitude` px: the stage tests' input flows (sample
    windows leave the frame at that size)"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.uniform(0.03, 0.12, 4)
    q = rng.uniform(0, 6, 4)
    u = amplitude * np.sin(p[0] * xs + q[0]) * np.cos(p[1] * ys + q[1])
    v = amplitude * np.cos(p[2] * xs + q[2]) * np.sin(p[3] * ys + q[3])
    return u.astype(np.float32), v.astype(np.float32)


BACKGROUND_FLOW = (-1, 0)
BLOCK_FLOW = (4, -2)


def two_layer_pair(h, w, seed, block=(32, 40), at=(32, 40)):
    """(frame_a, frame_b, truth): a background moving by (-1, 0) and a block of another texture, `block` = (rows, cols)
    pasted at `at` = (row, col) in frame_a and 4 px right, 2 px up from there in frame_b, moving by (4, -2).  Frames float32
    (h, w, 3) rounded to 8 bits; truth (h, w, 2) = the flow of frame_a's pixels."""
    big = T.texture(h + 32, w + 32, seed)
    fg = T.texture(h + 32, w + 32, seed + 7)[16:16 + block[0], 16:16 + block[1]]
    a = big[16:16 + h, 16:16 + w].copy()
    b = big[16:16 + h, 16 - BACKGROUND_FLOW[0]:16 - BACKGROUND_FLOW[0] + w].copy()
    r, c = at
    a[r:r + block[0], c:c + block[1]] = fg
    b[r + BLOCK_FLOW[1]:r + BLOCK_FLOW[1] + block[0], c + BLOCK_FLOW[0]:c + BLOCK_FLOW[0] + block[1]] = fg
    truth = np.empty((h, w, 2))
    truth[...] = BACKGROUND_FLOW
    truth[r:r + block[0], c:c + block[1]] = BLOCK_FLOW

    def q8(x):
        return ((x * 255).round() / 255).astype(np.float32)
    return q8(a), q8(b), truth
