"""float64 restatement of the temporal term of frame sequences, shared by test_temporal_cpu.py and
test_hip_temporal.py: the warp along the backward flow, its certainty (with the conditioning of its threshold tests), L_t and
its gradient, .flo writing, a synthetic sequence of a texture translated by a whole number of pixels per frame with its exact
flows, and the seeded cases of strotss_flow_warp's shape, channel, border and non-finite tests."""
import functools
import os

import numpy as np


def _taps(s, n):
    """the taps of one axis for the coordinates s: a NaN becomes -2, everything else is clamped to [-2, n + 1] (beyond it
    both taps are the edge pixel already, +-inf included), then lo = floor, hi = floor + 1, both clamped to [0, n - 1]"""
    with np.errstate(invalid="ignore"):
        s = np.where(np.isnan(s), -2.0, np.clip(s, -2.0, n + 1.0))
    fl = np.floor(s)
    i = fl.astype(np.int64)
    return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), s - fl


def bilinear(img, sx, sy):
    """img (h, w, c) sampled at (sx, sy) (each (h, w)): pixel centres at integer coordinates, 4 neighbours clamped.  A
    coordinate outside [0, n - 1] gives the edge pixel of its axis: 0 for s < 0, -inf and NaN, n - 1 for s > n - 1 and
    +inf; the result is finite wherever img is."""
    h, w = img.shape[:2]
    x0, x1, fx = _taps(sx, w)
    y0, y1, fy = _taps(sy, h)
    fx, fy = fx[..., None], fy[..., None]
    img = img.astype(np.float64)
    with np.errstate(invalid="ignore"):                 # a non-finite img (a planted forward flow): 0 * inf = NaN, as on the device
        return ((1 - fy) * ((1 - fx) * img[y0, x0] + fx * img[y0, x1]) + fy * ((1 - fx) * img[y1, x0] + fx * img[y1, x1]))


def warp64(prev, flow_b):
    h, w = flow_b.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fb = flow_b.astype(np.float64)
    with np.errstate(invalid="ignore"):
        return bilinear(prev, xs + fb[..., 0], ys + fb[..., 1])


def _slack(lhs, rhs):
    """relative slack |lhs - rhs| / max(|lhs|, |rhs|) of a test lhs > rhs; inf where an operand is not finite (the
    comparison is then decided by inf / NaN rules, not by rounding)"""
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        m = np.maximum(np.abs(lhs), np.abs(rhs))
        s = np.abs(lhs - rhs) / m
    return np.where(np.isfinite(lhs) & np.isfinite(rhs) & (m > 0), s, np.inf)


def certainty64(flow_b, flow_f=None, slack=False):
    """the {0, 1} certainty of strotss_flow_warp.  Non-finite flows follow from IEEE comparisons, as on the device: a NaN or
    infinite sample coordinate is not inside the frame (certainty 0); a threshold test whose left side is NaN (a NaN
    neighbour, or inf - inf) is not `>` and removes nothing; one whose left side is +inf against a finite right side
    removes the pixel.  slack=True: -> (certainty, s), s(p) the smallest relative slack of the threshold tests the device
    evaluates at p (the disocclusion test inside the frame, the motion-boundary test where the pixel is still certain),
    inf where it evaluates none: how far the float64 comparisons are from flipping under another rounding."""
    h, w = flow_b.shape[:2]
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    fb = flow_b.astype(np.float64)
    u, v = fb[..., 0], fb[..., 1]
    with np.errstate(invalid="ignore", over="ignore"):
        sx, sy = xs + u, ys + v
        ok = (sx >= 0) & (sx <= w - 1) & (sy >= 0) & (sy <= h - 1)
        fb2 = u * u + v * v
        least = np.full((h, w), np.inf)
        if flow_f is not None:
            wf = bilinear(flow_f, sx, sy)
            su, sv = u + wf[..., 0], v + wf[..., 1]
            lhs, rhs = su * su + sv * sv, 0.01 * (fb2 + wf[..., 0] ** 2 + wf[..., 1] ** 2) + 0.5
            least = np.where(ok, np.minimum(least, _slack(lhs, rhs)), least)
            ok &= ~(lhs > rhs)
        xm, xp = np.clip(np.arange(w) - 1, 0, w - 1), np.clip(np.arange(w) + 1, 0, w - 1)
        ym, yp = np.clip(np.arange(h) - 1, 0, h - 1), np.clip(np.arange(h) + 1, 0, h - 1)
        ux, vx = (u[:, xp] - u[:, xm]) * 0.5, (v[:, xp] - v[:, xm]) * 0.5
        uy, vy = (u[yp] - u[ym]) * 0.5, (v[yp] - v[ym]) * 0.5
        lhs, rhs = (ux * ux + uy * uy) + (vx * vx + vy * vy), 0.01 * fb2 + 0.002
        least = np.where(ok, np.minimum(least, _slack(lhs, rhs)), least)
        ok &= ~(lhs > rhs)
    return (ok.astype(np.float64), least) if slack else ok.astype(np.float64)


def temporal_loss64(x, target, cert):
    """(L_t, dL_t/dx) = ((1/(3hw)) sum_p c(p) |x(p) - target(p)|^2, its gradient), x / target (h, w, 3), cert (h, w)"""
    h, w = cert.shape
    d = x.astype(np.float64) - target.astype(np.float64)
    c = cert.astype(np.float64)[..., None]
    return float((c * d * d).sum() / (3 * h * w)), 2.0 * c * d / (3 * h * w)


def write_flo(path, flow):
    flow = np.asarray(flow, dtype=np.float32)
    h, w = flow.shape[:2]
    with open(path, "wb") as f:
        f.write(np.float32(202021.25).tobytes())
        f.write(np.array([w, h], dtype="<i4").tobytes())
        f.write(flow.astype("<f4").tobytes())


def texture(h, w, seed):
    """a smooth random RGB texture (h, w, 3) in [0, 1]"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((h // 6 + 2, w // 6 + 2, 3))
    ys = np.linspace(0, coarse.shape[0] - 1.001, h)
    xs = np.linspace(0, coarse.shape[1] - 1.001, w)
    sx, sy = np.meshgrid(xs, ys)
    return np.clip(bilinear(coarse, sx, sy) * 0.8 + 0.1 * rng.random((h, w, 3)), 0.0, 1.0)


def translated_sequence(dirpath, flow_dir, n_frames=3, h=60, w=80, shift=(3, 2), seed=0):
    """n_frames frames of one texture moved by shift = (dx, dy) pixels per frame (frame t shows the texture at offset
    t * shift: content at p in frame t came from p - shift in frame t-1), written as frame_{t}.png, with the exact flows
    backward_{t}_{t-1}.flo = -shift and forward_{t-1}_{t}.flo = +shift.  -> list of frame paths."""
    from PIL import Image
    dx, dy = shift
    big = texture(h + n_frames * dy + 8, w + n_frames * dx + 8, seed)
    os.makedirs(dirpath, exist_ok=True)
    os.makedirs(flow_dir, exist_ok=True)
    paths = []
    for t in range(n_frames):
        oy, ox = (n_frames - t) * dy, (n_frames - t) * dx
        frame = big[oy:oy + h, ox:ox + w]
        p = os.path.join(dirpath, f"frame_{t + 1:02d}.png")
        Image.fromarray((frame * 255).round().astype(np.uint8)).save(p)
        paths.append(p)
    for t in range(2, n_frames + 1):
        write_flo(os.path.join(flow_dir, f"backward_{t}_{t - 1}.flo"), np.broadcast_to(np.float32([-dx, -dy]), (h, w, 2)))
        write_flo(os.path.join(flow_dir, f"forward_{t - 1}_{t}.flo"), np.broadcast_to(np.float32([dx, dy]), (h, w, 2)))
    return paths


def consistency_error(outs, flow_b, flow_f=None):
    """E = mean over the frames t > 1 and the pixels with c = 1 of (out_t - warp(out_{t-1}))^2, outs (h, w, 3) in [0, 1]"""
    cert = certainty64(flow_b, flow_f).astype(bool)
    errs = []
    for prev, cur in zip(outs[:-1], outs[1:]):
        d = cur.astype(np.float64) - warp64(prev, flow_b)
        errs.append((d[cert] ** 2).mean())
    return float(np.mean(errs))


# ------------------------------------------------------------------------------------------------ cases of strotss_flow_warp
WARP_SHAPES = [(1, 1), (1, 7), (7, 1), (2, 2), (33, 71), (257, 300)]
WARP_CHANNELS = (1, 3, 4)
# The device evaluates the float64 threshold tests with FMA contraction and numpy does not: the two sides of a test can
# differ by a few ulp of float64 (2^-53 = 1.1e-16 each, a few operations deep: below 1e-14 relative to the larger side,
# cancellation in f_b + f_f included, since the slack is relative to the test's sides and not to the cancelled sum).  A case
# whose every evaluated test is further than this margin from equality has the same certainty under either rounding; 1e-9
# leaves five orders of magnitude.  Derived, not measured.
SLACK_MARGIN = 1e-9


def smooth_flow(h, w, seed, amp=3.0):
    """a few pixels of displacement, gradients mostly below the motion-boundary threshold"""
    rng = np.random.default_rng(seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    f = np.zeros((h, w, 2))
    for k in range(2):
        a, b, p, q = rng.uniform(0.01, 0.06, 4)
        f[..., k] = amp * (np.sin(a * xs + p * 7) * np.cos(b * ys + q * 5)) + rng.uniform(-2, 2)
    return f.astype(np.float32)


def random_warp_case(h, w, with_forward, flow_seed=1):
    """(prev (h, w, 3), flow_b, flow_f or None) of test_flow_warp_matches_float64: a smooth backward flow and, with_forward,
    roughly its inverse, wrong in a band: some pixels disoccluded, most not"""
    rng = np.random.default_rng(h * w)
    prev = rng.random((h, w, 3)).astype(np.float32)
    fb = smooth_flow(h, w, flow_seed)
    ff = None
    if with_forward:
        ff = (-fb + rng.normal(0, 0.05, fb.shape)).astype(np.float32)
        ff[h // 3: h // 3 + 5] += 3.0
    return prev, fb, ff


def min_slack(fb, ff):
    return float(certainty64(fb, ff, slack=True)[1].min())


def warp_prev(h, w, c):
    return np.random.default_rng(100 * h + w + c).random((h, w, c)).astype(np.float32)


HALF_SHIFTS = [(dx, dy) for dx in (-1.5, 0.0, 1.5) for dy in (-1.5, 0.0, 1.5) if (dx, dy) != (0.0, 0.0)]     # off every side and corner
WHOLE_SHIFTS = [(0, 0), (1, 0), (0, 1), (-1, -1), (2, -1), (-2, 1)]
_UP, _DOWN = np.float32(np.inf), np.float32(-np.inf)
# the next float32 beyond a whole shift: x + u is exact in float64, so the sample is just outside the frame at the border
BEYOND_SHIFTS = [(np.nextafter(np.float32(1), _UP), np.float32(0)), (np.float32(0), np.nextafter(np.float32(1), _UP)),
                 (np.nextafter(np.float32(-1), _DOWN), np.nextafter(np.float32(-1), _DOWN))]
PLANTED = [(1e9, 0.0), (0.0, -1e9), (np.inf, 0.0), (0.0, -np.inf), (np.nan, 0.0), (0.0, np.nan), (np.nan, np.nan),
           (np.inf, -np.inf), (-np.inf, np.nan)]


def _constant(h, w, shift):
    return np.ascontiguousarray(np.broadcast_to(np.asarray(shift, dtype=np.float32), (h, w, 2)))


def _planted_case(h, w, seed):
    """ordinary flows with huge, infinite and NaN vectors planted at single pixels of the backward flow (their neighbours'
    motion-boundary tests read them) and an infinite and a NaN vector in the forward flow"""
    rng = np.random.default_rng(seed)
    fb = smooth_flow(h, w, seed, amp=1.0) * np.float32(0.5)
    ff = (-fb + rng.normal(0, 0.05, fb.shape)).astype(np.float32)
    spots = rng.permutation(h * w)
    for (pu, pv), p in zip(PLANTED, spots):
        fb[p // w, p % w] = (pu, pv)
    for val, p in zip(((np.inf, 0.0), (np.nan, np.nan)), spots[len(PLANTED):]):
        ff[p // w, p % w] = val
    return fb, ff


def _redrawn(make, h, w, base_seed):
    """the first seed from base_seed on whose case keeps every evaluated test SLACK_MARGIN from equality, with and without
    the forward flow"""
    for seed in range(base_seed, base_seed + 50):
        fb, ff = make(h, w, seed)
        if min(min_slack(fb, None), min_slack(fb, ff)) > SLACK_MARGIN:
            return fb, ff
    raise AssertionError((make.__name__, h, w))


def _smooth_case(h, w, seed):
    rng = np.random.default_rng(seed)
    fb = smooth_flow(h, w, seed)
    ff = (-fb + rng.normal(0, 0.05, fb.shape)).astype(np.float32)
    ff[h // 3: h // 3 + 5] += 3.0
    return fb, ff


@functools.lru_cache(maxsize=None)
def warp_cases(h, w):
    """[(name, flow_b, flow_f)] float32 (h, w, 2), read-only; every case runs with flow_f and with None"""
    cases = [("smooth", *_redrawn(_smooth_case, h, w, 7 * h + w))]
    for kind, shifts in (("half", HALF_SHIFTS), ("whole", WHOLE_SHIFTS), ("beyond", BEYOND_SHIFTS)):
        for dx, dy in shifts:
            cases.append((f"{kind}({float(dx):g},{float(dy):g})", _constant(h, w, (dx, dy)), _constant(h, w, (-dx, -dy))))
    # every sample beyond the clamp of the coordinate ([-2, n + 1]): the forward flow would be sampled out of range
    cases.append(("far", _constant(h, w, (w + 2.25, -(h + 0.5))), _smooth_case(h, w, 3)[1]))
    cases.append(("planted", *_redrawn(_planted_case, h, w, 11 * h + w)))
    for _, fb, ff in cases:
        fb.setflags(write=False)
        ff.setflags(write=False)
    return cases
