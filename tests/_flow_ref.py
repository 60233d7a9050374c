"""numpy restatement of strotss_optical_flow, shared by test_flow_cpu.py and test_hip_flow.py:
coarse-to-fine Horn-Schunck with warping, solved by Jacobi iterations.  Every array is of `dtype` (float64: the statement
the kernels are tested against; float32: the yardstick of what the number format itself costs), so the two runs differ
only in their rounding.  Plus a pair of frames of one texture translated by a whole number of pixels."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _temporal_ref as T  # noqa: E402

DEFAULTS = dict(alpha2=0.01, warps=5, iters=32, min_side=12, max_levels=8)


def grey(img, dtype=np.float64):
    """(h, w, 3) -> (h, w): 0.299 R + 0.587 G + 0.114 B"""
    x = np.asarray(img).astype(dtype)
    return dtype(0.299) * x[..., 0] + dtype(0.587) * x[..., 1] + dtype(0.114) * x[..., 2]


def _clamped(n, d):
    return np.clip(np.arange(n) + d, 0, n - 1)


def blur(g):
    """separable binomial [1 4 6 4 1] / 16, along the rows (x) and then along the columns (y), indices clamped"""
    dt = g.dtype.type
    h, w = g.shape
    r = (g[:, _clamped(w, -2)] + g[:, _clamped(w, 2)] + dt(4) * (g[:, _clamped(w, -1)] + g[:, _clamped(w, 1)])
         + dt(6) * g) / dt(16)
    return (r[_clamped(h, -2)] + r[_clamped(h, 2)] + dt(4) * (r[_clamped(h, -1)] + r[_clamped(h, 1)]) + dt(6) * r) / dt(16)


def level_sizes(h, w, min_side=12, max_levels=8):
    """[(h_k, w_k)], finest first: halved (rounded up) while min(h_k, w_k) // 2 >= min_side, at most max_levels"""
    sizes = [(h, w)]
    while min(sizes[-1]) // 2 >= min_side and len(sizes) < max_levels:
        hk, wk = sizes[-1]
        sizes.append(((hk + 1) // 2, (wk + 1) // 2))
    return sizes


def pyramid(img, dtype=np.float64, min_side=12, max_levels=8):
    levels = [blur(grey(img, dtype))]
    for _ in level_sizes(*levels[0].shape, min_side, max_levels)[1:]:
        levels.append(np.ascontiguousarray(blur(levels[-1])[::2, ::2]))
    return levels


def bilinear(img, sx, sy):
    """img (h, w) sampled at (sx, sy): the rule of _temporal_ref.bilinear (pixel centres at integer coordinates, the 4
    neighbours clamped to the edge), every operand of img's dtype"""
    dt = img.dtype.type
    h, w = img.shape

    def taps(s, n):
        s = np.clip(s, dt(-2), dt(n + 1))
        fl = np.floor(s)
        i = fl.astype(np.int64)
        return np.clip(i, 0, n - 1), np.clip(i + 1, 0, n - 1), s - fl
    x0, x1, fx = taps(sx, w)
    y0, y1, fy = taps(sy, h)
    one = dt(1)
    return ((one - fy) * ((one - fx) * img[y0, x0] + fx * img[y0, x1])
            + fy * ((one - fx) * img[y1, x0] + fx * img[y1, x1]))


def upsample(u, h, w):
    """the flow component u of a coarser level at the size (h, w) of the next finer one: 2 * bilinear(u, x / 2, y / 2)"""
    dt = u.dtype.type
    ys, xs = np.mgrid[0:h, 0:w]
    return dt(2) * bilinear(u, xs.astype(u.dtype) / dt(2), ys.astype(u.dtype) / dt(2))


def coefficients(a, b, u, v, alpha2):
    """(Ix, Iy, c, inv) of one warp: B warped along (u, v), its central differences with clamped indices, the constant
    of the linearised data term and 1 / (alpha2 + Ix^2 + Iy^2)"""
    dt = a.dtype.type
    h, w = a.shape
    ys, xs = np.mgrid[0:h, 0:w]
    bw = bilinear(b, xs.astype(a.dtype) + u, ys.astype(a.dtype) + v)
    ix = (bw[:, _clamped(w, 1)] - bw[:, _clamped(w, -1)]) / dt(2)
    iy = (bw[_clamped(h, 1)] - bw[_clamped(h, -1)]) / dt(2)
    c = bw - a - ix * u - iy * v
    inv = dt(1) / (dt(alpha2) + ix * ix + iy * iy)
    return ix, iy, c, inv


def _average(u):
    dt = u.dtype.type
    h, w = u.shape
    ym, yp, xm, xp = _clamped(h, -1), _clamped(h, 1), _clamped(w, -1), _clamped(w, 1)
    n, s = u[ym], u[yp]
    return ((n + s + u[:, xm] + u[:, xp]) / dt(6)
            + (n[:, xm] + n[:, xp] + s[:, xm] + s[:, xp]) / dt(12))


def jacobi(u, v, ix, iy, c, inv, iters):
    for _ in range(iters):
        ub, vb = _average(u), _average(v)
        t = (ix * ub + iy * vb + c) * inv
        u, v = ub - ix * t, vb - iy * t
    return u, v


def optical_flow(frame_a, frame_b, dtype=np.float64, alpha2=0.01, warps=5, iters=32, min_side=12, max_levels=8):
    """F (h, w, 2) = (u, v) with frame_a(p) ~ frame_b(p + F(p)); frames (h, w, 3) in [0, 1]"""
    pa = pyramid(frame_a, dtype, min_side, max_levels)
    pb = pyramid(frame_b, dtype, min_side, max_levels)
    u = v = np.zeros(pa[-1].shape, dtype=dtype)
    for k in range(len(pa) - 1, -1, -1):
        a, b = pa[k], pb[k]
        if u.shape != a.shape:
            u, v = upsample(u, *a.shape), upsample(v, *a.shape)
        for _ in range(warps):
            ix, iy, c, inv = coefficients(a, b, u, v, alpha2)
            u, v = jacobi(u, v, ix, iy, c, inv, iters)
    assert u.dtype == dtype and v.dtype == dtype
    return np.stack([u, v], axis=-1)


# ------------------------------------------------------------------------------------------------ inputs and measures
def translated_pair(h, w, shift, seed=0):
    """(frame_prev, frame_cur) float32 (h, w, 3) in [0, 1], rounded to 8 bits as _temporal_ref.translated_sequence writes
    its frames: one texture, moved by shift = (dx, dy) whole pixels from the first to the second (content at p in
    frame_cur came from p - shift in frame_prev).  flow(frame_cur, frame_prev) = -shift, flow(frame_prev, frame_cur) =
    +shift."""
    dx, dy = shift
    m = 8 + max(abs(dx), abs(dy))
    big = T.texture(h + 2 * m, w + 2 * m, seed)

    def cut(oy, ox):
        return ((big[oy:oy + h, ox:ox + w] * 255).round() / 255).astype(np.float32)
    return cut(m + dy, m + dx), cut(m, m)


def smooth_pair(h, w, seed):
    """a random smooth pair with a non-constant motion of a few pixels: the second frame is the first one sampled along a
    smooth displacement field (float32, not rounded to 8 bits)"""
    rng = np.random.default_rng(seed)
    a = T.texture(h, w, seed)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float64)
    p = rng.uniform(0.02, 0.08, 4)
    q = rng.uniform(0, 6, 4)
    dx = 2.0 * np.sin(p[0] * xs + q[0]) * np.cos(p[1] * ys + q[1]) + rng.uniform(-1.5, 1.5)
    dy = 2.0 * np.cos(p[2] * xs + q[2]) * np.sin(p[3] * ys + q[3]) + rng.uniform(-1.5, 1.5)
    b = T.bilinear(a, xs + dx, ys + dy)
    return a.astype(np.float32), b.astype(np.float32)


def interior_epe(flow, truth, margin=8):
    """(mean, max) endpoint error with `margin` pixels removed on every side; truth = (u, v)"""
    d = np.asarray(flow, dtype=np.float64) - np.asarray(truth, dtype=np.float64)
    e = np.sqrt((d ** 2).sum(-1))[margin:-margin, margin:-margin]
    return float(e.mean()), float(e.max())


def certainty_agreement(flow_b, flow_f, shift):
    """share of the pixels with exact-flow certainty 1 (both exact flows) that the computed flows also give 1"""
    h, w = flow_b.shape[:2]
    dx, dy = shift
    exact = T.certainty64(np.broadcast_to(np.float64([-dx, -dy]), (h, w, 2)),
                          np.broadcast_to(np.float64([dx, dy]), (h, w, 2))).astype(bool)
    got = T.certainty64(np.asarray(flow_b, dtype=np.float64), np.asarray(flow_f, dtype=np.float64)).astype(bool)
    return float((got & exact).sum() / exact.sum())


# the cases of the acceptance table: (h, w, shift); conditions on each
KNOWN_MOTION = [(48, 64, (3, 2)), (96, 128, (5, -3)), (192, 256, (7, -4))]
MAX_INTERIOR_MEAN_EPE = 0.1
MIN_AGREEMENT = 0.9
