"""numpy restatement of the robust optical flow, dtype-parametrised like _flow_ref.py (float64: the
statement; float32: the yardstick and the kernels' twin), shared by test_flow_robust_cpu.py and test_hip_flow_robust.py.

The pyramid, the upsampling, the warp and Ix, Iy, c of a warp are _flow_ref's (`inv` is not used); the matching stage is
_flow_match_ref's.  The energy has Charbonnier penalties on the linearised data term and on the flow's gradient, minimised
with lagged weights: per warp, `outer` times

  1. weights(): from the current (u, v), with clamped indices,
       r  = (Ix u + Iy v) + c                                   d = 1 / sqrt(r r + eps_d^2)
       ux = (u(x+1) - u(x-1)) / 2, uy, vx, vy likewise          s = 1 / sqrt(((ux ux + uy uy) + (vx vx + vy vy)) + eps_s^2)
       g_q = (s_p + s_q) w_q / 2 for the 8 neighbours q: (s_p + s_q) * (1/12) for N, S, W, E, * (1/24) for the diagonals
       G  = ((g_N + g_S) + (g_W + g_E)) + ((g_NW + g_NE) + (g_SW + g_SE))
       rG = 1 / G                                               k = d / (alpha G + d (Ix Ix + Iy Iy))
  2. sweeps(): iters / outer Jacobi sweeps with s, rG, k frozen; g_q is formed again from s as above, and
       ub = (((g_N u_N + g_S u_S) + (g_W u_W + g_E u_E)) + ((g_NW u_NW + g_NE u_NE) + (g_SW u_SW + g_SE u_SE))) rG
       vb likewise,  t = ((Ix ub + Iy vb) + c) k,  u <- ub - Ix t,  v <- vb - Iy t.

That is the evaluation order: every operation above is one rounding of `dtype`, the parentheses are the order, 1/12 and
1/24 are constants of `dtype`, 1 / x and sqrt are correctly rounded.  flow_robust.hip performs the same float32 operations
one by one, so the float32 run of this file is its twin."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
import _flow_match_ref as M  # noqa: E402

DEFAULTS = dict(alpha=0.06, eps_d=1e-3, eps_s=1e-2, outer=4)
MAX_OUTER = 8


def _neighbours(x):
    """(N, S, W, E, NW, NE, SW, SE) of a plane, indices clamped"""
    h, w = x.shape
    ym, yp, xm, xp = R._clamped(h, -1), R._clamped(h, 1), R._clamped(w, -1), R._clamped(w, 1)
    n, s = x[ym], x[yp]
    return n, s, x[:, xm], x[:, xp], n[:, xm], n[:, xp], s[:, xm], s[:, xp]


def _couplings(s):
    """g_q of the 8 neighbours, in _neighbours' order"""
    dt = s.dtype.type
    c12, c24 = dt(1) / dt(12), dt(1) / dt(24)
    q = _neighbours(s)
    return [(s + q[i]) * c12 for i in range(4)] + [(s + q[i]) * c24 for i in range(4, 8)]


def _tree(t):
    return ((t[0] + t[1]) + (t[2] + t[3])) + ((t[4] + t[5]) + (t[6] + t[7]))


def smoothness_weight(u, v, eps_s):
    dt = u.dtype.type
    h, w = u.shape
    ym, yp, xm, xp = R._clamped(h, -1), R._clamped(h, 1), R._clamped(w, -1), R._clamped(w, 1)
    half = dt(0.5)
    ux, uy = (u[:, xp] - u[:, xm]) * half, (u[yp] - u[ym]) * half
    vx, vy = (v[:, xp] - v[:, xm]) * half, (v[yp] - v[ym]) * half
    return dt(1) / np.sqrt(((ux * ux + uy * uy) + (vx * vx + vy * vy)) + dt(eps_s) * dt(eps_s))


def weights(u, v, ix, iy, c, alpha=0.06, eps_d=1e-3, eps_s=1e-2):
    """(s, rG, k) of one weight update"""
    dt = u.dtype.type
    r = (ix * u + iy * v) + c
    d = dt(1) / np.sqrt(r * r + dt(eps_d) * dt(eps_d))
    s = smoothness_weight(u, v, eps_s)
    g = _tree(_couplings(s))
    k = d / (dt(alpha) * g + d * (ix * ix + iy * iy))
    return s, dt(1) / g, k


def sweeps(u, v, ix, iy, c, s, rg, k, n):
    """n Jacobi sweeps with frozen weights"""
    g = _couplings(s)
    for _ in range(n):
        ub = _tree([gq * q for gq, q in zip(g, _neighbours(u))]) * rg
        vb = _tree([gq * q for gq, q in zip(g, _neighbours(v))]) * rg
        t = ((ix * ub + iy * vb) + c) * k
        u, v = ub - ix * t, vb - iy * t
    return u, v


def update(u, v, ix, iy, c, n, alpha=0.06, eps_d=1e-3, eps_s=1e-2):
    """one weight update and its n sweeps -> (u, v, s, rG, k)"""
    s, rg, k = weights(u, v, ix, iy, c, alpha, eps_d, eps_s)
    u, v = sweeps(u, v, ix, iy, c, s, rg, k, n)
    return u, v, s, rg, k


def check_params(alpha, eps_d, eps_s, outer, iters):
    for name, x in (("alpha", alpha), ("eps_d", eps_d), ("eps_s", eps_s)):
        if not (np.isfinite(x) and x > 0):
            raise ValueError(f"{name} = {x}: expected a finite value > 0")
    if not (1 <= outer <= MAX_OUTER and int(outer) == outer and iters % outer == 0):
        raise ValueError(f"outer = {outer}: expected 1..{MAX_OUTER} and a divisor of iters = {iters}")


def optical_flow(frame_a, frame_b, dtype=np.float64, match_radius=0, alpha=0.06, eps_d=1e-3, eps_s=1e-2, outer=4, warps=5,
                 iters=32, min_side=12, max_levels=8):
    """F (h, w, 2) of the robust form; match_radius > 0: section 31's stage at every level before the warps, unchanged"""
    check_params(alpha, eps_d, eps_s, outer, iters)
    pa = R.pyramid(frame_a, dtype, min_side, max_levels)
    pb = R.pyramid(frame_b, dtype, min_side, max_levels)
    u = v = np.zeros(pa[-1].shape, dtype=dtype)
    for lv in range(len(pa) - 1, -1, -1):
        a, b = pa[lv], pb[lv]
        if u.shape != a.shape:
            u, v = R.upsample(u, *a.shape), R.upsample(v, *a.shape)
        if match_radius:
            u, v, _ = M.stage(a, b, u, v, match_radius)
        for _ in range(warps):
            ix, iy, c, _ = R.coefficients(a, b, u, v, 1.0)
            for _ in range(outer):
                u, v = update(u, v, ix, iy, c, iters // outer, alpha, eps_d, eps_s)[:2]
    assert u.dtype == dtype and v.dtype == dtype
    return np.stack([u, v], axis=-1)
