"""Float64 numpy restatement of colour distribution transfer: the basis sequence, an axis's range,
the integer histograms with the pixels whose bin float32 cannot decide, the transfer table in exact integers, the
application of a table, the whole iterative transfer, and the sliced Wasserstein metric the orderings are stated in.
Nothing here touches the product's code; the tests compare the kernels and the operator surface with it."""
import bisect

import numpy as np

U24 = 2.0 ** -24


def bases64(iters):
    """R_0 = I; R_t, t >= 1: the Q factor of the 3 x 3 normal draw of seed 1000 + t, signs such that diag(R) of the
    factorisation is positive; each rounded to float32 once (returned as float32, (iters, 3, 3), columns = axes)"""
    out = [np.eye(3)]
    for t in range(1, iters):
        q, r = np.linalg.qr(np.random.default_rng(1000 + t).standard_normal((3, 3)))
        out.append(q * np.sign(np.diag(r)))
    return np.stack(out).astype(np.float32)


def axis_range(R):
    """(lo, hi) float64 (3,) of the axes of a float32 basis: twice the unit cube's projection around its middle"""
    R = np.asarray(R, dtype=np.float32).astype(np.float64)
    lo0, hi0 = np.minimum(R, 0).sum(0), np.maximum(R, 0).sum(0)
    mid, width = (lo0 + hi0) / 2, hi0 - lo0
    return mid - width, mid + width


def axis_constants(R, bins):
    """(lo, hi, scale) as the kernels use them: float32 values, held in float64"""
    lo, hi = axis_range(R)
    f32 = lambda v: np.asarray(v, dtype=np.float64).astype(np.float32).astype(np.float64)
    return f32(lo), f32(hi), f32(bins / (hi - lo))


def counted(mask, n):
    return np.ones(n, dtype=bool) if mask is None else np.asarray(mask).reshape(-1) != 0


def project64(img, R, bins):
    """(ub, pos) float64 (n, 3): the clamped projections and bin positions of every pixel, exact up to float64 rounding
    (the pixels as they are given: float32 values exactly, float64 values without a rounding to float32)"""
    x = np.asarray(img, dtype=np.float64).reshape(-1, 3)
    lo, hi, scale = axis_constants(R, bins)
    ub = np.clip(x @ np.asarray(R, dtype=np.float32).astype(np.float64), lo, hi)
    return ub, (ub - lo) * scale


def hist64(img, R, bins, mask=None):
    """(3, bins) int64: the histogram at the float64 positions"""
    _, pos = project64(img, R, bins)
    on = counted(mask, pos.shape[0])
    j = np.minimum(pos.astype(np.int64), bins - 1)
    return np.stack([np.bincount(j[on, k], minlength=bins) for k in range(3)])


def hist_bounds(img, R, bins, mask=None):
    """(lower, upper, share): per bin the count of the pixels whose float64 position lies at least delta = bins 2^-20 from
    an integer (float32 puts them in the same bin: its position is within delta of this one), that count plus the flagged
    pixels of the two bins around their integer, and the share of flagged among the counted (pixel, axis) pairs"""
    _, pos = project64(img, R, bins)
    on = counted(mask, pos.shape[0])
    delta = bins * 2.0 ** -20
    lower, upper = np.zeros((3, bins), dtype=np.int64), np.zeros((3, bins), dtype=np.int64)
    flagged = 0
    for k in range(3):
        p = pos[on, k]
        near = np.abs(p - np.round(p)) < delta
        sure = np.bincount(np.minimum(p[~near].astype(np.int64), bins - 1), minlength=bins)
        edge = np.round(p[near]).astype(np.int64)
        below, above = np.clip(edge - 1, 0, bins - 1), np.clip(edge, 0, bins - 1)
        either = np.bincount(below, minlength=bins) + np.bincount(above[above != below], minlength=bins)
        lower[k], upper[k] = sure, sure + either
        flagged += int(near.sum())
    return lower, upper, flagged / max(1, 3 * int(on.sum()))


def identity_table(R, bins):
    lo, hi = axis_range(R)
    return lo[:, None] + np.arange(bins + 1)[None, :] * ((hi - lo) / bins)[:, None]


def table64(hist_src, hist_dst, R, bins):
    """(3, bins + 1) float64 from two (3, bins) integer histograms, in exact integers up to the one division"""
    lo, hi = axis_range(R)
    out = identity_table(R, bins)
    for k in range(3):
        hs, hc = [int(v) for v in hist_src[k]], [int(v) for v in hist_dst[k]]
        Ns, Nc = sum(hs), sum(hc)
        if Ns == 0 or Nc == 0:
            continue
        S, Cc = [0], [0]                                            # Python integers: exact at any size
        for j in range(bins):
            S.append(S[-1] + hs[j])
            Cc.append(Cc[-1] + hc[j])
        filled = [i for i in range(bins) if hc[i] > 0]
        reach = [Cc[i + 1] * Ns for i in filled]               # ascending
        width = (hi[k] - lo[k]) / bins
        for j in range(bins + 1):
            a = S[j] * Nc
            i = filled[bisect.bisect_left(reach, a)] if a else filled[0]
            frac = float(a - Cc[i] * Ns) / float(hc[i] * Ns)
            out[k, j] = lo[k] + (i + frac) * width
    return out


def slopes(table, R, bins):
    """L_k: the steepest slope of each axis's table, in axis units per axis unit"""
    _, _, scale = axis_constants(R, bins)
    return np.diff(np.asarray(table, dtype=np.float64), axis=1).max(1) * scale


def apply64(img, R, table, bins, mask=None):
    """(out, d): the moved image and the (n, 3) axis displacements in float64, with the kernels' float32 lo, hi, scale and
    the table as given"""
    x = np.asarray(img, dtype=np.float64)
    R64 = np.asarray(R, dtype=np.float32).astype(np.float64)
    T = np.asarray(table, dtype=np.float64)
    ub, pos = project64(x, R, bins)
    j = np.minimum(pos.astype(np.int64), bins - 1)
    f = pos - j
    d = np.stack([T[k, j[:, k]] + f[:, k] * (T[k, j[:, k] + 1] - T[k, j[:, k]]) - ub[:, k] for k in range(3)], axis=1)
    on = counted(mask, d.shape[0])
    d = np.where(on[:, None], d, 0.0)
    return x + (d @ R64.T).reshape(x.shape), d


def apply_bound(img, R, table, bins, d):
    """The per-element bound of strotss_color_transfer_apply against apply64, eps = 2^-24, by counting its roundings.
    Per axis k, with U = sum_i |R_ik| |x_i|, W = hi - lo, M = max(|lo|, |hi|), L = the table's steepest slope:
      u_k: three roundings, <= 3 eps U;  ub - lo and its product with scale: <= 2 eps W in axis units;
      so the position moves by <= 3 eps U + 2 eps W, the interpolant by <= L times that (it is continuous and piecewise
      linear: a bin flip changes nothing else);  T[j+1] - T[j]: eps L W / bins;  the fused multiply-add: eps M;
      the subtraction of ub: eps W, and ub's own error 3 eps U.
      |error of d_k| <= eps ((1 + L) 3 U + L W (2 + 1 / bins) + M + W) <= D_k = eps (1 + L) (3 U + 3 W + M).
    Per output channel i: sum_k |R_ik| D_k and three roundings of the chain x_i + sum_k R_ik d_k, each <= eps (|x_i| +
    sum_k |R_ik| |d_k|)."""
    x = np.abs(np.asarray(img, dtype=np.float64)).reshape(-1, 3)
    Ra = np.abs(np.asarray(R, dtype=np.float32).astype(np.float64))
    lo, hi, _ = axis_constants(R, bins)
    L = slopes(table, R, bins)
    D = U24 * (1 + L) * (3 * (x @ Ra) + 3 * (hi - lo) + np.maximum(np.abs(lo), np.abs(hi)))
    return (D @ Ra.T + 3 * U24 * (x + np.abs(d) @ Ra.T)).reshape(np.asarray(img).shape)


def transfer64(style, content, style_mask=None, content_mask=None, iters=10, bins=1024):
    """the whole iterative transfer in float64 (the pixels stay float64 between the iterations)"""
    x = np.asarray(style, dtype=np.float64).copy()
    for R in bases64(iters):
        table = table64(hist64(x, R, bins, style_mask), hist64(content, R, bins, content_mask), R, bins)
        x, _ = apply64(x, R, table, bins, style_mask)
    return x


def swd(a, b, mask_a=None, mask_b=None, directions=64):
    """The sliced Wasserstein distance between the colours of two images (their counted pixels): the root mean square, over
    64 fixed unit directions and the 199 quantiles 0.005 .. 0.995, of the difference of the projections' quantiles"""
    D = np.random.default_rng(7).standard_normal((3, directions))
    D /= np.linalg.norm(D, axis=0)
    q = np.linspace(0.005, 0.995, 199)
    pa = np.asarray(a, dtype=np.float64).reshape(-1, 3)[counted(mask_a, np.asarray(a).size // 3)] @ D
    pb = np.asarray(b, dtype=np.float64).reshape(-1, 3)[counted(mask_b, np.asarray(b).size // 3)] @ D
    return float(np.mean((np.quantile(pa, q, axis=0) - np.quantile(pb, q, axis=0)) ** 2)) ** 0.5


def affine_match64(style, content):
    """the affine map of section 15 in float64 (eps = (1/255)^2): what `match` gives"""
    x, y = np.asarray(style, dtype=np.float64).reshape(-1, 3), np.asarray(content, dtype=np.float64).reshape(-1, 3)
    e = (1 / 255.0) ** 2 * np.eye(3)

    def power(M, p):
        lam, vec = np.linalg.eigh(M)
        return (vec * lam ** p) @ vec.T
    A = power(np.cov(y.T, bias=True) + e, 0.5) @ power(np.cov(x.T, bias=True) + e, -0.5)
    return ((x - x.mean(0)) @ A.T + y.mean(0)).reshape(np.asarray(style).shape)
