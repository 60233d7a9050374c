"""Float64 numpy restatement of the photorealism term: the matting Laplacian of Levin et al. (2008)
with windows clipped to the image, as the regulariser of Luan et al. (2017).  Two independent statements -- (a) the dense
L assembled window by window, (b) N (p - q) with q the guided filter of tests/_smooth_ref.py -- a float32 run of (b) in the
kernels' order of operations, and ERR32, that run's worst errors per family, pinned.  Nothing here touches the product's
code."""
import numpy as np

from _smooth_ref import PAIRS, counts, eps32, guided_direct

U24 = 2.0 ** -24
MAX_RADIUS = 4
DENSE_MAX_PIXELS = 400


def window(y, x, h, w, r, shift=0):
    """the clipped window around (y, x) as two slices (shift: a planted error, the box moved by `shift` pixels)"""
    return (slice(max(y - r + shift, 0), min(y + r + shift, h - 1) + 1),
            slice(max(x - r + shift, 0), min(x + r + shift, w - 1) + 1))


def stats64(I, r, eps):
    """mu (h, w, 3) and the six distinct entries of Sigma^{-1} (h, w, 6; 00 01 02 11 12 22), Sigma = cov_w(I) + eps Id with
    eps at its float32 value: what strotss_matting_prepare stores, before the rounding to float32"""
    I = np.asarray(I, dtype=np.float64)
    h, w = I.shape[:2]
    mu, sinv = np.empty((h, w, 3)), np.empty((h, w, 6))
    for y in range(h):
        for x in range(w):
            win = I[window(y, x, h, w, r)].reshape(-1, 3)
            m = win.mean(0)
            d = win - m
            inv = np.linalg.inv(d.T @ d / len(win) + eps32(eps) * np.eye(3))
            mu[y, x] = m
            sinv[y, x] = [inv[i, j] for i, j in PAIRS]
    return mu, sinv


def dense_laplacian(I, r, eps):
    """statement (a): L (hw, hw), the sum over the windows k of delta_ij - (1/N_k)(1 + (I_i - mu_k)^T Sigma_k^{-1} (I_j - mu_k))"""
    I = np.asarray(I, dtype=np.float64)
    h, w = I.shape[:2]
    assert h * w <= DENSE_MAX_PIXELS
    idx = np.arange(h * w).reshape(h, w)
    L = np.zeros((h * w, h * w))
    for y in range(h):
        for x in range(w):
            sl = window(y, x, h, w, r)
            ids = idx[sl].ravel()
            win = I[sl].reshape(-1, 3)
            n = len(ids)
            d = win - win.mean(0)
            sigma = d.T @ d / n + eps32(eps) * np.eye(3)
            L[np.ix_(ids, ids)] += np.eye(n) - (1.0 + d @ np.linalg.solve(sigma, d.T)) / n
    return L


def value_grad_dense(p, I, r, eps):
    """(L_photo, dL_photo/dp) from statement (a)"""
    p = np.asarray(p, dtype=np.float64)
    h, w = p.shape[:2]
    Lp = (dense_laplacian(I, r, eps) @ p.reshape(h * w, 3)).reshape(h, w, 3)
    return float((p * Lp).sum() / (3.0 * h * w)), 2.0 * Lp / (3.0 * h * w)


def value_grad(p, I, r, eps, q=None):
    """(L_photo, dL_photo/dp) from statement (b): L p = N (p - q)"""
    p = np.asarray(p, dtype=np.float64)
    h, w = p.shape[:2]
    q = guided_direct(p, I, r, eps) if q is None else q
    n = counts(h, w, r)[..., None]
    return float((n * p * (p - q)).sum() / (3.0 * h * w)), 2.0 * n * (p - q) / (3.0 * h * w)


def loss_scale(p, I, r, eps, q=None):
    """(1 / (3 h w)) sum N |p| |p - q|: what the scalar's error is measured against"""
    p = np.asarray(p, dtype=np.float64)
    h, w = p.shape[:2]
    q = guided_direct(p, I, r, eps) if q is None else q
    return float((counts(h, w, r)[..., None] * np.abs(p) * np.abs(p - q)).sum() / (3.0 * h * w))


def value_grad_planted(p, I, r, eps, bug):
    """statement (b) written out with one planted error: "unclipped_n" (N_i = (2r+1)^2 at the borders), "eps_times_n" (eps
    multiplied by N_k), "no_factor_2", "one_stage" (a, b not averaged), "shifted_window" (every window moved by one);
    bug None is the statement itself"""
    p, I = np.asarray(p, dtype=np.float64), np.asarray(I, dtype=np.float64)
    h, w = p.shape[:2]
    shift = 1 if bug == "shifted_window" else 0
    a, b = np.empty((h, w, 3, 3)), np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            sl = window(y, x, h, w, r, shift)
            wi, wp = I[sl].reshape(-1, 3), p[sl].reshape(-1, 3)
            n = len(wi)
            mu, pbar = wi.mean(0), wp.mean(0)
            e = eps32(eps) * (n if bug == "eps_times_n" else 1)
            sigma = (wi - mu).T @ (wi - mu) / n + e * np.eye(3)
            a[y, x] = np.linalg.solve(sigma, (wi - mu).T @ (wp - pbar) / n).T         # [c, j]
            b[y, x] = pbar - a[y, x] @ mu
    q = np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            if bug == "one_stage":
                q[y, x] = a[y, x] @ I[y, x] + b[y, x]
            else:
                sl = window(y, x, h, w, r, shift)
                q[y, x] = a[sl].reshape(-1, 3, 3).mean(0) @ I[y, x] + b[sl].reshape(-1, 3).mean(0)
    n = np.full((h, w, 1), float((2 * r + 1) ** 2)) if bug == "unclipped_n" else counts(h, w, r)[..., None]
    two = 1.0 if bug == "no_factor_2" else 2.0
    return float((n * p * (p - q)).sum() / (3.0 * h * w)), two * n * (p - q) / (3.0 * h * w)


def _shifted(x, dy, dx, r):
    """x (h, w, ...) read at (y + dy, x + dx), zeros outside"""
    h, w = x.shape[:2]
    pad = np.zeros((h + 2 * r, w + 2 * r) + x.shape[2:], dtype=x.dtype)
    pad[r:r + h, r:r + w] = x
    return pad[r + dy:r + dy + h, r + dx:r + dx + w]


def matting_float32(p, I, r, eps):
    """(L_photo, dL_photo/dp) in float32, the order of operations of csrc/matting.hip: the stored statistics (float64,
    rounded once), every window summed once with the data shifted by (mu_k, p_k), rows top to bottom and left to right, the
    shift taken out, a = Sigma^{-1} cov and b = pbar - a . mu, their row sums left to right and column sums top to bottom,
    q = abar . I + bbar.  No fused multiply-adds (numpy has none).  The scalar: float32 terms, numpy's pairwise float32 sum
    (the kernel's tree has another shape and the same depth)."""
    f = np.float32
    p, I = np.asarray(p, dtype=f), np.asarray(I, dtype=f)
    h, w = p.shape[:2]
    mu64, sinv64 = stats64(I, r, eps)
    mu, sinv = mu64.astype(f), sinv64.astype(f)
    yy, xx = np.mgrid[0:h, 0:w]
    sI, sp, C = np.zeros((h, w, 3), f), np.zeros((h, w, 3), f), np.zeros((h, w, 3, 3), f)       # C[j, c]
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ok = ((yy + dy >= 0) & (yy + dy < h) & (xx + dx >= 0) & (xx + dx < w))
            d = _shifted(I, dy, dx, r) - mu
            e = _shifted(p, dy, dx, r) - p
            sI = np.where(ok[..., None], sI + d, sI)
            sp = np.where(ok[..., None], sp + e, sp)
            C = np.where(ok[..., None, None], C + d[..., :, None] * e[..., None, :], C)
    n = counts(h, w, r).astype(f)[..., None]
    mp = sp / n
    v = (C - sI[..., :, None] * mp[..., None, :]) / n[..., None]                                 # v[j, c]
    S = np.empty((h, w, 3, 3), f)
    for k, (i, j) in enumerate(PAIRS):
        S[..., i, j] = S[..., j, i] = sinv[..., k]
    a = np.empty((h, w, 3, 3), f)                                                                # a[c, j]
    for c in range(3):
        for j in range(3):
            a[..., c, j] = (S[..., j, 0] * v[..., 0, c] + S[..., j, 1] * v[..., 1, c]) + S[..., j, 2] * v[..., 2, c]
    b = (p + mp) - ((a[..., 0] * mu[..., 0, None] + a[..., 1] * mu[..., 1, None]) + a[..., 2] * mu[..., 2, None])
    ab = np.concatenate([a.reshape(h, w, 9), b], -1)
    rows = _shifted(ab, 0, -r, r)
    for dx in range(-r + 1, r + 1):
        rows = rows + _shifted(ab, 0, dx, r)
    cols = _shifted(rows, -r, 0, r)
    for dy in range(-r + 1, r + 1):
        cols = cols + _shifted(rows, dy, 0, r)
    m = cols / n
    abar, bbar = m[..., :9].reshape(h, w, 3, 3), m[..., 9:]
    q = ((abar[..., 0] * I[..., 0, None] + abar[..., 1] * I[..., 1, None]) + abar[..., 2] * I[..., 2, None]) + bbar
    d = p - q
    inv_n = f(1.0 / (3.0 * h * w))
    loss = f(np.sum((n * p) * d, dtype=f)) * inv_n
    coef = f(2.0 / (3.0 * h * w))
    return float(loss), coef * (n * d)


# The float32 run's worst errors over tests/_matting_cases.py (CASES), per eps: (gradient, relative to max |gradient|;
# scalar, relative to loss_scale).  Pinned: test_matting_cpu.py holds the run to them, the GPU tests hold the kernels to 8 x.
ERR32 = {
    1e-4: (2.2e-5, 1.4e-5),          # measured 2.11e-05 and 1.32e-05, both at 1 x 3, r = 2: Sigma^{-1} reaches 1 / eps
    1e-2: (7.8e-7, 1.6e-7),          # measured 7.35e-07 (48 x 64, r = 1) and 1.51e-07 (1 x 3, r = 2)
    1.0: (1.1e-6, 2.7e-7),           # measured 1.02e-06 (9 x 12 affine, r = 2) and 2.56e-07 (1 x 3, r = 1)
}
