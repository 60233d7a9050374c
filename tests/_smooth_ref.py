"""Float64 numpy restatement of photo smoothing: the guided filter of He, Sun and Tang (2013) with a
colour guide, windows clipped to the image and divided by their own pixel count.  Two independent statements -- direct
loops over the clipped windows with a cofactor solve, and separable cumulative sums with an LDL^T solve -- a float32
variant of the second (what the kernels must beat), and the per-element error budgets E_round and E_stat of the GPU tests.
Nothing here touches the product's code."""
import numpy as np

U24, U53 = 2.0 ** -24, 2.0 ** -53
MAX_RADIUS = 64
PAIRS = ((0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2))


# float32 roundings between the float64 solve and the stored pixel: the storage of a and b, the rounding of their window
# means, and the three fused multiply-adds b + a_0 I_0 + a_1 I_1 + a_2 I_2 (the last one's result is the stored pixel)
ROUNDINGS = 5


def gamma32(k):
    """k float32 roundings in a row: (1 + u)^k - 1 <= k u / (1 - k u), u = 2^-24"""
    return k * U24 / (1.0 - k * U24)


def eps32(eps):
    """the regulariser as the C entry receives it: rounded to float32"""
    return float(np.float32(eps))


def extents(n, r):
    """the number of pixels of [x - r, x + r] clipped to [0, n), for every x"""
    x = np.arange(n)
    return np.minimum(x + r, n - 1) - np.maximum(x - r, 0) + 1


def counts(h, w, r):
    """N_k: the pixel count of every clipped window, (h, w)"""
    return np.outer(extents(h, r), extents(w, r)).astype(np.float64)


def _box_axis0(x, r):
    """sums over [i - r, i + r] clipped, along axis 0, by cumulative sums RESTARTED every L = 2r + 1 elements: a window is the
    tail of one block plus the head of the next, so its rounding error is that of at most L additions whatever the length
    of the axis (an axis-long prefix sum would carry n u |prefix| into every window)."""
    n, L = x.shape[0], 2 * r + 1
    nb = -(-n // L)
    pad = np.zeros((nb * L,) + x.shape[1:], dtype=x.dtype)
    pad[:n] = x
    blocks = pad.reshape((nb, L) + x.shape[1:])
    head = np.cumsum(blocks, axis=1, dtype=x.dtype).reshape(pad.shape)                        # block start .. i
    tail = np.cumsum(blocks[:, ::-1], axis=1, dtype=x.dtype)[:, ::-1].reshape(pad.shape)      # i .. block end
    i = np.arange(n)
    lo, hi = np.maximum(i - r, 0), np.minimum(i + r, n - 1)
    two = lo // L != hi // L
    # one block: a full window that starts its block, or one clipped at the end of the axis (zeros behind it)
    one = np.where((lo % L == 0).reshape((-1,) + (1,) * (x.ndim - 1)), head[hi], tail[lo])
    return np.where(two.reshape((-1,) + (1,) * (x.ndim - 1)), tail[lo] + head[hi], one)


def box_sum(x, r):
    """clipped (2r+1) x (2r+1) window sums of an (h, w, ...) array in its own dtype: columns, then rows"""
    return np.swapaxes(_box_axis0(np.swapaxes(_box_axis0(x, r), 0, 1), r), 0, 1)


def terms(p, I):
    """(h, w, 21): I (3), I_i I_j for i <= j (6), p (3), I_j p_c (9, c major), in the dtype of the inputs"""
    return np.concatenate([I, np.stack([I[..., i] * I[..., j] for i, j in PAIRS], -1), p,
                           (p[..., :, None] * I[..., None, :]).reshape(p.shape[:-1] + (9,))], -1)


def moments(m, eps):
    """from the 21 window means: mu (.., 3), Sigma = cov(I) + eps Id (.., 3, 3), pbar (.., 3), cov[c, j] (.., 3, 3)"""
    mu, pbar = m[..., 0:3], m[..., 9:12]
    second = np.empty(m.shape[:-1] + (3, 3), dtype=m.dtype)
    for k, (i, j) in enumerate(PAIRS):
        second[..., i, j] = second[..., j, i] = m[..., 3 + k]
    sigma = second - mu[..., :, None] * mu[..., None, :] + m.dtype.type(eps) * np.eye(3, dtype=m.dtype)
    cov = m[..., 12:21].reshape(m.shape[:-1] + (3, 3)) - pbar[..., :, None] * mu[..., None, :]
    return mu, sigma, pbar, cov


def solve_cofactors(sigma, cov):
    """a[c] = Sigma^{-1} cov[c] by the adjugate over the determinant (closed form, no library call)"""
    s = sigma
    adj = np.empty_like(s)
    adj[..., 0, 0] = s[..., 1, 1] * s[..., 2, 2] - s[..., 1, 2] * s[..., 1, 2]
    adj[..., 1, 1] = s[..., 0, 0] * s[..., 2, 2] - s[..., 0, 2] * s[..., 0, 2]
    adj[..., 2, 2] = s[..., 0, 0] * s[..., 1, 1] - s[..., 0, 1] * s[..., 0, 1]
    adj[..., 0, 1] = adj[..., 1, 0] = s[..., 0, 2] * s[..., 1, 2] - s[..., 0, 1] * s[..., 2, 2]
    adj[..., 0, 2] = adj[..., 2, 0] = s[..., 0, 1] * s[..., 1, 2] - s[..., 0, 2] * s[..., 1, 1]
    adj[..., 1, 2] = adj[..., 2, 1] = s[..., 0, 1] * s[..., 0, 2] - s[..., 0, 0] * s[..., 1, 2]
    det = s[..., 0, 0] * adj[..., 0, 0] + s[..., 0, 1] * adj[..., 0, 1] + s[..., 0, 2] * adj[..., 0, 2]
    return (cov[..., :, None, :] * adj[..., None, :, :]).sum(-1) / det[..., None, None]


def solve_ldl(sigma, cov):
    """the same by the LDL^T factors of the symmetric positive definite Sigma, written out (closed form as well)"""
    s00, s01, s02 = sigma[..., 0, 0, None], sigma[..., 0, 1, None], sigma[..., 0, 2, None]
    s11, s12, s22 = sigma[..., 1, 1, None], sigma[..., 1, 2, None], sigma[..., 2, 2, None]
    c0, c1, c2 = cov[..., 0], cov[..., 1], cov[..., 2]                   # (.., 3): one value per output channel
    l10, l20 = s01 / s00, s02 / s00
    d1 = s11 - l10 * s01
    t12 = s12 - l20 * s01
    l21 = t12 / d1
    d2 = s22 - l20 * s02 - l21 * t12
    z1 = c1 - l10 * c0
    z2 = c2 - l20 * c0 - l21 * z1
    a2 = z2 / d2
    a1 = z1 / d1 - l21 * a2
    a0 = c0 / s00 - l10 * a1 - l20 * a2
    return np.stack([a0, a1, a2], -1)


def guided_direct(p, I, r, eps):
    """statement 1: loops over the pixels, every mean taken directly over the clipped window, cofactor solve.  Small images."""
    p, I = np.asarray(p, dtype=np.float64), np.asarray(I, dtype=np.float64)
    h, w = p.shape[:2]
    t = terms(p, I)
    win = lambda y, x: (slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1))
    a, b = np.empty((h, w, 3, 3)), np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            mu, sigma, pbar, cov = moments(t[win(y, x)].reshape(-1, 21).mean(0), eps32(eps))
            a[y, x] = solve_cofactors(sigma, cov)
            b[y, x] = pbar - a[y, x] @ mu
    q = np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            q[y, x] = a[win(y, x)].reshape(-1, 3, 3).mean(0) @ I[y, x] + b[win(y, x)].reshape(-1, 3).mean(0)
    return q


def guided_separable(p, I, r, eps, dtype=np.float64, full=False):
    """statement 2: separable cumulative sums (box_sum) and the LDL^T solve, everything in `dtype`.  full=True: a dict with
    q, a (h, w, 3[c], 3[j]), b, the 21 window means, mu, Sigma, pbar, cov."""
    p, I = np.asarray(p, dtype=dtype), np.asarray(I, dtype=dtype)
    n = counts(p.shape[0], p.shape[1], r).astype(dtype)
    m = box_sum(terms(p, I), r) / n[..., None]
    mu, sigma, pbar, cov = moments(m, eps32(eps))
    a = solve_ldl(sigma, cov)
    b = pbar - (a * mu[..., None, :]).sum(-1)
    abar, bbar = box_sum(a, r) / n[..., None, None], box_sum(b, r) / n[..., None]
    q = (abar * I[..., None, :]).sum(-1) + bbar
    if not full:
        return q
    return dict(q=q, a=a, b=b, means=m, mu=mu, sigma=sigma, pbar=pbar, cov=cov)


def guided_float32(p, I, r, eps):
    """the same in float32 throughout: what a kernel without float64 window sums would compute"""
    return guided_separable(p, I, r, eps, dtype=np.float32)


def error_budgets(p, I, r, eps, ref=None):
    """(E_round, E_stat), each (h, w, 3), from the reference's own quantities ("Tolerances").
    E_round: the kernels' five float32 roundings (ROUNDINGS), gamma_5 = 5 u / (1 - 5 u) with u = 2^-24, relative to
    sum_j boxmean(|a_cj|) |I_j| + boxmean(|b_c|).
    E_stat: the float64 roundings of the window sums and of the solve, propagated to first order through
    |Sigma^{-1}| <= 1 / eps and doubled (the reference adds up the same windows in two passes of at most 2r + 1 terms)."""
    p, I = np.asarray(p, dtype=np.float64), np.asarray(I, dtype=np.float64)
    ref = ref or guided_separable(p, I, r, eps, full=True)
    h, w = p.shape[:2]
    eps = eps32(eps)
    n = counts(h, w, r)
    mean = lambda x: box_sum(x, r) / n.reshape(n.shape + (1,) * (x.ndim - 2))
    a, b = np.abs(ref["a"]), np.abs(ref["b"])
    ma, mb, aI = mean(a), mean(b), np.abs(I)
    scale = (ma * aI[..., None, :]).sum(-1) + mb
    e_round = gamma32(ROUNDINGS) * scale
    # a window sum: n_y fused multiply-adds down the column, n_x - 1 additions along the row, one division
    g = ((extents(h, r)[:, None] + extents(w, r)[None, :] + 1) * U53)[..., None]
    same_sign = p.min() >= 0 and I.min() >= 0
    am = np.abs(ref["means"]) if same_sign else mean(terms(np.abs(p), np.abs(I)))     # window means of the absolute terms
    mI, mp, mIp = am[..., 0:3], am[..., 9:12], am[..., 12:21].reshape(h, w, 3, 3)
    mII = np.empty((h, w, 3, 3))
    for k, (i, j) in enumerate(PAIRS):
        mII[..., i, j] = mII[..., j, i] = am[..., 3 + k]
    g3 = (g + 3 * U53)[..., None]                       # + forming the product of two means, the difference, + eps
    d_mu, d_pbar = g * mI, g * mp
    d_sigma = g3 * (mII + 2 * mI[..., :, None] * mI[..., None, :] + eps) + 8 * U53 * np.abs(ref["sigma"])   # 8 u: LDL^T
    d_cov = g3 * (mIp + 2 * mp[..., :, None] * mI[..., None, :]) + 4 * U53 * np.abs(ref["cov"])
    norm_a = np.sqrt((a ** 2).sum(-1))
    d_a = (np.sqrt((d_cov ** 2).sum(-1)) + np.sqrt((d_sigma ** 2).sum((-1, -2)))[..., None] * norm_a) / eps    # (h, w, 3[c])
    d_b = d_pbar + (d_a[..., None] * mI[..., None, :] + a * d_mu[..., None, :]).sum(-1) \
        + 4 * U53 * (mp + (a * mI[..., None, :]).sum(-1))
    e_stat = ((mean(d_a)[..., None] + g[..., None] * ma) * aI[..., None, :]).sum(-1) + mean(d_b) + g * mb
    return e_round, 2 * e_stat


def residual(img, guide, r, eps):
    """R(img) = mean |img - guided(img; guide)|: how far an image is from its own edge-aware smoothing by the guide"""
    img = np.asarray(img, dtype=np.float64)
    return float(np.abs(img - guided_separable(img, guide, r, eps)).mean())


def box_mean_twice(p, r):
    """p box-averaged twice over the clipped windows: the filter's output under a constant guide"""
    p = np.asarray(p, dtype=np.float64)
    n = counts(p.shape[0], p.shape[1], r)[..., None]
    return box_sum(box_sum(p, r) / n, r) / n


def test_images(h, w, seed):
    """(p, I) float32: a guide in [0, 1] with smooth shading, a step edge and noise; an image that follows the guide through
    a colour mix, with noise of its own and values a little outside [0, 1] (the optimiser's result is not clamped)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    shade = 0.45 + 0.25 * np.sin(xx / 7.0 + rng.uniform(0, 6)) * np.cos(yy / 5.0 + rng.uniform(0, 6))
    step = 0.2 * (xx + yy > (h + w) / 2)
    I = np.clip((shade + step)[..., None] * rng.uniform(0.6, 1.0, 3) + 0.15 * rng.random((h, w, 3)), 0.0, 1.0)
    M = 0.7 * np.eye(3) + 0.15 * rng.standard_normal((3, 3))
    p = I @ M.T + 0.05 + 0.3 * (rng.random((h, w, 3)) - 0.5)
    return p.astype(np.float32), I.astype(np.float32)
