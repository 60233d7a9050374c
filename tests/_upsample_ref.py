"""Float64 numpy restatement of guided upsampling, on top of tests/_smooth_ref.py: the guided filter's
window means abar, bbar of (p, I_lo) at the result's size (h, w), interpolated to (H, W) with the taps of the project's
bilinear resize and applied to the full-resolution guide I_hi; "residual" adds the interpolated d = p - q_lo.  Two
independent statements (pixel loops with explicit taps and weights; vectorised gathers with the kernel's lerp order), a
float32 variant of the second, the analytic bound for an image affine in the guide, and the per-element budgets E_round and
E_stat of the GPU tests.  Nothing here touches the product's code."""
import numpy as np

import _smooth_ref as S

MODES = ("guided", "residual")
U24, U53 = S.U24, S.U53

# float32 roundings between the float64 window sums and the stored pixel, in units of u = 2^-24 times the magnitude each is
# relative to ("Tolerances"):
#   1  the storage of a and b                                   |  relative to the means of |a|, |b|, as in section 16
#   1  the rounding of their window means                       |
#   3  the lerp along x: fl(b - a) t is off by u t |b - a| <= 2 u max(|a|, |b|), the fused multiply-add rounds once more
#   3  the lerp along y, the same                               |  relative to the LARGEST of the four taps
#   3  the three fused multiply-adds of the pixel               |  relative to sum_j |A_cj| |I_j| + |B_c|
ROUNDINGS_GUIDED = 11
#   1  more for the residual's add, relative to |guided| + |up(d)|; up(d) itself: the subtraction p - q (1) and two lerps (6)
ROUNDINGS_RESIDUAL_ADD = 1
ROUNDINGS_D = 7


# ------------------------------------------------------------------ the resize
def taps(out_size, in_size):
    """(lo, hi, t) per output index: the taps of strotss_resize_bilinear, the source coordinate in float32 as the kernel
    computes it ((i + 0.5) * scale - 0.5, every operation rounded), half-pixel centres, clamped indices"""
    scale = np.float32(in_size) / np.float32(out_size)
    i = np.arange(out_size, dtype=np.float32)
    src = (i + np.float32(0.5)) * scale - np.float32(0.5)
    assert src.dtype == np.float32
    fl = np.floor(src)
    lo = np.maximum(fl.astype(np.int64), 0)
    hi = np.minimum(np.ceil(src).astype(np.int64), in_size - 1)
    return lo, hi, (src - fl).astype(np.float64)


def up(x, H, W, dtype=np.float64, rows=None):
    """x (h, w, ...) -> (H, W, ...): along x in both rows first, then along y, each lerp a + (b - a) t (t == 0 returns a).
    rows (an index array): only those output rows, for images too large to restate whole."""
    x = np.asarray(x, dtype=dtype)
    ylo, yhi, ty = (v if rows is None else v[rows] for v in taps(H, x.shape[0]))
    xlo, xhi, tx = taps(W, x.shape[1])
    tail = (1,) * (x.ndim - 2)
    tx, ty = tx.astype(dtype).reshape((1, W) + tail), ty.astype(dtype).reshape((len(ty), 1) + tail)
    top, bot = x[ylo], x[yhi]
    top = top[:, xlo] + (top[:, xhi] - top[:, xlo]) * tx
    bot = bot[:, xlo] + (bot[:, xhi] - bot[:, xlo]) * tx
    return top + (bot - top) * ty


def up_max(x, H, W, rows=None):
    """the largest |x| among the four taps of every output pixel"""
    x = np.abs(np.asarray(x, dtype=np.float64))
    ylo, yhi, _ = (v if rows is None else v[rows] for v in taps(H, x.shape[0]))
    xlo, xhi, _ = taps(W, x.shape[1])
    return np.maximum(np.maximum(x[ylo][:, xlo], x[ylo][:, xhi]), np.maximum(x[yhi][:, xlo], x[yhi][:, xhi]))


def down2(I_hi):
    """half-pixel bilinear downsample by exactly 2 without antialias: the mean of each 2 x 2 block"""
    I_hi = np.asarray(I_hi, dtype=np.float64)
    return 0.25 * (I_hi[0::2, 0::2] + I_hi[0::2, 1::2] + I_hi[1::2, 0::2] + I_hi[1::2, 1::2])


# ------------------------------------------------------------------ the two statements
def coefficients(p, I_lo, r, eps, dtype=np.float64):
    """the low-resolution stage: section 16's stages 1 and 2 on (p, I_lo).  dict of _smooth_ref's quantities plus
    abar (h, w, 3[c], 3[j]), bbar (h, w, 3), d = p - q."""
    p, I_lo = np.asarray(p, dtype=dtype), np.asarray(I_lo, dtype=dtype)
    ref = S.guided_separable(p, I_lo, r, eps, dtype=dtype, full=True)
    n = S.counts(p.shape[0], p.shape[1], r).astype(dtype)
    ref["abar"] = S.box_sum(ref["a"], r) / n[..., None, None]
    ref["bbar"] = S.box_sum(ref["b"], r) / n[..., None]
    ref["d"] = p - ref["q"]
    return ref


def upsample(p, I_lo, I_hi, r, eps, mode, dtype=np.float64, ref=None, rows=None):
    """statement 2 (vectorised): out = up(abar) I_hi + up(bbar) [+ up(d)], everything in `dtype`; rows: as in up()"""
    assert mode in MODES
    H, W = I_hi.shape[:2]
    I_hi = np.asarray(I_hi if rows is None else I_hi[rows], dtype=dtype)
    ref = ref or coefficients(p, I_lo, r, eps, dtype)
    out = (up(ref["abar"], H, W, dtype, rows) * I_hi[..., None, :]).sum(-1) + up(ref["bbar"], H, W, dtype, rows)
    return out + up(ref["d"], H, W, dtype, rows) if mode == "residual" else out


def upsample_float32(p, I_lo, I_hi, r, eps, mode):
    """float32 throughout: what kernels without float64 window sums would compute"""
    return upsample(p, I_lo, I_hi, r, eps, mode, dtype=np.float32)


def upsample_loops(p, I_lo, I_hi, r, eps, mode):
    """statement 1: loops over the pixels.  Window means taken directly over the clipped windows, cofactor solve, and per
    output pixel the four taps with their explicit weights (1 - ty)(1 - tx), (1 - ty) tx, ty (1 - tx), ty tx.  Small images."""
    assert mode in MODES
    p, I_lo, I_hi = (np.asarray(x, dtype=np.float64) for x in (p, I_lo, I_hi))
    h, w = p.shape[:2]
    H, W = I_hi.shape[:2]
    t = S.terms(p, I_lo)
    win = lambda y, x: (slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1))
    a, b = np.empty((h, w, 3, 3)), np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            mu, sigma, pbar, cov = S.moments(t[win(y, x)].reshape(-1, 21).mean(0), S.eps32(eps))
            a[y, x] = S.solve_cofactors(sigma, cov)
            b[y, x] = pbar - a[y, x] @ mu
    abar, bbar, d = np.empty((h, w, 3, 3)), np.empty((h, w, 3)), np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            abar[y, x] = a[win(y, x)].reshape(-1, 3, 3).mean(0)
            bbar[y, x] = b[win(y, x)].reshape(-1, 3).mean(0)
            d[y, x] = p[y, x] - (abar[y, x] @ I_lo[y, x] + bbar[y, x])
    ylo, yhi, ty = taps(H, h)
    xlo, xhi, tx = taps(W, w)
    out = np.empty((H, W, 3))
    for Y in range(H):
        for X in range(W):
            wts = (((1 - ty[Y]) * (1 - tx[X]), ylo[Y], xlo[X]), ((1 - ty[Y]) * tx[X], ylo[Y], xhi[X]),
                   (ty[Y] * (1 - tx[X]), yhi[Y], xlo[X]), (ty[Y] * tx[X], yhi[Y], xhi[X]))
            A = sum(wt * abar[y, x] for wt, y, x in wts)
            out[Y, X] = A @ I_hi[Y, X] + sum(wt * bbar[y, x] for wt, y, x in wts)
            if mode == "residual":
                out[Y, X] += sum(wt * d[y, x] for wt, y, x in wts)
    return out


# ------------------------------------------------------------------ the analytic bound
def affine_bound(I_lo, I_hi, M, r, eps, mode):
    """For p = M I_lo + t the window's coefficients are a_c = (Id - eps Sigma_k^{-1}) M_c and b_c = M_c mu_k + t_c - a_c mu_k,
    so a_c v + b_c - (M_c v + t_c) = -eps (Sigma_k^{-1} M_c) (v - mu_k) for every colour v.  With v = I_hi(i), through the box
    mean over the windows k of each tap and the bilinear weights of the taps:
      |out_c(i) - (M I_hi(i) + t)_c| <= up_k(eps |Sigma_k^{-1}|_2 |M_c|_2 |I_hi(i) - mu_k|_2);
    residual adds up() of |d| <= the same at the low resolution (v = I_lo(j), section 16's shrinkage).  -> (H, W, 3)."""
    I_lo, I_hi = np.asarray(I_lo, dtype=np.float64), np.asarray(I_hi, dtype=np.float64)
    h, w = I_lo.shape[:2]
    H, W = I_hi.shape[:2]
    ref = S.guided_separable(I_lo, I_lo, r, eps, full=True)
    inv_norm = 1.0 / np.linalg.eigvalsh(ref["sigma"])[..., 0]              # |Sigma_k^{-1}|_2 = 1 / lambda_min, (h, w)
    n = S.counts(h, w, r)
    norm_m = np.sqrt((np.asarray(M, dtype=np.float64) ** 2).sum(-1))       # |M_c|_2
    ylo, yhi, ty = taps(H, h)
    xlo, xhi, tx = taps(W, w)
    e = S.eps32(eps)
    per_pixel = np.empty((H, W))
    for Y in range(H):
        for X in range(W):
            field = S.box_sum(inv_norm * np.sqrt(((I_hi[Y, X] - ref["mu"]) ** 2).sum(-1)), r) / n
            per_pixel[Y, X] = (1 - ty[Y]) * ((1 - tx[X]) * field[ylo[Y], xlo[X]] + tx[X] * field[ylo[Y], xhi[X]]) \
                + ty[Y] * ((1 - tx[X]) * field[yhi[Y], xlo[X]] + tx[X] * field[yhi[Y], xhi[X]])
    bound = e * per_pixel[..., None] * norm_m
    if mode == "residual":
        shrink = np.empty((h, w))
        for y in range(h):
            for x in range(w):
                win = (slice(max(y - r, 0), min(y + r, h - 1) + 1), slice(max(x - r, 0), min(x + r, w - 1) + 1))
                shrink[y, x] = (inv_norm[win] * np.sqrt(((I_lo[y, x] - ref["mu"][win]) ** 2).sum(-1))).mean()
        bound = bound + up(e * shrink[..., None] * norm_m, H, W)
    return bound


# ------------------------------------------------------------------ the budgets of the GPU tests
def error_budgets(p, I_lo, I_hi, r, eps, mode, ref=None, rows=None):
    """(E_round, E_stat), each (H, W, 3), from the reference's own quantities ("Tolerances").
    E_round: gamma_11 (sum_j upmax(mean|a_cj|) |I_hi_j| + upmax(mean|b_c|)); residual: gamma_12 of that, + gamma_8 upmax|d|,
    + upmax of section 16's gamma_5 budget of q_lo (which enters d).  upmax: the largest of the four taps.
    E_stat: section 16's float64 terms of abar and bbar, kept apart, interpolated with the bilinear weights (they propagate
    linearly) and applied to |I_hi|; residual adds up() of section 16's E_stat of q_lo.  Doubled, as there.  rows: as in up()."""
    assert mode in MODES
    H, W = I_hi.shape[:2]
    p, I_lo, I_hi = (np.asarray(x, dtype=np.float64) for x in (p, I_lo, I_hi if rows is None else I_hi[rows]))
    ref = ref or coefficients(p, I_lo, r, eps)
    h, w = p.shape[:2]
    eps = S.eps32(eps)
    up_max, up = (lambda x, H, W, f=f: f(x, H, W, rows=rows) for f in (globals()["up_max"], globals()["up"]))
    n = S.counts(h, w, r)
    mean = lambda x: S.box_sum(x, r) / n.reshape(n.shape + (1,) * (x.ndim - 2))
    a, b = np.abs(ref["a"]), np.abs(ref["b"])
    ma, mb, aI, aH = mean(a), mean(b), np.abs(I_lo), np.abs(I_hi)
    scale_hi = (up_max(ma, H, W) * aH[..., None, :]).sum(-1) + up_max(mb, H, W)
    # section 16's statistics terms, as _smooth_ref.error_budgets forms them
    g = ((S.extents(h, r)[:, None] + S.extents(w, r)[None, :] + 1) * U53)[..., None]
    same_sign = p.min() >= 0 and I_lo.min() >= 0
    am = np.abs(ref["means"]) if same_sign else mean(S.terms(np.abs(p), np.abs(I_lo)))
    mI, mp, mIp = am[..., 0:3], am[..., 9:12], am[..., 12:21].reshape(h, w, 3, 3)
    mII = np.empty((h, w, 3, 3))
    for k, (i, j) in enumerate(S.PAIRS):
        mII[..., i, j] = mII[..., j, i] = am[..., 3 + k]
    g3 = (g + 3 * U53)[..., None]
    d_mu, d_pbar = g * mI, g * mp
    d_sigma = g3 * (mII + 2 * mI[..., :, None] * mI[..., None, :] + eps) + 8 * U53 * np.abs(ref["sigma"])
    d_cov = g3 * (mIp + 2 * mp[..., :, None] * mI[..., None, :]) + 4 * U53 * np.abs(ref["cov"])
    norm_a = np.sqrt((a ** 2).sum(-1))
    d_a = (np.sqrt((d_cov ** 2).sum(-1)) + np.sqrt((d_sigma ** 2).sum((-1, -2)))[..., None] * norm_a) / eps
    d_b = d_pbar + (d_a[..., None] * mI[..., None, :] + a * d_mu[..., None, :]).sum(-1) \
        + 4 * U53 * (mp + (a * mI[..., None, :]).sum(-1))
    d_abar = mean(d_a)[..., None] + g[..., None] * ma                    # (h, w, 3[c], 3[j])
    d_bbar = mean(d_b) + g * mb                                           # (h, w, 3)
    e_stat = (up(d_abar, H, W) * aH[..., None, :]).sum(-1) + up(d_bbar, H, W)
    if mode == "guided":
        return S.gamma32(ROUNDINGS_GUIDED) * scale_hi, 2 * e_stat
    scale_lo = (ma * aI[..., None, :]).sum(-1) + mb
    e_round = S.gamma32(ROUNDINGS_GUIDED + ROUNDINGS_RESIDUAL_ADD) * scale_hi \
        + S.gamma32(ROUNDINGS_D + ROUNDINGS_RESIDUAL_ADD) * up_max(ref["d"], H, W) \
        + up_max(S.gamma32(S.ROUNDINGS) * scale_lo, H, W)
    e_stat_lo = (d_abar * aI[..., None, :]).sum(-1) + d_bbar
    return e_round, 2 * (e_stat + up(e_stat_lo, H, W))


# ------------------------------------------------------------------ inputs
def test_images(h, w, H, W, seed):
    """(p, I_lo, I_hi) float32: _smooth_ref's pair (p, I_lo) at (h, w), and its guide pattern drawn at (H, W) with the same
    seed (the same shading phases and colours, an edge along the same diagonal, noise of its own) as I_hi"""
    p, I_lo = S.test_images(h, w, seed)
    _, I_hi = S.test_images(H, W, seed)
    return p, I_lo, I_hi
