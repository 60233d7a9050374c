"""Float64 restatement of the pixel-space priors (strotss_pool_mean, strotss_detail_fwd_bwd, strotss_tv_fwd_bwd,
StepEngine(detail=, tv_weight=)) in NumPy alone, with their analytic gradients, and the bounds
tests/test_hip_pixel_prior.py holds the library to.

Detail term, x and c (h, w, 3), per pool size p with hp = ceil(h / p), wp = ceil(w / p):
    P_p(u)(i, j)   the mean of the pixels cell (i, j) covers, cnt(i, j) of them (partial cells on the last row / column)
    (L u)(k)       deg(k) u(k) - sum of the 4-neighbours of k inside the hp x wp grid (the graph Laplacian: symmetric)
    D_p            L (P_p(x) - P_p(c)) per channel;   m_p >= 0 cell weights, 1 when absent
    L_p            (1 / (3 hp wp)) sum_k m_p(k) sum_ch D_p(k, ch)^2
    dL_p/dx(q, ch) (2 / (3 hp wp cnt(k))) (L (m_p D_p))(k, ch) for pixel q of cell k
Total variation, eps = TV_EPS:
    dx(r, s) = x(r, s+1) - x(r, s), 0 in the last column; dy likewise, 0 in the last row;  n = sqrt(dx^2 + dy^2 + eps^2)
    L_tv = (1 / (3 h w)) sum (n - eps);   dL_tv/dx(q) = (1 / (3 h w)) ((dx / n)(left of q) - (dx / n)(q) + (dy / n)(above q)
    - (dy / n)(q)), a neighbour outside the image contributing 0

Yardstick: the same functions with every array in float32, the operations in the order the kernels apply them (pooling sums
a cell's rows left to right, then the row sums; the neighbours as ((up + down) + left) + right; n - eps as
(dx^2 + dy^2) / (n + eps), which is the same number without the cancellation).  err32 = max|g32 - g64| / max|g64| per case, its worst value per family pinned in
ERR32, the per-element tolerance TOL_GRAD[family] = MARGIN * ERR32[family] of max|ref| (MARGIN = 8, the rule of DESIGN.md
section 25); losses to LOSS_TOL relative (section 12's figure for a reduction of this kind).  `plant` states one deliberate
error each, for tests/test_pixel_prior_cpu.py."""
import numpy as np

TV_EPS = 1.0 / 255.0
MARGIN = 8.0
LOSS_TOL = 1e-5
# worst err32 per family over _pixel_prior_cases.DETAIL / TV, as printed by tests/test_pixel_prior_cpu.py (which asserts that
# a run's worst lies between a quarter and twice the pinned value)
ERR32 = {
    "detail": 2.0e-7,        # 257x300-p1_2_8-absent
    "detail16": 1.0e-6,      # 17x16-p16-random.  A pool size of 16 among them: the means of 256 values in [0, 1] differ by
                             # 0.03, so there D rests on some cancellation after all
    "tv": 1.8e-7,            # 42x63
}
TOL_GRAD = {k: MARGIN * v for k, v in ERR32.items()}


def family(pools):
    return "detail16" if 16 in tuple(pools) else "detail"


PLANTS = ("no_cnt", "zero_pad", "weight_after", "no_factor2", "tv_wrap")


def grid(h, w, p):
    return -(-h // p), -(-w // p)


def counts(h, w, p):
    """cnt(i, j): the pixels cell (i, j) covers"""
    hp, wp = grid(h, w, p)
    rows = np.minimum(p, h - p * np.arange(hp))
    cols = np.minimum(p, w - p * np.arange(wp))
    return rows[:, None] * cols[None, :]


def pool(u, p, dtype=np.float64):
    """P_p(u), u (h, w, ch): every row of the cell summed left to right, the row sums added top to bottom, in `dtype`, then
    divided by the pixel count"""
    u = np.asarray(u, dtype=dtype)
    h, w, ch = u.shape
    hp, wp = grid(h, w, p)
    pad = np.zeros((hp * p, wp * p, ch), dtype=dtype)
    pad[:h, :w] = u
    acc = np.zeros((hp, wp, ch), dtype=dtype)
    for dr in range(p):
        racc = np.zeros((hp, wp, ch), dtype=dtype)
        for ds in range(p):
            racc = racc + pad[dr::p, ds::p]        # a pixel the cell does not cover adds an exact 0
        acc = acc + racc
    return (acc / counts(h, w, p).astype(dtype)[:, :, None]).astype(dtype)


def laplacian(u, zero_pad=False):
    """(L u) on the (hp, wp, ch) grid: deg(k) u(k) - (((up + down) + left) + right), neighbours outside the grid absent
    (zero_pad: the planted error, deg = 4 everywhere)"""
    hp, wp = u.shape[:2]
    z = np.zeros((hp + 2, wp + 2) + u.shape[2:], dtype=u.dtype)
    z[1:-1, 1:-1] = u
    i, j = np.arange(hp)[:, None], np.arange(wp)[None, :]
    deg = ((i > 0).astype(int) + (i < hp - 1) + (j > 0) + (j < wp - 1)).astype(u.dtype)
    if zero_pad:
        deg = np.full_like(deg, 4)
    return (deg[:, :, None] * u - (((z[:-2, 1:-1] + z[2:, 1:-1]) + z[1:-1, :-2]) + z[1:-1, 2:])).astype(u.dtype)


def detail(x, c, pools, weights=None, gscales=None, dtype=np.float64, plant=None, pooled_content=None):
    """([L_p], sum_p gscales[p] dL_p/dx): x, c (h, w, 3); weights[j] the (hp, wp) cell weights of pools[j] or None;
    gscales default 1.  The gradient is accumulated over the pool sizes in ascending order."""
    x = np.asarray(x, dtype=dtype)
    h, w, _ = x.shape
    weights = [None] * len(pools) if weights is None else weights
    gscales = [1.0] * len(pools) if gscales is None else gscales
    losses, grad = [], np.zeros_like(x)
    for j, p in enumerate(pools):
        hp, wp = grid(h, w, p)
        pc = pool(c, p, dtype) if pooled_content is None else np.asarray(pooled_content[j], dtype=dtype)
        d = (pool(x, p, dtype) - pc).astype(dtype)
        D = laplacian(d, zero_pad=plant == "zero_pad")
        m = None if weights[j] is None else np.asarray(weights[j], dtype=dtype)[:, :, None]
        E = D if m is None else (m * D).astype(dtype)
        n = 3.0 * hp * wp
        losses.append(dtype((E * D).sum(dtype=dtype)) * dtype(1.0 / n))
        if plant == "weight_after" and m is not None:
            G = (m * laplacian(D)).astype(dtype)
        else:
            G = laplacian(E, zero_pad=plant == "zero_pad")
        coef = dtype((1.0 if plant == "no_factor2" else 2.0) * float(gscales[j]) / n)
        cnt = np.full((hp, wp), p * p) if plant == "no_cnt" else counts(h, w, p)
        cell = (G * (coef / cnt.astype(dtype))[:, :, None]).astype(dtype)
        grad = (grad + np.repeat(np.repeat(cell, p, axis=0), p, axis=1)[:h, :w]).astype(dtype)
    return losses, grad


def tv(x, eps=TV_EPS, gscale=1.0, dtype=np.float64, plant=None):
    """(L_tv, gscale * dL_tv/dx): x (h, w, 3)"""
    x = np.asarray(x, dtype=dtype)
    h, w, _ = x.shape
    eps = dtype(eps)
    dx, dy = np.zeros_like(x), np.zeros_like(x)
    if plant == "tv_wrap":
        dx, dy = np.roll(x, -1, axis=1) - x, np.roll(x, -1, axis=0) - x
    else:
        dx[:, :-1] = x[:, 1:] - x[:, :-1]
        dy[:-1] = x[1:] - x[:-1]
    ss = (dx * dx + dy * dy).astype(dtype)
    n = np.sqrt(ss + eps * eps).astype(dtype)
    a, b = (dx / n).astype(dtype), (dy / n).astype(dtype)
    n3 = 3.0 * h * w
    if dtype == np.float64:
        loss = (n - eps).sum() / n3                     # the statement
    else:
        loss = dtype((ss / (n + eps)).sum(dtype=dtype)) * dtype(1.0 / n3)      # the kernel's form of it
    al, bu = np.zeros_like(a), np.zeros_like(b)
    if plant == "tv_wrap":
        al, bu = np.roll(a, 1, axis=1), np.roll(b, 1, axis=0)
    else:
        al[:, 1:] = a[:, :-1]
        bu[1:] = b[:-1]
    grad = (dtype(float(gscale) / n3) * ((al - a) + (bu - b))).astype(dtype)
    return loss, grad


def err32(g32, g64):
    scale = float(np.abs(g64).max())
    return float(np.abs(g32.astype(np.float64) - g64).max()) / scale if scale > 0 else float(np.abs(g32).max())
