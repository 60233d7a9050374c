"""Float64 restatement of every loss term the HIP loss entries compute, value and gradient w.r.t. the prediction rows,
written from the reference's definitions (nn/losses.py:12-80, run_strotss.py:27-40) independently of the kernels and of
oracle/numpy_ref.py (which tests/test_loss_cases_cpu.py uses as a cross-check).

Relaxed EMD (cosine, l2, 'both', the palette with and without the YUV conversion): tf.reduce_min splits the gradient of a
minimum equally among its ties; a tie is a duplicate group (tests/_loss_cases.py), never a float64 equality.  The cases are
conditioned so that no minimum is within TAU_C of another value, so the f32 kernels must select exactly these entries.

The L1 terms (self-similarity, its column-weighted form, moment matching) differentiate through sign(a - b), which f32
rounding may flip where |a - b| is tiny.  Their reference is FLIP-AWARE: an entry whose float64 |a - b| is below `tau`
(the f32 error of a and b, derived below from the stated error of the cost / covariance entries) is ambiguous; the
reference gradient gives it sign 0 and returns a per-element bound, the sum of the absolute contributions of the
ambiguous entries through the same linear chain (abs-propagated, so it covers every sign assignment of them).  The check
on a kernel's gradient is then  |got - ref| <= bound + tol * max|ref|  element by element (`check_grad`)."""
import numpy as np

RGB2YUV = np.array([[0.299, -0.14714119, 0.61497538],
                    [0.587, -0.28886916, -0.51496512],
                    [0.114, 0.43601035, -0.10001026]], dtype=np.float64)
U = 2.0 ** -24             # f32 unit roundoff
# Stated bound on |cost_f32 - cost_f64| of one cosine entry made by the bf16x3 / f32 cost GEMMs of the loss section (the
# prediction rows' self-distance matrix of the self-similarity term); tests/test_hip_loss_terms.py asserts it per case.
EPS_COST = 5e-6          # measured <= 3.4e-6 at d = 2179
# Minima of a conditioned case's float64 cost matrix are separated from the next distinct value by more than this.
TAU_C = 2.0 * EPS_COST
# Covariance / mean entries: |f32 - f64| <= COV_K * U * (sqrt(rows) + 2) * mean_k |c_ka c_kb|  (mean: ... * mean_k |y_ka|),
# the error of an f32 accumulation of `rows` terms of random sign in rounding; asserted per case on strotss_moment_stats.
COV_K = 2.0              # measured error <= 0.74 of this bound
# tests/test_hip_loss_terms.py: every scalar within TOL_SCALAR relative of float64, every gradient within
# TOL_GRAD of max|ref| (the L1 terms outside their flip bound)
TOL_SCALAR = 5e-5         # measured <= 6.7e-6
TOL_GRAD = 2e-5           # measured <= 1.3e-5 (REMD both at d = 2179), the rest <= 4.6e-6


def inv_norm(x):
    return 1.0 / np.sqrt(np.maximum((x * x).sum(1), 1e-12))


def cos_dist(x, y):
    return 1.0 - (x * inv_norm(x)[:, None]) @ (y * inv_norm(y)[:, None]).T


def unnormalise(y, r, g_hat, q):
    """dL/dy from dL/dyhat (yhat = y r): r (g - yhat q), q = yhat . g, zero where the row norm clamps"""
    live = (y * y).sum(1) >= 1e-12
    return r[:, None] * (g_hat - (y * r[:, None]) * (q * live)[:, None])


def check_grad(got, ref, bound, tol):
    """(passes, worst |got - ref| / max|ref| outside the bound, RMS of |got - ref| / max|ref|): the GPU-side comparison"""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    scale = max(np.abs(ref).max(), 1e-30)
    err = np.abs(got - ref)
    b = np.zeros_like(ref) if bound is None else bound
    excess = np.maximum(err - b, 0.0) / scale
    ok = bool(np.isfinite(got).all()) and bool((err <= b + tol * scale).all())
    return ok, float(excess.max()), float(np.sqrt((err * err).mean()) / scale)


# ------------------------------------------------------------------ self-similarity (losses.py:55-66)
def _selfsim_parts(y, c, eps_cost):
    n = y.shape[0]
    Dx, Dy = cos_dist(y, y), cos_dist(c, c)
    sxr, syr = Dx.sum(0), Dy.sum(0)
    sx, sy = np.maximum(sxr, 1e-12), np.maximum(syr, 1e-12)
    A, B = Dx / sx[None, :], Dy / sy[None, :]
    # an entry of error e in every D of a column moves A by <= e / s + A * n e / s; a clamped column holds exact zeros
    # (tests/_loss_cases.exact_rows), which carry no error; the f32 quotient adds U * A
    ea = np.where(sxr >= 1e-12, eps_cost * (1.0 + n * np.abs(A)) / sx[None, :], 0.0)
    eb = np.where(syr >= 1e-12, eps_cost * (1.0 + n * np.abs(B)) / sy[None, :], 0.0)
    tau = ea + eb + 2.0 * U * (np.abs(A) + np.abs(B))
    return Dx, sxr, sx, A, B, tau


def _selfsim_chain(y, Dx, sxr, sx, A, S, rounding=False):
    """dL/dy for dL/dA = S: S -> t -> Gd -> M -> (q, g_hat) -> unnormalise.  rounding: also the f32 error of the last two
    steps, 4 U (sqrt(n) + 2) r (|M| |yhat| + |yhat| |M| |1 - D|): the radial parts g_hat and yhat q cancel, and they are
    large where many prediction rows are identical (every entry between them has the same sign)"""
    ry = inv_norm(y)
    t = (S * A).sum(0) * (sxr >= 1e-12)
    Gd = (S - t[None, :]) / sx[None, :]
    M = -(Gd + Gd.T)
    q = (M * (1.0 - Dx)).sum(1)
    g = unnormalise(y, ry, M @ (y * ry[:, None]), q)
    if not rounding:
        return g
    yh, Ma = np.abs(y * ry[:, None]), np.abs(M)
    return g, 4.0 * U * (np.sqrt(y.shape[0]) + 2.0) * ry[:, None] * (Ma @ yh + yh * (Ma * np.abs(1.0 - Dx)).sum(1)[:, None])


def _selfsim_chain_abs(y, Dx, sxr, sx, A, Sa):
    """the same chain on absolute values: an elementwise bound of |chain(S)| for every S with |S| <= Sa.  A diagonal entry
    D_jj = 1 - yhat_j.yhat_j is constant, so its sign reaches the gradient only through t_j (times A_jj) and through the
    rounding residue of the radial projection: M_jj yhat_j (1 - (1 - D_jj)) = M_jj yhat_j D_jj."""
    ry = inv_norm(y)
    yh = np.abs(y * ry[:, None])
    ta = (Sa * np.abs(A)).sum(0) * (sxr >= 1e-12)
    Sd = np.diag(Sa).copy()
    Ga = (Sa - np.diag(Sd) + ta[None, :]) / sx[None, :]
    Ma = Ga + Ga.T
    qa = (Ma * np.abs(1.0 - Dx)).sum(1)
    radial = 2.0 * Sd / sx * np.abs(np.diag(Dx))
    return ry[:, None] * (Ma @ yh + yh * (qa + radial)[:, None])


def selfsim(y, c, weight=None, eps_cost=EPS_COST, signs=None):
    """self_similarity(y, c) (weight None) or its column-weighted form (1/n) sum_j w_j sum_i |A_ij - B_ij|:
    (loss, grad, bound (flips and the rounding of the radial projection), number of ambiguous off-diagonal entries; the n diagonal ones, both sides rounding noise around 0,
    are always ambiguous).  signs: an explicit sign matrix for the ambiguous entries (tests)."""
    n = y.shape[0]
    Dx, sxr, sx, A, B, tau = _selfsim_parts(y, c, eps_cost)
    w = np.ones(n) if weight is None else np.asarray(weight, np.float64)
    diff = A - B
    loss = (np.abs(diff) * w[None, :]).sum() / n
    amb = np.abs(diff) < tau
    sg = np.where(amb, 0.0 if signs is None else signs, np.sign(diff))
    scale = w[None, :] / n
    grad, rnd = _selfsim_chain(y, Dx, sxr, sx, A, sg * scale, rounding=True)
    bound = _selfsim_chain_abs(y, Dx, sxr, sx, A, amb * scale) + rnd
    return loss, grad, bound, int(amb.sum() - np.diag(amb).sum())


def selfsim_ambiguous(y, c, eps_cost=EPS_COST):
    Dx, sxr, sx, A, B, tau = _selfsim_parts(y, c, eps_cost)
    return np.abs(A - B) < tau


# ------------------------------------------------------------------ moment matching (losses.py:39-52)
def cov_tau(v, rows=None):
    """stated |f32 - f64| bound of the covariance and of the mean of the rows of v"""
    rows = v.shape[0] if rows is None else rows
    cv = np.abs(v - v.mean(0))
    k = COV_K * U * (np.sqrt(rows) + 2.0)
    return k * (cv.T @ cv) / rows, k * np.abs(v).mean(0)


def moment_stats(v):
    m = v.mean(0)
    cv = v - m
    return m, cv.T @ cv / v.shape[0]


def moment(x, y, signs=None, signs_mean=None):
    """moment_matching(x, y) = mae(cov x, cov y) + mae(mean x, mean y), gradient w.r.t. y:
    (loss, grad, bound, number of ambiguous entries)."""
    n, d = y.shape
    mx, Sx = moment_stats(x)
    my, Sy = moment_stats(y)
    tcx, tmx = cov_tau(x)
    tcy, tmy = cov_tau(y)
    loss = np.abs(Sx - Sy).mean() + np.abs(mx - my).mean()
    dc, dm = Sy - Sx, my - mx
    amb, ambm = np.abs(dc) < tcx + tcy, np.abs(dm) < tmx + tmy
    T = np.where(amb, 0.0 if signs is None else signs, np.sign(dc)) / (d * d)
    cy = y - my
    dcy = cy @ (T + T.T) / n
    grad = dcy - dcy.mean(0, keepdims=True)
    grad = grad + np.where(ambm, 0.0 if signs_mean is None else signs_mean, np.sign(dm))[None, :] / (d * n)
    Ta = amb / (d * d)
    dca = np.abs(cy) @ (Ta + Ta.T) / n
    bound = dca + dca.mean(0, keepdims=True) + ambm[None, :] / (d * n)
    return loss, grad, bound, int(amb.sum() + ambm.sum())


# ------------------------------------------------------------------ relaxed EMD (losses.py:69-80)
def remd_weights(C, gx, gy, branch=None, tie="split"):
    """(loss, W = dL/dC, row branch taken) for L = max(mean_i min_j C, mean_j min_i C); ties = duplicate groups, split
    equally.  branch / tie override the rule (negative controls): branch 'row' / 'col', tie 'first' (all to one member)."""
    ns, n = C.shape
    rx, ry = C.min(1).mean(), C.min(0).mean()
    row = (rx >= ry) if branch is None else branch == "row"
    W = np.zeros_like(C)
    M, g_other, scale = (C, gy, ns) if row else (C.T, gx, n)
    Wv = W if row else W.T
    j = M.argmin(1)
    for a in range(M.shape[0]):
        members = np.flatnonzero(g_other == g_other[j[a]])
        if tie == "first":
            members = members[:1]
        Wv[a, members] = 1.0 / (scale * len(members))
    return (rx if row else ry), W, bool(row)


def remd(x, y, gx, gy, metric="cos", branch=None, tie="split"):
    """relaxed_emd(x, y, metric) at any width, metric 'cos' | 'l2' | 'both': (loss, grad w.r.t. y, row branch taken,
    elementwise bound of the f32 rounding of the l2 part's cancellation -- zero for 'cos')"""
    d = y.shape[1]
    G = x @ y.T
    nx, ny = (x * x).sum(1), (y * y).sum(1)
    rx, ry = inv_norm(x), inv_norm(y)
    cos = 1.0 - G * rx[:, None] * ry[None, :]
    m = nx[:, None] + ny[None, :] - 2.0 * G
    l2 = np.sqrt(np.maximum(m, 1e-6) / d)
    C = {"cos": cos, "l2": l2, "both": cos + l2}[metric]
    loss, W, row = remd_weights(C, gx, gy, branch, tie)
    grad = np.zeros_like(y)
    bound = np.zeros_like(y)
    if metric in ("cos", "both"):
        grad += unnormalise(y, ry, -(W.T @ (x * rx[:, None])), -(W * (1.0 - cos)).sum(0))
    if metric in ("l2", "both"):
        K = W * (m >= 1e-6) / (d * l2)                  # d l2_ij / d y_j = (y_j - x_i) / (d l2_ij)
        grad += K.sum(0)[:, None] * y - K.T @ x
        # m = |x|^2 + |y|^2 - 2 x.y cancels where x_i and y_j are close (the palette's nearest colours): its f32 error
        # dm <= (4 + sqrt(d)) U (|x|^2 + |y|^2 + 2 |x.y|) moves l2 by dm / (2 m) relative, and y_j - x_i has an error of
        # 2 U (|x_i| + |y_j|): per selected entry |K| (|y_j - x_i| dm / (2 m) + 2 U (|x_i| + |y_j|))
        i, j = np.nonzero(K)
        dm = (4.0 + np.sqrt(d)) * U * (nx[i] + ny[j] + 2.0 * np.abs(G[i, j]))
        k = np.abs(K[i, j])[:, None]
        diff = np.abs(y[j] - x[i])
        np.add.at(bound, j, k * (diff * (dm / (2.0 * m[i, j]))[:, None] + 2.0 * U * (np.abs(x[i]) + np.abs(y[j]))))
    return loss, grad, row, bound


def palette(x, y, gx, gy, yuv=True, branch=None, tie="split"):
    """relaxed_emd(yuv(x[:, :3]), yuv(y[:, :3]), 'both') (run_strotss.py:36-39; yuv False: on RGB): (loss, gradient w.r.t.
    the prediction's RGB columns, row branch taken, bound as remd's)"""
    P = RGB2YUV if yuv else np.eye(3)
    loss, g, row, b = remd(x[:, :3] @ P, y[:, :3] @ P, gx, gy, "both", branch, tie)
    return loss, g @ P.T, row, b @ np.abs(P.T)
