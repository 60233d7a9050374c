"""Float64 restatement of the sliced palette term (strotss_palette_sliced_fwd_bwd, StepEngine(palette_transport="sliced"),
DESIGN.md section 25) in NumPy alone, with its analytic gradient, and the bounds tests/test_hip_palette_sliced.py holds the
library to.

With y_i = yuv(pred_i[:3]) (i < n), s_j = yuv(style_j[:3]) (j < ns), yuv(x) = x @ RGB2YUV (convert_rgb_to_yuv) and P unit
directions theta_p of R^3 (nn.rand.palette_directions):
    a[p][i] = <theta_p, y_i>, b[p][j] = <theta_p, s_j>, each product summed left to right, each set sorted by (value, row)
    W_p  = sum_ij len_ij |a_(i) - b_(j)|,  len_ij = max(0, min((i+1) ns, (j+1) n) - max(i ns, j n)) / (n ns)
    loss = (2 / (sqrt(3) P)) sum_p W_p
    dloss/da[p][i] = (2 / (sqrt(3) P)) sum_j len_{rank(i), j} sign(a[p][i] - b_(j)),  sign(0) = 0
    dy_i = sum_p dloss/da[p][i] theta_p (p ascending),  dpred_i[:3] = dy_i @ RGB2YUV^T
For theta uniform on the sphere E|<theta, v>| = |v| / 2, so for a fixed coupling the expectation of the loss is
sum_ij pi_ij |y_i - s_j| / sqrt(3): the l2_distance part of the 'both' cost of the palette relaxed EMD.

Yardstick: the same function with every array in float32.  Tie-free cases (tests/_palette_sliced_cases.py):
err32 = max|g32 - g64| / max|g64| per case, its worst value per family pinned in ERR32, the per-element tolerance
TOL_GRAD[family] = MARGIN * ERR32[family] (MARGIN = 8, the project's margin for loss operators).  Full-shape cases hold
near-ties that float32 decides either way: there the gradient is held in relative Frobenius norm to MARGIN times the float32
restatement's own relative Frobenius error at that case (FRO32)."""
import functools

import numpy as np

RGB2YUV = np.array([[0.299, -0.14714119, 0.61497538],
                    [0.587, -0.28886916, -0.51496512],
                    [0.114, 0.43601035, -0.10001026]], dtype=np.float64)
MARGIN = 8.0
LOSS_TOL = 5e-5            # the project's loss_tolerance (_sinkhorn_ref.loss_tolerance at a zero stated bound)
# worst err32 per family over _palette_sliced_cases.ELEMENTWISE, as printed by tests/test_palette_sliced_cpu.py (which asserts
# that a run's worst lies between a quarter and twice the pinned value)
ERR32 = {
    "yuv": 1.3e-7,       # n64_ns37_p8
    "raw": 8.8e-8,       # n37_ns64_p8
    # the constructed line cases (widths 256, 512 and 1024) hold their own values
    "line_yuv": 1.2e-7,  # line_n1023_ns1024_p8
    "line_raw": 1.5e-7,  # line_n513_ns300_p8
}
TOL_GRAD = {k: MARGIN * v for k, v in ERR32.items()}
# relative Frobenius error of the float32 restatement's gradient at the full-shape cases (same test, same window)
FRO32 = {
    "full_n1024_ns1024_p64": 1.0e-7,
    "full_n1024_ns1024_p1024": 1.7e-7,
    "full_n1000_ns1024_p33": 6.8e-8,
    "full_n768_ns600_p64": 1.0e-7,
    "full_n1024_ns1_p64": 1.8e-3,        # float32 turns one sign: |a - b| = 5.4e-9 in direction 26
    "full_n1_ns1024_p64": 1.1e-7,
}
TOL_FRO = {k: MARGIN * v for k, v in FRO32.items()}


def family(case):
    return ("line_" if case.kind.startswith("line") else "") + ("yuv" if case.rgb_to_yuv else "raw")


@functools.lru_cache(maxsize=None)
def overlaps(n, ns):
    """(I, J, LEN): the pairs of quantile cells that overlap and the overlap in units of 1 / (n ns), whole numbers; I ascending"""
    I, J, LEN = [], [], []
    for i in range(n):
        lo, hi = i * ns, (i + 1) * ns
        j = lo // n
        while j < ns and j * n < hi:
            I.append(i); J.append(j); LEN.append(min(hi, (j + 1) * n) - max(lo, j * n))
            j += 1
    return np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(LEN, np.int64)


def yuv(x, rgb_to_yuv=True):
    """x[:, :3] @ RGB2YUV, each product rounded on its own and summed left to right (no library GEMM: its order is not fixed)"""
    x = x[:, :3]
    if not rgb_to_yuv:
        return x
    m = RGB2YUV.astype(x.dtype)
    return (x[:, 0:1] * m[0][None, :] + x[:, 1:2] * m[1][None, :]) + x[:, 2:3] * m[2][None, :]


def projections(rows, dirs, rgb_to_yuv=True):
    """(P, rows) projections, each product summed left to right"""
    y = yuv(rows, rgb_to_yuv)
    return (dirs[:, 0:1] * y[None, :, 0] + dirs[:, 1:2] * y[None, :, 1]) + dirs[:, 2:3] * y[None, :, 2]


def order_of(a, descending_ties=False):
    """per direction the rows in ascending (value, row) order; -0 == +0 compares equal, the stable sort keeps the rows'"""
    if descending_ties:
        return a.shape[1] - 1 - np.argsort(a[:, ::-1], axis=1, kind="stable")
    return np.argsort(a, axis=1, kind="stable")


def palette_sliced(style, pred, dirs, rgb_to_yuv=True, dtype=np.float64, weights="len", scale=True, transpose=True,
                   descending_ties=False, swap_rank=None):
    """(loss, dloss/dpred[:, :3] (n, 3)) as float64: style (ns, >= 3), pred (n, >= 3), dirs (P, 3), computed in `dtype`.  The
    keywords plant errors for the negative controls: weights="max" takes 1 / max(n, ns) for every overlapping pair,
    scale=False drops 2 / sqrt(3), transpose=False applies RGB2YUV in place of its transpose in the backward,
    descending_ties sorts equal values by descending row, swap_rank=(p, r) exchanges the sorted prediction ranks r and r + 1 of
    direction p (two misplaced elements of one sort)."""
    x = np.asarray(style, dtype)[:, :3]
    y = np.asarray(pred, dtype)[:, :3]
    th = np.asarray(dirs, dtype)
    n, ns, P = y.shape[0], x.shape[0], th.shape[0]
    a, b = projections(y, th, rgb_to_yuv), projections(x, th, rgb_to_yuv)
    oa, ob = order_of(a, descending_ties), order_of(b, descending_ties)
    if swap_rank is not None:
        p, r = swap_rank
        oa = oa.copy()
        oa[p, [r, r + 1]] = oa[p, [r + 1, r]]
    a_s, b_s = np.take_along_axis(a, oa, 1), np.take_along_axis(b, ob, 1)
    I, J, LEN = overlaps(n, ns)
    if weights == "len":
        wgt = LEN.astype(dtype) * dtype(1.0 / (float(n) * float(ns)))
    else:
        wgt = np.full(len(LEN), 1.0 / max(n, ns), dtype)
    diff = a_s[:, I] - b_s[:, J]
    c = dtype((2.0 / np.sqrt(3.0) if scale else 1.0) / P)
    loss = c * (wgt[None, :] * np.abs(diff)).sum(1, dtype=dtype).sum(dtype=dtype)
    starts = np.flatnonzero(np.r_[True, I[1:] != I[:-1]])
    coef_sorted = np.add.reduceat(wgt[None, :] * np.sign(diff), starts, axis=1)          # (P, n) at the sorted position
    coef = np.empty_like(coef_sorted)
    np.put_along_axis(coef, oa, coef_sorted, 1)                                           # at the original row
    dy = np.zeros((n, 3), dtype)
    for p in range(P):                                                                    # p ascending
        dy += coef[p][:, None] * th[p][None, :]
    dy *= c
    m = RGB2YUV.astype(dtype)
    g = (dy @ (m.T if transpose else m)) if rgb_to_yuv else dy
    return float(loss), g.astype(np.float64)


def err_over_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def rel_fro(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def min_gap(style, pred, dirs, rgb_to_yuv=True, skip_exact=False):
    """the smallest float64 gap of a case: between neighbours within each sorted set and between any a and any b of a direction.
    skip_exact: gaps that are exactly 0 (the duplicate rows, a prediction equal to the style) are left out."""
    a = projections(np.asarray(pred, np.float64), np.asarray(dirs, np.float64), rgb_to_yuv)
    b = projections(np.asarray(style, np.float64), np.asarray(dirs, np.float64), rgb_to_yuv)
    worst = np.inf
    for p in range(a.shape[0]):
        both = np.sort(np.concatenate([a[p], b[p]]))          # neighbours of the merged set cover all three kinds of pairs
        gaps = np.diff(both)
        if skip_exact:
            gaps = gaps[gaps != 0.0]
        if gaps.size:
            worst = min(worst, float(gaps.min()))
    return worst
