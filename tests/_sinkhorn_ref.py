"""References and tolerances of the Sinkhorn and pairwise-distance tests (tests/test_sinkhorn_cases_cpu.py on the CPU,
tests/test_hip_sinkhorn.py on the GPU).

Reference: loss and d(loss)/d(pred) of oracle.strotss_oracle.sinkhorn_knopp in torch float64 AUTOGRAD on the CPU (no
hand-written reverse sweep: the kernels' derivation is not shared).  Yardstick: the same function in torch float32 on the
CPU; err32 = max|g32 - g64| / max|g64| per case.  Its worst value per family is pinned below (ERR32), and the per-element
gradient tolerance is TOL_SK[family] = MARGIN * ERR32[family]:  |got - ref| <= TOL_SK * max|ref|.

Why a margin of 8: the kernels sum in other orders than torch's CPU kernels and use __expf, whose relative error grows like
|l M| 2^-23 (about 5e-6 at l M = 30), and their reverse sweep is hand-written; none of these should cost more than a small
multiple of the f32 noise of the operation itself.

`variant` restates the iteration with switches for the negative controls (unswitched it equals the oracle: asserted)."""
import numpy as np
import torch

import _sinkhorn_cases as SC
from oracle import strotss_oracle as O

MARGIN = 8.0
U = 2.0 ** -24             # f32 unit roundoff
# worst err32 per family over tests/_sinkhorn_cases.py, as printed by tests/test_sinkhorn_cases_cpu.py (which asserts that a
# run's worst lies between a quarter and twice the pinned value).  Five families where three would do: d = 1 (where
# m = x^2 + y^2 - 2 x y cancels to a few digits in f32) and the all-clamped case (where l = 400 multiplies the f32 rounding of
# the cost entries) would otherwise set the tolerance of the d = 3 and of the cosine cases.
ERR32 = {
    "cosine": 2.6e-6,
    "wide": 2.8e-6,          # 'l2' / 'both' at d >= 35
    "narrow": 1.2e-4,        # 'l2' / 'both' at d = 3 (n100_ns31_rgb 1.5e-5, n4096_ns2_far_row 1.1e-4)
    "d1": 5.3e-4,            # 'l2' / 'both' at d = 1
    "all_clamped": 1.1e-4,
}
TOL_SK = {k: MARGIN * v for k, v in ERR32.items()}
# pairwise distances with a random upstream gradient, gradients to both sides: the same construction
ERR32_PAIR = {
    "wide": 5.5e-7,          # cosine at every width, 'l2' / 'both' at d >= 35
    "narrow": 7.2e-7,        # 'l2' / 'both' at d = 3
}
TOL_PAIR = {k: MARGIN * v for k, v in ERR32_PAIR.items()}
# the l of every run that does not take 10: 'l2' / 'both' take the largest of SC.L_CHOICES that is conditioned, the
# all-clamped case the first of SC.L_CLAMPED (choose_l; the CPU test asserts that this table is what choose_l gives)
L_TAKEN = {
    ("n1_ns33", "l2"): 5.0, ("n1_ns33", "both"): 5.0,
    ("n17_ns1", "l2"): 5.0, ("n17_ns1", "both"): 5.0,
    ("n37_ns65_all_clamped", "cosine"): 400.0,
}


def l_of(label, metric):
    return L_TAKEN.get((label, metric), 10.0)


def family(case, metric):
    if case.kind == "all_clamped":
        return "all_clamped"
    return "cosine" if metric == "cosine" else "d1" if case.d == 1 else case.family_d


def pair_family(d, kind):
    return "narrow" if d <= 3 and kind != "cosine" else "wide"


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def sinkhorn(x, y, metric, l, T, dtype=torch.float64, fn=O.sinkhorn_knopp):
    """(loss, gradient w.r.t. y) as float64 NumPy, computed in `dtype` by autograd"""
    xt, yt = _t(x, dtype), _t(y, dtype).requires_grad_(True)
    out = fn(xt, yt, metric, float(l), int(T))
    g, = torch.autograd.grad(out, yt)
    return float(out.detach()), g.double().numpy()


def clamp_arguments(x, y, metric, l, T):
    """float64: (all K v arguments, all K^T u arguments) over the T iterations, each a flat array"""
    with torch.no_grad():
        xt, yt = _t(x, torch.float64), _t(y, torch.float64)
        K = torch.exp(-l * O.dist_metrics[metric](xt, yt))
        p, q = 1.0 / xt.shape[0], 1.0 / yt.shape[0]
        v = torch.ones(yt.shape[0], 1, dtype=torch.float64)
        kv, ktu = [], []
        for _ in range(T):
            a = K @ v
            u = p / torch.clamp(a, min=SC.CLAMP_EPS)
            b = K.t() @ u
            v = q / torch.clamp(b, min=SC.CLAMP_EPS)
            kv.append(a.numpy().ravel()); ktu.append(b.numpy().ravel())
    return np.concatenate(kv), np.concatenate(ktu)


def conditioned(case, metric, l):
    kv, ktu = clamp_arguments(case.x, case.y, metric, l, case.T)
    if case.kind == "all_clamped":
        return bool((kv <= SC.CLAMPED_BELOW).all() and ((ktu <= SC.CLAMPED_BELOW) | (ktu >= SC.CLAMPED_ABOVE)).all())
    return bool(min(kv.min(), ktu.min()) >= SC.CLAMP_CLEAR)


def choose_l(case, metric):
    """the case's l, or None when no choice is conditioned"""
    if case.kind == "all_clamped":
        choices = SC.L_CLAMPED
    else:
        choices = (SC.L_COSINE,) if metric == "cosine" else SC.L_CHOICES
    for l in choices:
        if conditioned(case, metric, l):
            return l
    return None


def variant(x, y, distance="cosine", l=10.0, N_iter=30, second_marginal_ns=False, v0_over_n=False, l2_through_clamp=False,
            drop_cosine_chain=False):
    """oracle.sinkhorn_knopp restated with one planted error each: second marginal 1 / ns; v_0 = 1 / n; the l2 gradient let
    through tf.maximum(m, 1e-6) where it clamps; for 'both', the cosine part held constant in the chain rule."""
    cos = O.cosine_distance(x, y)
    if distance != "cosine":
        m = (x ** 2).sum(1).view(-1, 1) + (y ** 2).sum(1).view(1, -1) - 2.0 * (x @ y.T)
        mc = torch.clamp(m, min=1e-6)
        if l2_through_clamp:
            mc = mc.detach() + (m - m.detach())
        l2 = torch.sqrt(mc / x.shape[1])
    M = {"cosine": cos, "l2": None if distance == "cosine" else l2,
         "both": None if distance == "cosine" else (cos.detach() if drop_cosine_chain else cos) + l2}[distance]
    K = torch.exp(-l * M)
    p = 1.0 / x.shape[0]
    q = 1.0 / (x.shape[0] if second_marginal_ns else y.shape[0])
    v = torch.full((y.shape[0], 1), 1.0 / y.shape[0] if v0_over_n else 1.0, dtype=M.dtype)
    for _ in range(N_iter):
        u = p / torch.clamp(K @ v, min=1e-12)
        v = q / torch.clamp(K.t() @ u, min=1e-12)
    return (u * ((K * M) @ v)).sum()


def loss_tolerance(case, l):
    """relative tolerance of the loss value: the project's TOL_SCALAR; the all-clamped case adds l U (sqrt(d) + 2).  There
    u = p / eps and v = q / eps wherever both clamps act, so the loss is (p q / eps^2) sum K M over those entries and moves by
    l dM relative when the cost entries move by dM; a cosine entry is one minus a dot product of d terms of two unit vectors,
    whose f32 error is bounded by U (sqrt(d) + 2) however the products are ordered (the form of _loss_ref.COV_K).  At
    l = 400, d = 131 that is 3.2e-4: f32 cannot hold this loss to 5e-5 (torch's own f32 run misses it: 1.0e-4)."""
    from _loss_ref import TOL_SCALAR
    return TOL_SCALAR + (l * U * (np.sqrt(case.d) + 2.0) if case.kind == "all_clamped" else 0.0)


def err_over_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ------------------------------------------------------------------ pairwise distances
def pair_grads(x, y, G, kind, dtype=torch.float64):
    """(dx, dy) of sum(G * dist_metrics[kind](x, y)) by autograd in `dtype`, as float64 NumPy"""
    xt, yt = _t(x, dtype).requires_grad_(True), _t(y, dtype).requires_grad_(True)
    out = (O.dist_metrics[kind](xt, yt) * _t(G, dtype)).sum()
    gx, gy = torch.autograd.grad(out, (xt, yt))
    return gx.double().numpy(), gy.double().numpy()


# ------------------------------------------------------------------ strotss_rows_gemm_bwd


def rows_gemm(W, B, x, r, q, g, k, base):
    """(added dx, per-element bound): g r_i (sum_j W_ij B_j - x_i r_i q_i) over ALL columns of W, in float64, and
    4 U (sqrt(k) + 2) |g| r_i (sum_j |W_ij| |B_j| + |x_i| r_i |q_i|), the form _loss_ref._selfsim_chain uses for this GEMM
    (k = the number of non-zero terms of the sum; zero terms add exactly), plus the one rounding no f32 `+=` onto a
    non-zero base can avoid, U |base + added| (taken twice: the base itself is given in f32, the sum in float64)."""
    out = g * r[:, None] * (W @ B - x * (r * q)[:, None])
    bound = 4.0 * U * (np.sqrt(k) + 2.0) * abs(g) * r[:, None] * (np.abs(W) @ np.abs(B) + np.abs(x) * (r * np.abs(q))[:, None])
    return out, bound + 2.0 * U * np.abs(base + out)
