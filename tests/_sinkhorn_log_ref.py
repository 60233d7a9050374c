"""Float64 restatement of the log-domain Sinkhorn term (strotss_sinkhorn_log_cos_fwd_bwd_panels) and
the tolerances tests/test_hip_sinkhorn_log.py holds the GPU to (CPU side: tests/test_sinkhorn_log_cpu.py).

With M[i][j] the cosine distance (i < ns style row, j < n prediction row; the norms and the 1e-12 guard of
oracle.cosine_distance), px = 1 / ns, py = 1 / n, phi = log u, psi = log v and psi_0 = 0, for t = 1 .. T:

    phi_t[i] = log px - LSE_j(psi_{t-1}[j] - L M[i][j])
    psi_t[j] = log py - LSE_i(phi_t[i]    - L M[i][j])
    loss     = sum_ij exp(phi_T[i] + psi_T[j] - L M[i][j]) M[i][j]

LSE is the max-shifted log-sum-exp; there is no clamp and no K matrix; the gradient goes through all T iterations by
torch.autograd (no hand-written reverse sweep: the kernels' derivation is not shared).  Wherever oracle.sinkhorn_knopp
engages no clamp the two are the same function.

Yardstick, as tests/_sinkhorn_ref.py: err32 = the float32-CPU run of this restatement against its float64 run, the loss
relative, the gradient element-wise over max|ref|; its worst per family is pinned in ERR32 (tests/test_sinkhorn_log_cpu.py
prints every case's and asserts the pin), the GPU's tolerance is TOL_SK[family] = MARGIN * ERR32[family], and every family
has to meet CAP: a tolerance above 1e-3 of max|ref| could hide a wrong kernel.  The loss keeps the project's TOL_SCALAR.

The switches of `sinkhorn_log` are the negative controls (unswitched: the statement above)."""
import numpy as np
import torch

from oracle import strotss_oracle as O

MARGIN = 8.0
CAP = 1e-3
TOL_SCALAR = 5e-5
COL_CHUNKS = 16
# worst err32 per family over tests/_sinkhorn_log_cases.py, as printed by tests/test_sinkhorn_log_cpu.py (which asserts that
# a run's worst is at most twice the pinned value, and that MARGIN times the pinned value meets CAP).  A family is the range
# of L (the exponent phi + psi - L M is rounded to f32 at a magnitude of up to 2 L) and whether the case is a full shape
# (d = 2179, n ns >= 300000: more terms in every sum).
ERR32 = {
    "l10": 1.7e-6,           # L <= 10 at d = 35 (ns257_n256)
    "l10_full": 5.5e-6,      # ns600_n768_d2179_L10
    "l100": 3.3e-5,          # L = 100 at d = 35 (ns200_n256_L100 1.6e-5, the far-row cases 2.8e-5 and 3.3e-5)
    "l100_full": 9.5e-5,     # ns600_n768_d2179_L100 (ns1024_n1024_d2179_L100 6.9e-5)
    "lmax": 7.9e-5,          # ns200_n256_Lmax at L = 500
}
# the loss, relative: 1.7e-6 at L = 500 and below 8e-7 elsewhere.  MARGIN times it lies below the project's TOL_SCALAR in every
# family (asserted on the CPU), so the loss keeps TOL_SCALAR as its tolerance, as the linear term's tests do.
ERR32_LOSS = {"l10": 1.4e-7, "l10_full": 1.7e-7, "l100": 7.8e-7, "l100_full": 3.4e-7, "lmax": 1.7e-6}
TOL_SK = {k: MARGIN * v for k, v in ERR32.items()}


def family(case):
    base = "l10" if case.l <= 10.0 else "l100" if case.l <= 100.0 else "lmax"
    return base + "_full" if case.full and base != "lmax" else base


def _t(a, dtype):
    return torch.as_tensor(np.asarray(a), dtype=dtype)


def lse(a, dim, shift=True):
    """log sum exp over `dim` (kept), shifted by the maximum unless shift is False"""
    if not shift:
        return torch.log(torch.exp(a).sum(dim=dim, keepdim=True))
    return torch.logsumexp(a, dim=dim, keepdim=True)          # shifted by the maximum; saves only its input and output


def potentials(x, y, l, T, swap_marginals=False, psi0_log_py=False, shift=True):
    """(M, phi_T (ns, 1), psi_T (1, n)) of the statement above"""
    M = O.cosine_distance(x, y)
    ns, n = M.shape
    lpx, lpy = float(np.log(1.0 / ns)), float(np.log(1.0 / n))
    if swap_marginals:
        lpx, lpy = lpy, lpx
    psi = torch.full((1, n), lpy if psi0_log_py else 0.0, dtype=M.dtype)
    phi = None
    for _ in range(int(T)):
        phi = lpx - lse(psi - l * M, 1, shift)
        psi = lpy - lse(phi - l * M, 0, shift)
    return M, phi, psi


def sinkhorn_log(x, y, l=10.0, T=30, **switches):
    M, phi, psi = potentials(x, y, float(l), T, **switches)
    return (torch.exp(phi + psi - l * M) * M).sum()


def run(x, y, l, T, dtype=torch.float64, **switches):
    """(loss, gradient w.r.t. y) as float64 NumPy, computed in `dtype` by autograd"""
    xt, yt = _t(x, dtype), _t(y, dtype).requires_grad_(True)
    out = sinkhorn_log(xt, yt, l, T, **switches)
    g, = torch.autograd.grad(out, yt)
    return float(out.detach()), g.double().numpy()


def row_marginals(x, y, l, T, dtype=torch.float64):
    """sum_j P_ij of the log form's plan after the last half-step, (ns,)"""
    with torch.no_grad():
        M, phi, psi = potentials(_t(x, dtype), _t(y, dtype), float(l), T)
        return torch.exp(phi + psi - l * M).sum(1).double().numpy()


def linear_row_marginals(x, y, l, T):
    """the same of oracle.sinkhorn_knopp's plan u K v in float64, and the smallest argument of its first clamp"""
    with torch.no_grad():
        xt, yt = _t(x, torch.float64), _t(y, torch.float64)
        K = torch.exp(-l * O.cosine_distance(xt, yt))
        v = torch.ones(yt.shape[0], 1, dtype=torch.float64)
        least = np.inf
        for _ in range(int(T)):
            a = K @ v
            least = min(least, float(a.min()))
            u = (1.0 / xt.shape[0]) / torch.clamp(a, min=1e-12)
            v = (1.0 / yt.shape[0]) / torch.clamp(K.t() @ u, min=1e-12)
        return (u * (K @ v)).numpy().ravel(), least


def err_over_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# ------------------------------------------------------------------ the chunked column reduction, restated in NumPy float32
def chunked_column_lse(a, empty=(-np.inf, 0.0)):
    """LSE over the rows of a (n, ns) the way the column pass reduces it: COL_CHUNKS row chunks of ceil(n / COL_CHUNKS) rows,
    each an online (max, sum) pair, a chunk without rows `empty`, the pairs combined in the order 0 .. 15 with the guard that
    keeps two empty pairs from forming -inf - (-inf).  float32 throughout, as the kernel."""
    a = np.asarray(a, np.float32)
    n, ns = a.shape
    per = (n + COL_CHUNKS - 1) // COL_CHUNKS
    pairs = []
    for k in range(COL_CHUNKS):
        rows = a[k * per:min(n, (k + 1) * per)]
        if rows.shape[0] == 0:
            pairs.append((np.full(ns, empty[0], np.float32), np.full(ns, empty[1], np.float32)))
        else:
            m = rows.max(0)
            pairs.append((m, np.exp(rows - m).sum(0, dtype=np.float32)))
    m, s = pairs[0]
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for m2, s2 in pairs[1:]:
            mx = np.maximum(m, m2)
            live = mx > -np.inf
            safe = np.where(live, mx, np.float32(0))
            s = np.where(live, s * np.exp(m - safe) + s2 * np.exp(m2 - safe), np.float32(0)).astype(np.float32)
            m = mx
        return (m + np.log(s)).astype(np.float32)


def run_chunked32(x, y, l, T, empty=(-np.inf, 0.0)):
    """phi_T of the iteration in NumPy float32 with the column pass reduced by chunked_column_lse (the row pass plain)"""
    M = O.cosine_distance(_t(x, torch.float64), _t(y, torch.float64)).numpy().astype(np.float32)      # (ns, n)
    ns, n = M.shape
    lf = np.float32(l)
    lpx, lpy = np.float32(np.log(1.0 / ns)), np.float32(np.log(1.0 / n))
    psi = np.zeros(n, np.float32)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        for _ in range(int(T)):
            phi = lpx - chunked_column_lse((psi[None, :] - lf * M).T, empty)
            a = phi[:, None] - lf * M
            mx = a.max(0)
            psi = (lpy - (mx + np.log(np.exp(a - mx).sum(0, dtype=np.float32)))).astype(np.float32)
    return phi.astype(np.float64)


# ------------------------------------------------------------------ the step
def style_loss_sinkhorn_log(target, prediction, alpha, l, T):
    """_transport_ref.style_loss_sinkhorn with the log form in place of oracle.sinkhorn_knopp"""
    inv_alpha = 1 / max(alpha, 1)
    l_m = O.moment_matching(target, prediction)
    l_sk = sinkhorn_log(target, prediction, float(l), int(T))
    l_pal = O.relaxed_emd(O.convert_rgb_to_yuv(target), O.convert_rgb_to_yuv(prediction), "both")
    return l_m + l_sk + inv_alpha * l_pal


def reference_step(P, l, T, dtype=torch.float64, blend_weights=None, vgg=None):
    """_transport_ref.reference_step (same problem P, same outputs) with style_loss_sinkhorn_log as the style loss"""
    import _transport_ref as TR
    saved = TR.style_loss_sinkhorn
    TR.style_loss_sinkhorn = style_loss_sinkhorn_log
    try:
        return TR.reference_step(P, l, T, dtype, blend_weights=blend_weights, vgg=vgg)
    finally:
        TR.style_loss_sinkhorn = saved


# worst float32-CPU distance of the step restatement from its float64 run over _transport_cases.STEPS and the blend step at
# L = 10 and L = 100, as printed by tests/test_sinkhorn_log_cpu.py: (scalars relative to max(1, |ref|), gradients in relative
# L2).  Recorded, not asserted, as _transport_ref.STEP32 (the float32 sums depend on the machine's thread count).
STEP32 = {10.0: {"scalar": 5.3e-8, "grad": 2.8e-4}, 100.0: {"scalar": 5.1e-8, "grad": 2.8e-4}}      # gradients: 5.0e-5 at most with one style


def step_bounds(l):
    """(scalar bound, gradient bound) of a step at this L: _transport_ref's TOL_SCALAR and GRAD_TOL where the recorded float32
    distance stays within a quarter of them, MARGIN times the recorded distance where it does not"""
    import _transport_ref as TR
    rec = STEP32[float(l)]
    return (TR.TOL_SCALAR if rec["scalar"] <= TR.TOL_SCALAR / 4 else MARGIN * rec["scalar"],
            TR.GRAD_TOL if rec["grad"] <= TR.GRAD_TOL / 4 else MARGIN * rec["grad"])
