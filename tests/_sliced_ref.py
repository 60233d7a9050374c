"""Float64 restatement of the sliced Wasserstein style term (strotss_sliced_cos_fwd_bwd, StepEngine(style_transport=
"sliced")) with torch autograd, and the bounds tests/test_hip_sliced.py holds the library to.

With xhat_i (i < n) the prediction rows and shat_j (j < ns) the style rows, L2-normalised by rsqrt(max(|x|^2, 1e-12)), and
P sign directions eps_p (nn.rand.sliced_signs: the host twin of the device's Philox bits):
    a[p][i] = <eps_p, xhat_i>, b[p][j] = <eps_p, shat_j>, each direction sorted by torch.sort(stable=True): by (value, row)
    W_p  = sum_ij len_ij (a_(i) - b_(j))^2,  len_ij = max(0, min((i+1) ns, (j+1) n) - max(i ns, j n)) / (n ns)
    loss = sum_p W_p / (2 P)
len_ij is the overlap of the quantile cells [i/n, (i+1)/n] and [j/ns, (j+1)/ns]: at most n + ns - 1 pairs overlap, listed by
`overlaps` in integer arithmetic, so W_p is a sum over that list and no n x ns matrix is formed.  The sort's permutation is
piecewise constant: autograd through torch.sort gives the gradient the library computes.

Yardstick: the same function in torch float32 on the CPU.  Operator cases that are tie-free (tests/_sliced_cases.py):
err32 = max|g32 - g64| / max|g64| per case, its worst value per family pinned in ERR32, and the per-element tolerance is
TOL_GRAD[family] = MARGIN * ERR32[family] (MARGIN = 8, the project's margin for loss operators: the library sums in other
orders than torch's CPU kernels, none of which should cost more than a small multiple of the operation's own f32 noise).
Full-shape cases hold near-ties that float32 decides either way: there the gradient is held in relative Frobenius norm to
MARGIN times the float32 restatement's own relative Frobenius error at that case (FRO32)."""
import functools

import numpy as np
import torch

import _transport_ref as TR
from oracle import strotss_oracle as O

MARGIN = 8.0
# worst err32 per family over _sliced_cases.ELEMENTWISE, as printed by tests/test_sliced_cpu.py (which asserts that a run's
# worst lies between a quarter and twice the pinned value)
ERR32 = {
    "wide": 2.2e-6,      # d = 35 (n130_ns130_p4)
    "narrow": 6.3e-7,    # d = 3 (n96_ns33_p2_rgb, the only one)
    # the constructed arc cases (widths 512 and 1024) hold their own values: both sides lie on one arc, so a - b is a fraction
    # of a grid step and the gradient is small against the projections' own float32 error
    "arc_wide": 6.1e-4,      # d = 35 (arc_n1024_ns513_p4)
    "arc_narrow": 3.3e-4,    # d = 3 (arc_n1023_ns1024_p4)
}
TOL_GRAD = {k: MARGIN * v for k, v in ERR32.items()}
# relative Frobenius error of the float32 restatement's gradient at the full-shape cases (same test, same window)
FRO32 = {
    "full_n1024_ns1024_p256": 6.7e-4,
    "full_n768_ns600_p64": 3.2e-4,
    "full_n1000_ns1024_p33": 8.1e-4,
    "full_n1024_ns1024_p1024": 6.7e-4,
}
TOL_FRO = {k: MARGIN * v for k, v in FRO32.items()}


def family(case):
    shape = "narrow" if case.d <= 3 else "wide"
    # an arc case with one atom on a side has a - b of order one, like the searched cases: it is held to their tolerance
    return "arc_" + shape if case.kind.startswith("arc") and min(case.n, case.ns) > 1 else shape


@functools.lru_cache(maxsize=None)
def overlaps(n, ns):
    """(I, J, LEN): the pairs of quantile cells that overlap and the overlap in units of 1 / (n ns), whole numbers"""
    I, J, LEN = [], [], []
    for i in range(n):
        lo, hi = i * ns, (i + 1) * ns
        j = lo // n
        while j < ns and j * n < hi:
            I.append(i); J.append(j); LEN.append(min(hi, (j + 1) * n) - max(lo, j * n))
            j += 1
    return np.asarray(I, np.int64), np.asarray(J, np.int64), np.asarray(LEN, np.int64)


def len_matrix(n, ns):
    """the overlaps as an (n, ns) matrix of whole numbers (units of 1 / (n ns)): for the property tests"""
    I, J, LEN = overlaps(n, ns)
    m = np.zeros((n, ns), np.int64)
    m[I, J] = LEN
    return m


def normalise(x):
    return x * torch.rsqrt(torch.clamp((x * x).sum(1, keepdim=True), min=1e-12))


def projections(x, signs):
    """(P, rows) projections of the normalised rows of x.  Identical rows must take identical bits wherever they stand, so
    that the stable sort breaks their tie by the row and a permuted copy of a set matches it exactly; a CPU GEMM may sum a row
    in another order at another position or alignment (seen at rows 5 and 900 of 1024, d = 35, and between a 64-row matrix
    and its permutation).  In float64 the value is therefore taken from sums that are exact in any order: with |xhat| <= 1,
    q1 = round(xhat 2^40) and q2 = round((xhat - q1 2^-40) 2^80) are whole numbers below 2^41, at most 2^12 signed terms of
    them stay below 2^53, and what is dropped is below 2^-81 a term; the gradient still flows through the plain product.  In
    float32 (the yardstick) the product's bits are kept, and rows repeated within x take the bits of the first of them."""
    xhat = normalise(x)
    proj = (xhat @ signs.T).T.contiguous()
    if x.dtype == torch.float64:
        assert x.shape[1] <= 4096
        with torch.no_grad():
            q1 = torch.round(xhat * 2.0 ** 40)
            q2 = torch.round((xhat - q1 * 2.0 ** -40) * 2.0 ** 80)
            exact = ((q1 @ signs.T) * 2.0 ** -40 + (q2 @ signs.T) * 2.0 ** -80).T.contiguous()
        return exact + (proj - proj.detach())
    rows = x.detach().numpy()
    _, first, inverse = np.unique(rows, axis=0, return_index=True, return_inverse=True)
    if len(first) == rows.shape[0]:
        return proj
    src = torch.as_tensor(first[inverse.reshape(-1)])
    return proj + (proj[:, src] - proj).detach()


def sliced_loss(target, prediction, signs, weights="len", half=True, descending_ties=False, swap_rank=None):
    """the term on torch tensors of one dtype: target (ns, d) style rows, prediction (n, d), signs (P, d).  The keywords plant
    errors for the negative controls: weights="max" takes 1 / max(n, ns) for every overlapping pair, half=False drops the
    1/2, descending_ties sorts equal values by descending row, swap_rank=(p, r) exchanges the sorted prediction ranks r and
    r + 1 of direction p (two misplaced elements of one sort)."""
    n, ns, P = prediction.shape[0], target.shape[0], signs.shape[0]
    a, b = projections(prediction, signs), projections(target, signs)
    if descending_ties:
        a_s, b_s = _sort_desc_ties(a), _sort_desc_ties(b)
    else:
        a_s, b_s = torch.sort(a, dim=1, stable=True)[0], torch.sort(b, dim=1, stable=True)[0]
    if swap_rank is not None:
        p, r = swap_rank
        perm = torch.arange(n)
        perm[r], perm[r + 1] = r + 1, r
        a_s = torch.cat([a_s[:p], a_s[p:p + 1][:, perm], a_s[p + 1:]])
    I, J, LEN = overlaps(n, ns)
    if weights == "len":
        wgt = torch.as_tensor(LEN.astype(np.float64) / (float(n) * float(ns)), dtype=a.dtype)
    else:
        wgt = torch.full((len(LEN),), 1.0 / max(n, ns), dtype=a.dtype)
    diff = a_s[:, torch.as_tensor(I)] - b_s[:, torch.as_tensor(J)]
    total = (wgt[None, :] * diff * diff).sum()
    return total / ((2.0 if half else 1.0) * P)


def _sort_desc_ties(a):
    """ascending by value, equal values by DESCENDING row: the stable sort of the row-reversed matrix"""
    return torch.sort(torch.flip(a, dims=[1]), dim=1, stable=True)[0]


def signs_of(seed, t, n_proj, d, dtype=torch.float64):
    from nn import rand
    return torch.as_tensor(rand.sliced_signs(seed, t, n_proj, d), dtype=dtype)


def sliced(x, y, signs, dtype=torch.float64, **plant):
    """(loss, dloss/dy (n, d)) as float64 NumPy: x the style rows, y the prediction rows, computed in `dtype`"""
    xt = torch.as_tensor(np.asarray(x), dtype=dtype)
    yt = torch.as_tensor(np.asarray(y), dtype=dtype).requires_grad_(True)
    loss = sliced_loss(xt, yt, torch.as_tensor(np.asarray(signs), dtype=dtype), **plant)
    g, = torch.autograd.grad(loss, yt)
    return float(loss.detach().double()), g.double().numpy()


def err_over_max(got, ref):
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


def rel_fro(got, ref):
    return float(np.linalg.norm(np.asarray(got, np.float64) - ref) / max(np.linalg.norm(ref), 1e-300))


def min_gap(x, y, signs):
    """the smallest gap between sorted neighbours over all directions and both sides, in float64"""
    s = torch.as_tensor(np.asarray(signs), dtype=torch.float64)
    gaps = []
    for rows in (x, y):
        v = torch.sort(projections(torch.as_tensor(np.asarray(rows), dtype=torch.float64), s), dim=1)[0]
        if v.shape[1] > 1:
            gaps.append(float((v[:, 1:] - v[:, :-1]).min()))
    return min(gaps) if gaps else float("inf")


# ------------------------------------------------------------------ the step
TOL_SCALAR, GRAD_TOL = TR.TOL_SCALAR, TR.GRAD_TOL


def style_loss_sliced(target, prediction, alpha, signs):
    inv_alpha = 1 / max(alpha, 1)
    l_m = O.moment_matching(target, prediction)
    l_sw = sliced_loss(target, prediction, signs)
    l_pal = O.relaxed_emd(O.convert_rgb_to_yuv(target), O.convert_rgb_to_yuv(prediction), "both")
    return l_m + l_sw + inv_alpha * l_pal


def train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, n_proj, seed, t0=0):
    """_transport_ref.train_step with the sliced term: call number c (regions in order, within a region the styles of a blend
    in order) takes the directions of draw t0 + c, as the engine's device counter does"""
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_a = ls_a = 0.0
    r, c = len(indices_per_region), int(t0)
    for idx, style in zip(indices_per_region, styles_per_region):
        c_feat = O.sample_features(content_feat, idx, True)
        p_feat = O.sample_features(pred, idx, True)
        lc = O.content_loss(c_feat, p_feat)
        blend = style if isinstance(style, list) else [(1.0, style)]
        ls = 0.0
        for w, s in blend:
            ls = ls + w * style_loss_sliced(s, p_feat, alpha, signs_of(seed, c, n_proj, p_feat.shape[1], p_feat.dtype))
            c += 1
        loss = loss + (alpha * lc + ls) / loss_denom
        lc_a, ls_a = lc_a + lc, ls_a + ls
    loss = loss / r
    grads = torch.autograd.grad(loss, variables)
    return {"loss": loss.detach(), "loss_c": (lc_a / r).detach(), "loss_s": (ls_a / r).detach(), "grads": list(grads),
            "img": img.detach()}


def reference_step(P, n_proj, seed, dtype=torch.float64, blend_weights=None, vgg=None):
    """_transport_ref.reference_step with the sliced term"""
    net = O.VGG(P["weights"], dtype=dtype) if vgg is None else vgg
    plain = O.VGG(P["weights"], dtype=dtype)
    c, styles = P["content"].to(dtype), [s.to(dtype) for s in P["styles"]]
    with torch.no_grad():
        cf = [c] + plain(c)
        sfs = [[s] + plain(s) for s in styles]
        per_region = []
        for sets in P["s_idx"]:
            samples = [O.sample_features(sf, si, False) for sf, si in zip(sfs, sets)]
            per_region.append(samples[0] if blend_weights is None else list(zip(blend_weights, samples)))
    init = O.make_laplacian(c) + styles[0].mean(dim=(1, 2), keepdim=True)
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]
    out = train_step(variables, net, cf, per_region, P["idx"], P["alpha"], P["denom"], n_proj, seed)
    out["init"] = init
    return out
