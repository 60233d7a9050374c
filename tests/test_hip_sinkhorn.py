"""The three loss entries of the C ABI that tests/test_hip_loss_terms.py leaves out -- strotss_sinkhorn_cos_fwd_bwd,
strotss_sinkhorn_metric_fwd_bwd ('l2' / 'both') and strotss_rows_gemm_bwd (the backward of losses.cosine_distance /
l2_distance in both arguments) -- element by element against float64, with that file's harness (tests/_loss_harness.py):
a first call on a zero buffer, then NaN-filled workspaces, a seeded base in the gradient buffer, sentinels in its padding.

Sinkhorn: every case of tests/_sinkhorn_cases.py (n below COL_CHUNKS, n = 1, ns = 1, n = 64 and not a multiple of 64, ns
around 32 / 64 / 256, T = 1 / 2 / 64, duplicate rows, an l2 clamp that acts, every 1e-12 clamp acting, a row only v_0 = 1 keeps
off the clamp) against float64 autograd of oracle.strotss_oracle.sinkhorn_knopp: the loss within _sinkhorn_ref.loss_tolerance
relative, every gradient element within TOL_SK[family] of max|ref| (8 x the float32-CPU error of the same function, pinned by
tests/test_sinkhorn_cases_cpu.py).  The measured worst values are in DESIGN.md section 6."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import _sinkhorn_cases as SC
import _sinkhorn_ref as SR
from _loss_harness import DEV, LC_pad, SENTINEL, fbuf, report, run_entry

pytestmark = pytest.mark.gpu

EINVAL, EALIGN, ERANGE = -1, -2, -3
RUNS = SC.runs()
GSCALES = (1.0, 0.37)


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@functools.lru_cache(maxsize=None)
def ref64(label, metric):
    c = SC.make_case(label)
    return SR.sinkhorn(c.x, c.y, metric, SR.l_of(label, metric), c.T)


def entry(ops, c, metric, l, gs, T=None):
    """fn(gpred, loss4) calling the case's entry through nn._ops"""
    bx, by = fbuf(c.x), fbuf(c.y)
    T = c.T if T is None else T
    if metric == "cosine":
        rs = ops.row_inv_norm(bx, c.ns)
        return lambda gp, lo: ops.sinkhorn_cos_fwd_bwd(bx, rs, c.ns, by, c.n, c.d, l, T, gs, gp, lo[0])
    return lambda gp, lo: ops.sinkhorn_metric_fwd_bwd(bx, c.ns, by, c.n, c.d, metric, l, T, gs, gp, lo[0])


def check_loss(what, c, l, got, ref):
    rel = abs(got - ref) / max(abs(ref), 1e-30)
    report(f"scalar:{what}", c.label, f"{rel:.3e}")
    assert abs(got - ref) <= SR.loss_tolerance(c, l) * abs(ref), (what, got, ref)


def check_elements(what, label, got, ref, tol):
    err = SR.err_over_max(got, ref)
    report(f"grad:{what}", label, f"max {err:.3e} of tol {tol:.3e}")
    assert np.isfinite(got).all() and (np.abs(got - ref) <= tol * np.abs(ref).max()).all(), (what, err, tol)


@pytest.mark.parametrize("label,metric", RUNS, ids=[f"{a}-{m}" for a, m in RUNS])
def test_sinkhorn_entries(ops, label, metric):
    c = SC.make_case(label)
    l = SR.l_of(label, metric)
    ref_l, ref_g = ref64(label, metric)
    zero = label == "n50_ns40_d1" and metric == "cosine"          # one column: every cosine distance is 0, so is the gradient
    tol = SR.TOL_SK[SR.family(c, metric)]
    scale = max(np.abs(ref_g).max(), 1e-3 if zero else 0.0)
    losses = []
    for k, gs in enumerate(GSCALES):
        fn = entry(ops, c, metric, l, gs)
        got, loss, g0 = run_entry(ops, fn, c.n, c.d, scale * gs, 30 + k)
        what = f"sinkhorn_{metric}:g{gs}"
        if zero:
            report(f"grad:{what}", label, f"max|g| {np.abs(got).max():.3e}")
            assert abs(loss[0, 0]) <= 1e-6 and np.abs(got).max() <= 1e-6 and np.abs(g0).max() <= 1e-6
        else:
            check_loss(what, c, l, loss[0, 0], ref_l)
            check_elements(what, label, got / gs, ref_g, tol)
            check_elements(what + ":zero_base", label, g0.astype(np.float64) / gs, ref_g, tol)
        # a second identical call: the same bits
        g1 = torch.zeros((LC_pad(c.n), LC_pad(c.d)), dtype=torch.float32, device=DEV)
        l1 = torch.zeros(4, 4, dtype=torch.float32, device=DEV)
        fn(g1, l1)
        torch.cuda.synchronize()
        assert np.array_equal(g1[:c.n, :c.d].cpu().numpy(), g0) and not g1[c.n:].any() and not g1[:, c.d:].any()
        assert l1[0, 0].item() == loss[0, 0] and not l1.flatten()[1:].any()
        if c.kind == "dup":
            assert np.array_equal(g0[SC.DUP_ROWS[0]], g0[SC.DUP_ROWS[1]]), "duplicate prediction rows differ"
        losses.append(loss[0, 0])
    assert losses[0] == losses[1], "the loss depends on gscale"


@pytest.mark.parametrize("metric", SC.METRICS)
@pytest.mark.parametrize("label", SC.PUBLIC_LABELS)
def test_public_sinkhorn_knopp(label, metric):
    from nn import losses
    c = SC.make_case(label)
    l = SR.l_of(label, metric)
    ref_l, ref_g = ref64(label, metric)
    x = torch.as_tensor(c.x, dtype=torch.float32, device=DEV)
    y = torch.as_tensor(c.y, dtype=torch.float32, device=DEV).requires_grad_(True)
    out = losses.sinkhorn_knopp(x, y, metric, l, c.T)
    got, = torch.autograd.grad(out, y)
    torch.cuda.synchronize()
    check_loss(f"public_sinkhorn_{metric}", c, l, float(out.detach()), ref_l)
    check_elements(f"public_sinkhorn_{metric}", label, got.double().cpu().numpy(), ref_g, SR.TOL_SK[SR.family(c, metric)])
    if c.kind == "dup":
        assert torch.equal(got[SC.DUP_ROWS[0]], got[SC.DUP_ROWS[1]])


def test_sinkhorn_entries_refuse_on_real_buffers(ops):
    """every refusal happens before the first launch: gpred and loss_out keep their bits"""
    from nn import _hip
    lib = _hip.lib()
    c = SC.make_case("n65_ns31_T2")                       # d = 35: a row stride of 48 holds the rows and is no multiple of 32
    bx, by = fbuf(c.x), fbuf(c.y)
    rs = ops.row_inv_norm(bx, c.ns)
    by48 = torch.zeros((LC_pad(c.n), 48), dtype=torch.float32, device=DEV)
    by48[:c.n, :c.d] = by[:c.n, :c.d]
    g = torch.full((LC_pad(c.n), LC_pad(c.d)), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    nb = [lib.strotss_sinkhorn_workspace_bytes(c.ns, c.n, c.T), lib.strotss_sinkhorn_metric_workspace_bytes(c.ns, c.n, c.T)]
    ws = torch.zeros(max(nb) + 64, dtype=torch.uint8, device=DEV)
    p, f = _hip.ptr, C.c_float

    def cos(ns=c.ns, pred=by, ld=by.shape[1], l=10.0, T=c.T, nbytes=nb[0]):
        return lib.strotss_sinkhorn_cos_fwd_bwd(p(bx), p(rs), ns, p(pred), c.n, c.d, ld, f(l), T, f(1.0), p(g), p(loss), p(ws),
                                                nbytes, _hip.stream_ptr())

    def met(ns=c.ns, pred=by, ld=by.shape[1], l=10.0, T=c.T, nbytes=nb[1], metric=2):
        return lib.strotss_sinkhorn_metric_fwd_bwd(p(bx), ns, p(pred), c.n, c.d, ld, metric, f(l), T, f(1.0), p(g), p(loss),
                                                   p(ws), nbytes, _hip.stream_ptr())
    for fn in (cos, met):
        assert fn(T=0) == ERANGE and fn(T=65) == ERANGE
        assert fn(l=0.0) == ERANGE and fn(l=-1.0) == ERANGE
        assert fn(pred=by48, ld=48) == EALIGN
        assert fn(ns=0) == EINVAL
    assert met(metric=0) == EINVAL
    assert cos(nbytes=nb[0] - 1) == EINVAL and met(nbytes=nb[1] - 1) == EINVAL
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((loss == SENTINEL).all())
    assert cos() == 0 and met() == 0 and met(metric=1) == 0          # ... and the same arguments unspoiled are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool((loss[1:] == SENTINEL).all()) and float(loss[0]) != SENTINEL


# ------------------------------------------------------------------ strotss_rows_gemm_bwd
def _rows_gemm_call(ops, W, B, x, r, q, n, k, g, seed):
    """(added dx float64, base float64): dx seeded, its rows >= n hold the sentinel"""
    t = lambda a: torch.as_tensor(a, dtype=torch.float32, device=DEV).contiguous()
    ld = x.shape[1]
    dx = torch.full((LC_pad(n), ld), SENTINEL, dtype=torch.float32)
    dx[:n] = torch.as_tensor(np.random.default_rng(seed).standard_normal((n, ld)), dtype=torch.float32)
    dx = dx.to(DEV)
    base = dx.clone()
    ops.rows_gemm_bwd(t(W), k, t(B), t(x), t(r), t(q), n, g, dx)
    torch.cuda.synchronize()
    assert torch.equal(dx[n:], base[n:]), "rows >= n of dx changed"
    base64 = base[:n].double().cpu().numpy()
    return dx[:n].double().cpu().numpy() - base64, base64


@pytest.mark.parametrize("ld", SC.ROWS_GEMM_LD)
def test_rows_gemm_bwd_matches_its_formula(ops, ld):
    """dx += g r_i (sum_j W_ij B_j - x_i r_i q_i) with W's columns >= k zero, every element within the GEMM's f32 bound"""
    worst = 0.0
    for n in SC.ROWS_GEMM_N:
        for k in SC.ROWS_GEMM_K:
            W, B, x, r, q = SC.rows_gemm_problem(n, k, ld, 11)
            for g in SC.ROWS_GEMM_G:
                got, base = _rows_gemm_call(ops, W, B, x, r, q, n, k, g, 40)
                ref, bound = SR.rows_gemm(W, B, x, r, q, g, k, base)
                ratio = float((np.abs(got - ref) / bound).max())
                worst = max(worst, ratio)
                assert np.isfinite(got).all() and ratio <= 1.0, (n, k, ld, g, ratio)
    report("rows_gemm:err_over_bound", f"ld{ld}", f"{worst:.3e}")


def test_rows_gemm_bwd_sums_over_every_column_of_W(ops):
    """The header's contract: the product runs over all ldw columns of W and rows of B, and a caller that wants the sum over
    j < k zero-fills the rest.  With non-zero values there, the entry returns the sum over ldw -- and not the sum over k."""
    for n, k, ld in ((33, 33, 64), (65, 100, 32), (31, 1, 64)):
        W, B, x, r, q = SC.rows_gemm_problem(n, k, ld, 12, beyond_k=True)
        got, base = _rows_gemm_call(ops, W, B, x, r, q, n, k, 1.0, 41)
        ref, bound = SR.rows_gemm(W, B, x, r, q, 1.0, W.shape[1], base)
        assert (np.abs(got - ref) <= bound).all(), (n, k, ld)
        Wk = W.copy()
        Wk[:, k:] = 0.0
        ref_k, bound_k = SR.rows_gemm(Wk, B, x, r, q, 1.0, k, base)
        assert not (np.abs(got - ref_k) <= bound_k).all()
    from nn import _hip
    z = torch.zeros((64, 64), dtype=torch.float32, device=DEV)
    v = torch.zeros(64, dtype=torch.float32, device=DEV)
    call = lambda ldw, k, ld=64: _hip.lib().strotss_rows_gemm_bwd(_hip.ptr(z), ldw, k, _hip.ptr(z), _hip.ptr(z), _hip.ptr(v),
                                                                 _hip.ptr(v), 33, ld, C.c_float(1.0), _hip.ptr(z),
                                                                 _hip.stream_ptr())
    assert call(64, 65) == EINVAL and call(64, 0) == EINVAL and call(48, 33) == EALIGN and call(64, 33, 48) == EALIGN


# ------------------------------------------------------------------ the public distances, gradients to both sides
@pytest.mark.parametrize("kind", SC.PAIR_KINDS)
@pytest.mark.parametrize("label", SC.PAIR_LABELS)
def test_public_distances_differentiate_both_arguments(label, kind):
    from nn import losses
    x, y, G = SC.make_pair(label)
    rx, ry = SR.pair_grads(x, y, G, kind)
    xt = torch.as_tensor(x, dtype=torch.float32, device=DEV).requires_grad_(True)
    yt = torch.as_tensor(y, dtype=torch.float32, device=DEV).requires_grad_(True)
    out = (losses.dist_metrics[kind](xt, yt) * torch.as_tensor(G, dtype=torch.float32, device=DEV)).sum()
    gx, gy = torch.autograd.grad(out, (xt, yt))
    torch.cuda.synchronize()
    tol = SR.TOL_PAIR[SR.pair_family(x.shape[1], kind)]
    check_elements(f"{kind}:dx", label, gx.double().cpu().numpy(), rx, tol)
    check_elements(f"{kind}:dy", label, gy.double().cpu().numpy(), ry, tol)
