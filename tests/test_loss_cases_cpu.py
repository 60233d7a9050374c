"""CPU checks of the loss cases (tests/_loss_cases.py) and of the float64 flip-aware reference (tests/_loss_ref.py) that
tests/test_hip_loss_terms.py holds the HIP loss entries to: the reference equals numpy_ref and float64 autograd of the
oracle where no entry is ambiguous, its bound covers every sign of the ambiguous entries, every case meets its
conditioning, and the comparison function catches planted errors."""
import itertools

import numpy as np
import pytest
import torch

import _loss_cases as LC
import _loss_ref as LR
from oracle import numpy_ref as NR
from oracle import strotss_oracle as O


def _small(n, ns, d, seed):
    rng = np.random.default_rng(seed)
    return LC.hyper_rows(rng, ns, d), LC.hyper_rows(rng, n, d), LC.hyper_rows(rng, n, d)


def _autograd(fn, *args):
    t = [torch.from_numpy(a) for a in args]
    t[-1].requires_grad_(True)
    out = fn(*t)
    g, = torch.autograd.grad(out, t[-1])
    return float(out), g.numpy()


def _rel(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


def test_reference_equals_numpy_ref_and_float64_autograd():
    x, y, c = _small(48, 64, 35, 7)
    gx, gy = np.arange(64), np.arange(48)
    l, g, b, namb = LR.selfsim(y, c)
    assert namb == 0
    ln, gn = NR.self_similarity_fwd_bwd(y, c)
    la, ga = _autograd(lambda cc, yy: O.self_similarity(yy, cc), c, y)
    assert abs(l - ln) < 1e-12 and abs(l - la) < 1e-12
    assert _rel(g, gn) < 1e-9 and _rel(g, ga) < 1e-9        # the diagonal's sign reaches the gradient only as rounding
    w = np.random.default_rng(3).random(48)
    lw, gw, _, _ = LR.selfsim(y, c, weight=w)
    wt = torch.from_numpy(w)
    law, gaw = _autograd(lambda cc, yy: ((O.cosine_distance(yy, yy) / torch.clamp(O.cosine_distance(yy, yy).sum(0), min=1e-12)
                                          - O.cosine_distance(cc, cc) / torch.clamp(O.cosine_distance(cc, cc).sum(0), min=1e-12))
                                         .abs() * wt[None, :]).sum() / 48, c, y)
    assert abs(lw - law) < 1e-12 and _rel(gw, gaw) < 1e-9
    l, g, b, namb = LR.moment(x, y)
    assert namb == 0
    ln, gn = NR.moment_matching_fwd_bwd(x, y)
    la, ga = _autograd(O.moment_matching, x, y)
    assert abs(l - ln) < 1e-12 and abs(l - la) < 1e-12 and _rel(g, gn) < 1e-9 and _rel(g, ga) < 1e-9
    for metric in ("cos", "l2", "both"):
        l, g, _, _ = LR.remd(x, y, gx, gy, metric)
        la, ga = _autograd(lambda xx, yy: O.relaxed_emd(xx, yy, "cosine" if metric == "cos" else metric), x, y)
        assert abs(l - la) < 1e-12 and _rel(g, ga) < 1e-9, metric
        if metric == "cos":
            ln, gn = NR.relaxed_emd_cos_fwd_bwd(x, y)
            assert abs(l - ln) < 1e-12 and _rel(g, gn) < 1e-9
    l, g, _, _ = LR.palette(x, y, gx, gy, True)
    ln, gn = NR.palette_remd_fwd_bwd(x[:, :3], y[:, :3])
    assert abs(l - ln) < 1e-12 and _rel(g, gn) < 1e-9
    l, g, _, _ = LR.palette(x, y, gx, gy, False)
    la, ga = _autograd(lambda xx, yy: O.relaxed_emd(xx[:, :3], yy[:, :3], "both"), x, y)
    assert abs(l - la) < 1e-12 and _rel(g, ga[:, :3]) < 1e-9


def test_bound_covers_every_sign_of_the_ambiguous_entries(monkeypatch):
    x, y, c = _small(7, 9, 10, 11)
    # a stated error large enough to make a handful of entries ambiguous
    amb = LR.selfsim_ambiguous(y, c, eps_cost=4e-3)
    off = amb & ~np.eye(7, dtype=bool)
    assert 2 <= off.sum() <= 10, off.sum()
    l, ref, bound, namb = LR.selfsim(y, c, eps_cost=4e-3)
    assert namb == off.sum() and bound.max() > 0
    pos = np.argwhere(amb)
    for signs in itertools.product((-1.0, 1.0), repeat=len(pos)):
        S = np.zeros(amb.shape)
        S[tuple(pos.T)] = signs
        _, g, _, _ = LR.selfsim(y, c, eps_cost=4e-3, signs=S)
        assert (np.abs(g - ref) <= bound * (1 + 1e-12) + 1e-300).all()
    monkeypatch.setattr(LR, "COV_K", 1e5)
    xm, ym = x[:, :6], y[:, :6]
    l, ref, bound, namb = LR.moment(xm, ym)
    mx, Sx = LR.moment_stats(xm); my, Sy = LR.moment_stats(ym)
    tcx, tmx = LR.cov_tau(xm); tcy, tmy = LR.cov_tau(ym)
    amb, ambm = np.abs(Sy - Sx) < tcx + tcy, np.abs(my - mx) < tmx + tmy
    assert 2 <= amb.sum() + ambm.sum() <= 12, (amb.sum(), ambm.sum())
    pos, posm = np.argwhere(amb), np.flatnonzero(ambm)
    for signs in itertools.product((-1.0, 1.0), repeat=len(pos) + len(posm)):
        T = np.zeros(amb.shape)
        T[tuple(pos.T)] = signs[:len(pos)]
        Tm = np.zeros(ambm.shape)
        Tm[posm] = signs[len(pos):]
        _, g, _, _ = LR.moment(xm, ym, signs=T, signs_mean=Tm)
        assert (np.abs(g - ref) <= bound * (1 + 1e-12) + 1e-300).all()


@pytest.mark.parametrize("label", LC.LABELS)
def test_case_meets_its_conditioning(label):
    c = LC.make_case(label)
    assert c.x.shape == (c.ns, c.d) and c.y.shape == (c.n, c.d) and c.c.shape == (c.n, c.d)
    for v in (c.x, c.y, c.c):
        assert (v >= 0).all() and (v[:, :3] <= 1).all()
    costs = LC.cost_matrices(c.x, c.y, c.d)
    for m in LC.METRICS:
        assert LC.conditioned(costs[m], c.gx, c.gy), m
    for g, v in ((c.gx, c.x), (c.gy, c.y)):          # a duplicate group's rows are identical
        for k in np.unique(g):
            assert (v[g == k] == v[k]).all()
    if c.kind == "flat_style":
        assert np.bincount(c.gx).max() >= LC.FLAT_STYLE_ROWS
        # one list holds them all: some prediction row is the minimum of every row of the group (row branch) or some
        # column's minimum is the group (column branch)
        C = costs["cos"]
        assert np.bincount(c.gx)[c.gx[C.argmin(0)]].max() >= LC.FLAT_STYLE_ROWS or \
            np.bincount(C.argmin(1)[c.gx == np.bincount(c.gx).argmax()]).max() >= LC.FLAT_STYLE_ROWS
    if c.kind == "flat_pred":
        assert np.bincount(c.gy).max() >= LC.FLAT_PRED_ROWS
    if c.kind == "regime":
        assert all(0.6 <= (v[:, 3:] == 0).mean() <= 0.9 and (v[:, 3:].max(0) == 0).mean() >= 0.05 for v in (c.x, c.y, c.c))
    if c.kind == "exact_rows":
        assert (LR.cos_dist(c.y, c.y).diagonal() == 0).all() and (LR.cos_dist(c.c, c.c) == 0).all()


def test_cases_take_both_branches_and_reach_the_edges():
    rows = {m: set() for m in LC.METRICS}
    for c in LC.all_cases():
        costs = LC.cost_matrices(c.x, c.y, c.d)
        for m in LC.METRICS:
            rows[m].add(LC.branch_gap(costs[m]) >= 0)
    for m in LC.METRICS:
        assert rows[m] == {True, False}, m
    shapes = {(c.n, c.ns, c.d) for c in LC.all_cases()}
    assert {(1024, 1024, 2179), (1024, 2048, 2179), (1, 64, 2179), (2, 64, 2179), (37, 1500, 2179), (200, 300, 3100)} <= shapes
    assert any(c.n % 32 and c.ns % 64 for c in LC.all_cases())


@pytest.mark.parametrize("k", [4])
def test_blend_styles_are_conditioned(k):
    base = LC.make_case("step")
    for (x, gx), ns in zip(LC.blend_styles(k), LC.BLEND_NS):
        assert x.shape == (ns, base.d)
        costs = LC.cost_matrices(x, base.y, base.d)
        for m in ("cos", "palette_yuv"):
            assert LC.conditioned(costs[m], gx, base.gy), m


@pytest.mark.parametrize("label", [l for l in LC.LABELS])
def test_ambiguous_entries_are_rare(label):
    """the flip bounds cannot swallow the check: at most 1e-4 of the off-diagonal self-similarity entries (or one entry)
    and at most 2e-4 of the moment entries (symmetric pairs counted twice) are ambiguous"""
    c = LC.make_case(label)
    amb = LR.selfsim_ambiguous(c.y, c.c)
    off = int(amb.sum() - np.diag(amb).sum())
    assert off <= max(1e-4 * c.n * c.n, 1), off
    _, _, _, namb = LR.moment(c.x, c.y)
    assert namb <= 2e-4 * (c.d * c.d + c.d), namb


# ------------------------------------------------------------------ negative controls: check_grad must catch each
def _fails(got, ref, bound=None):
    ok, worst, _ = LR.check_grad(got, ref, bound, LR.TOL_GRAD)
    return not ok and worst > LR.TOL_GRAD


def test_negative_control_palette_row_scaled():
    c = LC.make_case("small_region_n37")
    _, g, _, b = LR.palette(c.x, c.y, c.gx, c.gy, True)
    assert LR.check_grad(g, g, None, LR.TOL_GRAD)[0]
    bad = g.copy()
    r = np.abs(g).max(1).argmax()
    bad[r] *= 1.001
    assert _fails(bad, g, b)


def test_negative_control_zeroed_chunk():
    c = LC.make_case("small_region_n37")
    _, g, _, _ = LR.remd(c.x, c.y, c.gx, c.gy, "cos")
    bad = g.copy()
    r, k = np.unravel_index(np.abs(g).argmax(), g.shape)
    bad[r, k // 64 * 64:k // 64 * 64 + 64] = 0.0
    assert _fails(bad, g)


def test_negative_control_branch_swapped():
    c = LC.make_case("step")
    _, g, row, _ = LR.remd(c.x, c.y, c.gx, c.gy, "cos")
    _, bad, _, _ = LR.remd(c.x, c.y, c.gx, c.gy, "cos", branch="col" if row else "row")
    assert _fails(bad, g)


def test_negative_control_tie_to_its_first_member():
    c = LC.make_case("flat_pred_600_of_1024")
    # the row branch, where the ties among the 600 identical prediction rows carry the gradient
    _, g, row, _ = LR.remd(c.x, c.y, c.gx, c.gy, "cos", branch="row")
    _, bad, _, _ = LR.remd(c.x, c.y, c.gx, c.gy, "cos", branch="row", tie="first")
    assert _fails(bad, g)


def test_negative_control_one_certain_sign_flipped():
    c = LC.make_case("small_region_n37")
    l, g, bound, _ = LR.selfsim(c.y, c.c)
    Dx, sxr, sx, A, B, tau = LR._selfsim_parts(c.y, c.c, LR.EPS_COST)
    amb = np.abs(A - B) < tau
    S = np.where(amb, 0.0, np.sign(A - B))
    i, j = np.argwhere(~amb & ~np.eye(c.n, dtype=bool))[0]
    S[i, j] = -S[i, j]
    bad = LR._selfsim_chain(c.y, Dx, sxr, sx, A, S / c.n)
    assert _fails(bad, g, bound)
