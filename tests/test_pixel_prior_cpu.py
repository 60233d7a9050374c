"""CPU-only checks of the pixel-space priors: the float64 restatement's gradients against
torch.autograd through an independent statement of both terms (pooling by padded reshape, the grid Laplacian as the
Kronecker sum of two path Laplacians), five planted errors that the comparison must catch, the float32 yardstick ERR32, the
step restatement's float32 run against the step bounds, and the command line: the three flags parse and every refusal is
raised before a file is opened."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_prior_cases as PC  # noqa: E402
import _pixel_prior_ref as PR  # noqa: E402

AUTOGRAD_TOL = 1e-10


def path_laplacian(n):
    L = torch.zeros((n, n), dtype=torch.float64)
    for k in range(n - 1):
        L[k, k] += 1; L[k + 1, k + 1] += 1
        L[k, k + 1] -= 1; L[k + 1, k] -= 1
    return L


def pool_t(u, p):
    h, w, ch = u.shape
    hp, wp = PR.grid(h, w, p)
    pad = torch.zeros((hp * p, wp * p, ch), dtype=u.dtype)
    pad[:h, :w] = u
    s = pad.reshape(hp, p, wp, p, ch).sum(dim=(1, 3))
    return s / torch.from_numpy(PR.counts(h, w, p)).to(u.dtype)[:, :, None]


def detail_t(x, c, pools, weights):
    """[L_p] as torch scalars of x"""
    h, w, _ = x.shape
    out = []
    for p, m in zip(pools, weights):
        hp, wp = PR.grid(h, w, p)
        u = pool_t(x, p) - pool_t(c, p)
        D = torch.einsum("ik,kjc->ijc", path_laplacian(hp), u) + torch.einsum("jk,ikc->ijc", path_laplacian(wp), u)
        mm = torch.ones((hp, wp), dtype=x.dtype) if m is None else torch.from_numpy(m).to(x.dtype)
        out.append((mm[:, :, None] * D * D).sum() / (3 * hp * wp))
    return out


def tv_t(x, eps=PR.TV_EPS):
    h, w, _ = x.shape
    dx = torch.cat([x[:, 1:] - x[:, :-1], torch.zeros((h, 1, 3), dtype=x.dtype)], dim=1)
    dy = torch.cat([x[1:] - x[:-1], torch.zeros((1, w, 3), dtype=x.dtype)], dim=0)
    return (torch.sqrt(dx * dx + dy * dy + eps * eps) - eps).sum() / (3 * h * w)


def detail_autograd(label):
    P = PC.detail_inputs(label)
    x = torch.from_numpy(P["x"].astype(np.float64)).requires_grad_(True)
    terms = detail_t(x, torch.from_numpy(P["c"].astype(np.float64)), P["pools"], P["weights"])
    total = sum(terms)
    g = torch.autograd.grad(total, x)[0] if total.requires_grad and total.grad_fn is not None else torch.zeros_like(x)
    return [float(t.detach()) for t in terms], g.numpy()


def detail_distance(label, plant=None):
    """(worst loss distance, gradient distance) of the restatement, with or without a planted error, from autograd, relative
    to max(1, max|autograd|)"""
    P = PC.detail_inputs(label)
    ref_l, ref_g = detail_autograd(label)
    got_l, got_g = PR.detail(P["x"], P["c"], P["pools"], P["weights"], plant=plant)
    dl = max(abs(float(a) - b) for a, b in zip(got_l, ref_l))
    return dl, float(np.abs(got_g - ref_g).max()) / max(1.0, float(np.abs(ref_g).max()))


def tv_distance(label, plant=None):
    P = PC.tv_inputs(label)
    x = torch.from_numpy(P["x"].astype(np.float64)).requires_grad_(True)
    ref_t = tv_t(x)
    ref_g = torch.autograd.grad(ref_t, x)[0].numpy()
    ref_l = float(ref_t.detach())
    got_l, got_g = PR.tv(P["x"], plant=plant)
    return abs(float(got_l) - float(ref_l)), float(np.abs(got_g - ref_g).max()) / max(1.0, float(np.abs(ref_g).max()))


# ------------------------------------------------------------------ 1. the restatement against autograd
@pytest.mark.parametrize("label", PC.DETAIL_LABELS)
def test_detail_restatement_matches_autograd(label):
    dl, dg = detail_distance(label)
    print(f"MEASURE detail autograd {label}: loss {dl:.3e} gradient {dg:.3e}")
    assert dl <= AUTOGRAD_TOL and dg <= AUTOGRAD_TOL


@pytest.mark.parametrize("label", PC.TV_LABELS)
def test_tv_restatement_matches_autograd(label):
    dl, dg = tv_distance(label)
    print(f"MEASURE tv autograd {label}: loss {dl:.3e} gradient {dg:.3e}")
    assert dl <= AUTOGRAD_TOL and dg <= AUTOGRAD_TOL


def test_graph_laplacian_is_symmetric_and_kills_constants():
    rng = np.random.default_rng(0)
    u, v = rng.random((5, 7, 3)), rng.random((5, 7, 3))
    assert abs(float((PR.laplacian(u) * v).sum() - (u * PR.laplacian(v)).sum())) < 1e-12
    assert float(np.abs(PR.laplacian(np.ones((5, 7, 3)))).max()) == 0.0
    # pooling: every cell the mean of what it covers, partial cells included
    a = rng.random((5, 7, 1))
    assert abs(float(PR.pool(a, 4)[1, 1, 0]) - float(a[4:, 4:].mean())) < 1e-15
    assert np.array_equal(PR.pool(a, 1), a)


# ------------------------------------------------------------------ 2. planted errors
PLANTED = {                      # planted error -> the case that must catch it
    "no_cnt": ("detail", "5x7-p2-absent"),               # ragged cells on both edges
    "zero_pad": ("detail", "1x5-p1-absent"),
    "weight_after": ("detail", "42x63-p1_4-random"),
    "no_factor2": ("detail", "2x3-p1_2-random"),
    "tv_wrap": ("tv", "1x5"),
}


@pytest.mark.parametrize("plant", PR.PLANTS)
def test_planted_errors_fail_the_comparison(plant):
    kind, label = PLANTED[plant]
    dl, dg = (detail_distance if kind == "detail" else tv_distance)(label, plant)
    print(f"MEASURE planted {plant} on {label}: loss {dl:.3e} gradient {dg:.3e}")
    assert dg > 1e3 * AUTOGRAD_TOL, (plant, label, dg)
    clean = (detail_distance if kind == "detail" else tv_distance)(label)
    assert max(clean) <= AUTOGRAD_TOL


def test_tv_wrap_is_also_caught_on_a_column():
    assert tv_distance("5x1", "tv_wrap")[1] > 1e3 * AUTOGRAD_TOL


# ------------------------------------------------------------------ 3. the float32 yardstick
def test_float32_restatement_error_is_the_pinned_one():
    worst = {"detail": 0.0, "detail16": 0.0, "tv": 0.0}
    for label in PC.DETAIL_LABELS:
        P = PC.detail_inputs(label)
        l64, g64 = PR.detail(P["x"], P["c"], P["pools"], P["weights"])
        l32, g32 = PR.detail(P["x"], P["c"], P["pools"], P["weights"], dtype=np.float32)
        e = PR.err32(g32, g64)
        rel = max((abs(float(a) - float(b)) / abs(float(b)) for a, b in zip(l32, l64) if float(b) != 0), default=0.0)
        print(f"MEASURE err32 detail {label} {e:.3e} loss {rel:.3e}")
        assert g32.dtype == np.float32 and rel <= PR.LOSS_TOL / 4
        fam = PR.family(P["pools"])
        worst[fam] = max(worst[fam], e)
    for label in PC.TV_LABELS:
        P = PC.tv_inputs(label)
        l64, g64 = PR.tv(P["x"])
        l32, g32 = PR.tv(P["x"], dtype=np.float32)
        e = PR.err32(g32, g64)
        rel = abs(float(l32) - float(l64)) / abs(float(l64)) if float(l64) != 0 else abs(float(l32))
        print(f"MEASURE err32 tv {label} {e:.3e} loss {rel:.3e}")
        assert g32.dtype == np.float32 and rel <= PR.LOSS_TOL / 4
        worst["tv"] = max(worst["tv"], e)
    print("MEASURE err32 worst", worst)
    for fam, e in worst.items():
        assert PR.ERR32[fam] / 4 <= e <= 2.0 * PR.ERR32[fam], (fam, e)
        assert PR.TOL_GRAD[fam] == 8.0 * PR.ERR32[fam]


def test_exact_inputs_give_exact_zeros_in_float32():
    """what the library is held to bit for bit: x a copy of c -> every D_p and the gradient exactly 0; a constant image ->
    L_tv and its gradient exactly 0 (the (dx^2 + dy^2) / (n + eps) form has no sqrt(eps^2) - eps left over)"""
    P = PC.detail_inputs("42x63-p1_4-random")
    l, g = PR.detail(P["c"], P["c"], P["pools"], P["weights"], dtype=np.float32)
    assert all(float(v) == 0.0 for v in l) and not g.any()
    lt, gt = PR.tv(np.full((5, 7, 3), 0.3, dtype=np.float32), dtype=np.float32)
    assert float(lt) == 0.0 and not gt.any()


# ------------------------------------------------------------------ 4. the step restatement's own float32 run
def test_step_restatement_float32_run_stays_within_a_quarter_of_the_step_bounds():
    import _pixel_prior_step as PS
    for lb in PS.LABELS:
        ref = PS.reference_step(lb)
        f32 = PS.reference_step(lb, dtype=torch.float32)
        sc, gr = PS.step_distance(f32, ref)
        d_share = PS.DETAIL_WEIGHT * ref["loss_detail"] / float(ref["loss"])
        t_share = PS.TV_WEIGHT * ref["loss_tv"] / float(ref["loss"])
        print(f"MEASURE step32 {lb}: scalars {sc:.3e} gradient {gr:.3e}; shares of the loss: detail {d_share:.3f} tv {t_share:.3f}")
        assert sc <= PS.TOL_SCALAR / 4 and gr <= PS.GRAD_TOL / 4, (lb, sc, gr)
        assert d_share > 0.05 and t_share > 0.05, (lb, d_share, t_share)


# ------------------------------------------------------------------ 5. the command line
def _args(*extra):
    import run_strotss as RS
    return RS.build_parser().parse_args(["no_such_content.jpg", "no_such_style.jpg"] + list(extra))


def test_parser_accepts_the_three_flags():
    import run_strotss as RS
    a = _args("--detail_weight", "2.5", "--detail_pool", "1", "2", "8", "--tv_weight", "0.5")
    assert a.detail_weight == 2.5 and a.detail_pool == [1, 2, 8] and a.tv_weight == 0.5
    assert RS._pixel_prior_input(a) == dict(detail=(2.5, [1, 2, 8]), tv=0.5)
    a = _args()
    assert a.detail_weight is None and a.detail_pool is None and a.tv_weight is None
    assert RS._pixel_prior_input(a) == dict(detail=None, tv=0.0)
    assert RS._pixel_prior_input(_args("--detail_weight", "1"))["detail"] == (1.0, list(RS.DEFAULT_DETAIL_POOLS)) == (1.0, [1, 4])
    assert [names[0] for names, _ in RS._FLAGS[-3:]] == ["--detail_weight", "--detail_pool", "--tv_weight"]


REFUSED = [
    ("--detail_weight", "-1"), ("--detail_weight", "nan"), ("--detail_weight", "inf"),
    ("--tv_weight", "-0.5"), ("--tv_weight", "nan"),
    ("--detail_pool", "1", "4"),                                   # needs --detail_weight
    ("--detail_weight", "1", "--detail_pool", "3"), ("--detail_weight", "1", "--detail_pool", "4", "1"),
    ("--detail_weight", "1", "--detail_pool", "2", "2"), ("--detail_weight", "1", "--detail_pool", "1", "2", "4", "8"),
    ("--detail_weight", "1", "--strips"), ("--tv_weight", "1", "--strips"),
]


@pytest.mark.parametrize("extra", REFUSED, ids=[" ".join(e) for e in REFUSED])
def test_refusals_come_before_any_file_is_opened(extra):
    """the content and style paths do not exist: a ValueError (not a FileNotFoundError) shows the order"""
    import run_strotss as RS
    with pytest.raises(ValueError):
        RS.run(_args(*extra))


@pytest.mark.parametrize("extra", [("--detail_weight", "1"), ("--tv_weight", "1"), ("--tv_weight", "1", "--video")])
def test_refused_under_torchrun_with_several_ranks(extra, monkeypatch):
    import run_strotss as RS
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(_args(*extra))


def test_engine_keywords_and_pool_check():
    from nn import _hip, _ops, engine
    assert _ops.TV_EPS == PR.TV_EPS == 1.0 / 255.0
    assert _hip.DETAIL_POOLS == (1, 2, 4, 8, 16) and _hip.MAX_DETAIL_POOLS == 3
    assert _ops.check_detail_pools((1, 4)) == [1, 4]
    for bad in ([], [3], [4, 1], [1, 1], [1, 2, 4, 8], [True], "14", None):
        with pytest.raises(ValueError):
            _ops.check_detail_pools(bad)
    t = engine.DetailTarget(torch.zeros(4, 4, 3), (1, 4), 2.0)
    assert t.cell_map is None and t.weight == 2.0
