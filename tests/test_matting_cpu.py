"""The photorealism term without a GPU: the two float64 statements of tests/_matting_ref.py against each
other, the dense matting Laplacian's properties, the gradient against torch.autograd through an independent torch
statement, planted errors that must fail on named cases, the float32 yardstick, the step restatement's own float32 run, the
status codes of refused C calls, and the command line's refusals."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _matting_cases as MC  # noqa: E402
import _matting_ref as MR  # noqa: E402
import _smooth_ref as SR  # noqa: E402

STATEMENT_TOL = 1e-10


# ------------------------------------------------------------------ 1. the two statements, and L itself
@pytest.mark.parametrize("label", MC.DENSE_LABELS)
def test_dense_laplacian_equals_count_times_residual(label):
    P = MC.inputs(label)
    ld, gd = MR.value_grad_dense(P["p"], P["I"], P["r"], P["eps"])
    assert abs(ld - P["loss"]) <= STATEMENT_TOL and float(np.abs(gd - P["grad"]).max()) <= STATEMENT_TOL
    assert P["loss"] >= -STATEMENT_TOL


@pytest.mark.parametrize("label", ["1x1-r1-eps0.0001-random", "1x3-r4-eps0.0001-random", "5x7-r2-eps0.01-random",
                                   "9x12-r1-eps0.0001-random", "9x12-r4-eps1-random", "9x12-r2-eps0.0001-constant_guide"])
def test_laplacian_is_symmetric_kills_constants_and_is_positive_semidefinite(label):
    P = MC.inputs(label)
    L = MR.dense_laplacian(P["I"], P["r"], P["eps"])
    norm = max(float(np.abs(L).max()), 1e-300)
    assert float(np.abs(L - L.T).max()) <= STATEMENT_TOL * norm
    assert float(np.abs(L @ np.ones(len(L))).max()) <= STATEMENT_TOL * max(norm, 1.0)
    assert float(np.linalg.eigvalsh((L + L.T) / 2).min()) >= -STATEMENT_TOL * max(norm, 1.0)


def test_affine_images_cost_only_the_eps_shrinkage_and_colour_shifts_are_free():
    P = MC.inputs("9x12-r1-eps0.0001-affine")
    rnd = MC.inputs("9x12-r1-eps0.0001-random")
    assert 0 <= P["loss"] < 0.05 * rnd["loss"]
    l0, g0 = MR.value_grad(rnd["p"], rnd["I"], 1, 1e-4)
    l1, g1 = MR.value_grad(rnd["p"].astype(np.float64) + np.array([0.3, -0.2, 0.1]), rnd["I"], 1, 1e-4)
    assert abs(l0 - l1) <= STATEMENT_TOL and float(np.abs(g0 - g1).max()) <= STATEMENT_TOL


def _torch_loss(p, I, r, eps):
    """an independent statement in torch float64: zero-padded box sums by convolution, uncentred moments, a library solve"""
    h, w = p.shape[:2]
    box = lambda x: torch.nn.functional.conv2d(x.permute(2, 0, 1)[:, None], torch.ones(1, 1, 2 * r + 1, 2 * r + 1, dtype=x.dtype),
                                               padding=r)[:, 0].permute(1, 2, 0)
    n = box(torch.ones(h, w, 1, dtype=p.dtype))
    mean = lambda x: box(x) / n
    mu, pbar = mean(I), mean(p)
    sigma = mean((I[..., :, None] * I[..., None, :]).reshape(h, w, 9)).reshape(h, w, 3, 3) - mu[..., :, None] * mu[..., None, :] \
        + SR.eps32(eps) * torch.eye(3, dtype=p.dtype)
    cov = mean((I[..., :, None] * p[..., None, :]).reshape(h, w, 9)).reshape(h, w, 3, 3) - mu[..., :, None] * pbar[..., None, :]
    a = torch.linalg.solve(sigma, cov)                                  # [j, c]
    b = pbar - (a * mu[..., :, None]).sum(-2)
    abar, bbar = mean(a.reshape(h, w, 9)).reshape(h, w, 3, 3), mean(b)
    q = (abar * I[..., :, None]).sum(-2) + bbar
    return (n * p * (p - q)).sum() / (3.0 * h * w)


@pytest.mark.parametrize("label", ["1x3-r1-eps0.0001-random", "5x7-r4-eps0.01-random", "9x12-r2-eps0.0001-random",
                                   "17x33-r1-eps0.0001-random", "17x33-r4-eps1-random", "9x12-r1-eps0.0001-affine"])
def test_gradient_equals_autograd_through_an_independent_statement(label):
    P = MC.inputs(label)
    p = torch.from_numpy(P["p"].astype(np.float64)).requires_grad_(True)
    loss = _torch_loss(p, torch.from_numpy(P["I"].astype(np.float64)), P["r"], P["eps"])
    (g,) = torch.autograd.grad(loss, p)
    assert abs(float(loss.detach()) - P["loss"]) <= STATEMENT_TOL
    assert float(np.abs(g.numpy() - P["grad"]).max()) <= STATEMENT_TOL


# ------------------------------------------------------------------ 2. planted errors must fail, each on a named case
PLANTED = {
    "unclipped_n": "5x7-r2-eps0.01-random",
    "eps_times_n": "9x12-r1-eps0.01-random",
    "no_factor_2": "9x12-r1-eps0.0001-random",
    "one_stage": "9x12-r2-eps0.0001-random",
    "shifted_window": "16x16-r1-eps0.0001-random",
}


def _planted_distance(label, bug):
    P = MC.inputs(label)
    l, g = MR.value_grad_planted(P["p"], P["I"], P["r"], P["eps"], bug)
    return abs(l - P["loss"]) / P["scale"], float(np.abs(g - P["grad"]).max()) / float(np.abs(P["grad"]).max())


@pytest.mark.parametrize("bug", list(PLANTED))
def test_planted_errors_fail_the_comparison(bug):
    label = PLANTED[bug]
    dl, dg = _planted_distance(label, bug)
    bound = 8 * MR.ERR32[MC.BY_LABEL[label][3]][0]
    print(f"MEASURE planted {bug} on {label}: loss {dl:.3e} gradient {dg:.3e} (the GPU test's bound {bound:.1e})")
    assert dg > 100 * bound, (bug, label, dg)
    assert max(_planted_distance(label, None)) <= STATEMENT_TOL


# ------------------------------------------------------------------ 3. the float32 yardstick
def test_float32_restatement_stays_within_the_pinned_errors():
    worst = {eps: [0.0, 0.0] for eps in MR.ERR32}
    for label in MC.LABELS:
        eg, el = MC.float32_errors(label)
        eps = MC.BY_LABEL[label][3]
        assert eg <= MR.ERR32[eps][0] and el <= MR.ERR32[eps][1], (label, eg, el)
        worst[eps] = [max(worst[eps][0], eg), max(worst[eps][1], el)]
    print("MEASURE err32 worst", worst)
    for eps, (eg, el) in worst.items():                # pinned at the run's own worst, not above it
        assert eg >= MR.ERR32[eps][0] / 2 and el >= MR.ERR32[eps][1] / 2, (eps, eg, el)


def test_float32_run_of_a_single_pixel_is_exactly_zero():
    P = MC.inputs("1x1-r4-eps0.0001-random")
    l, g = MR.matting_float32(P["p"], P["I"], 4, 1e-4)
    assert l == 0.0 and not g.any() and P["loss"] == 0.0 and not P["grad"].any()


def test_step_restatement_float32_run_stays_within_a_quarter_of_the_step_bounds():
    import _matting_step as MS
    for lb in MS.LABELS:
        ref = MS.reference_step(lb)
        f32 = MS.reference_step(lb, dtype=torch.float32)
        sc, gr = MS.step_distance(lb, f32, ref)
        share = MS.photo_share(lb, ref)
        print(f"MEASURE step32 {lb}: scalars {sc:.3e} gradient {gr:.3e}; the photo term's share of the loss {share:.3f}")
        assert sc <= MS.TOL_SCALAR / 4 and gr <= MS.GRAD_TOL / 4, (lb, sc, gr)
        assert 0.10 <= share <= 0.30, (lb, share)


# ------------------------------------------------------------------ 4. the C entries' refusals (nothing is launched)
EINVAL, EALIGN, ERANGE = -1, -2, -3
B = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)
NULL = None


@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_abi_version_and_sizes(lib):
    from nn import _hip
    assert lib.strotss_abi_version() == 8 and _hip.MATTING_MAX_RADIUS == MR.MAX_RADIUS == 4
    assert lib.strotss_matting_stats_bytes(5, 7) == 36 * 35
    assert lib.strotss_matting_workspace_bytes(16, 16) == 32 and lib.strotss_matting_workspace_bytes(17, 33) == 16 + 32
    for h, w in ((0, 5), (5, -1), (1 << 15, 1 << 15)):
        assert lib.strotss_matting_stats_bytes(h, w) == lib.strotss_matting_workspace_bytes(h, w) == 0


def test_matting_prepare_refusals(lib):
    f = C.c_float
    call = lambda guide=B, h=8, w=12, r=1, eps=1e-4, stats=B: lib.strotss_matting_prepare(guide, h, w, r, f(eps), stats, NULL)
    for kw in (dict(guide=NULL), dict(stats=NULL), dict(h=0), dict(w=-1), dict(h=1 << 15, w=1 << 15)):
        assert call(**kw) == EINVAL, kw
    for kw in (dict(r=0), dict(r=5), dict(r=-1), dict(eps=0.99e-4), dict(eps=1.01), dict(eps=float("nan")), dict(eps=float("inf")),
               dict(eps=-1.0)):
        assert call(**kw) == ERANGE, kw
    for kw in (dict(guide=ODD), dict(stats=ODD)):
        assert call(**kw) == EALIGN, kw


def test_matting_fwd_bwd_refusals(lib):
    f = C.c_float
    names = ("img", "guide", "stats", "gimg", "loss", "ws")

    def call(h=8, w=12, r=1, **ptrs):
        a = {k: ptrs.get(k, B) for k in names}
        return lib.strotss_matting_fwd_bwd(a["img"], a["guide"], a["stats"], h, w, r, f(1.0), a["gimg"], a["loss"], a["ws"], NULL)

    for k in names:
        assert call(**{k: NULL}) == EINVAL, k
    assert call(h=0) == call(w=0) == call(h=1 << 15, w=1 << 15) == EINVAL
    assert call(r=0) == call(r=5) == ERANGE
    for k in ("img", "guide", "stats", "gimg", "ws"):
        assert call(**{k: ODD}) == EALIGN, k


# ------------------------------------------------------------------ 5. the command line and the engine's checks
def _args(*extra):
    import run_strotss as RS
    return RS.build_parser().parse_args(["no_such_content.jpg", "no_such_style.jpg"] + list(extra))


def test_parser_accepts_the_three_flags():
    import run_strotss as RS
    a = _args("--photo_weight", "2.5", "--photo_radius", "2", "--photo_eps", "0.01")
    assert RS._photo_term_input(a) == (2.5, 2, 0.01)
    assert RS._photo_term_input(_args("--photo_weight", "0")) == (0.0, 1, 1e-4) == (0.0, RS.DEFAULT_PHOTO_RADIUS, RS.DEFAULT_PHOTO_EPS)
    a = _args()
    assert a.photo_weight is None and a.photo_radius is None and a.photo_eps is None and RS._photo_term_input(a) is None
    assert RS._photo_term_input(argparse.Namespace()) is None              # a namespace from before the flags existed
    assert RS._photo_term_input(_args("--photo_weight", "1", "--photo_eps", "1e-4"))[2] == 1e-4     # the float32 value is in range


REFUSED = [
    ("--photo_weight", "-1"), ("--photo_weight", "nan"), ("--photo_weight", "inf"),
    ("--photo_radius", "2"), ("--photo_eps", "0.01"),                       # need --photo_weight
    ("--photo_weight", "1", "--photo_radius", "0"), ("--photo_weight", "1", "--photo_radius", "5"),
    ("--photo_weight", "1", "--photo_eps", "0.00009"), ("--photo_weight", "1", "--photo_eps", "1.5"),
    ("--photo_weight", "1", "--photo_eps", "nan"),
    ("--photo_weight", "1", "--strips"), ("--photo_weight", "1", "--video", "--strips"),
]


@pytest.mark.parametrize("extra", REFUSED, ids=[" ".join(e) for e in REFUSED])
def test_refusals_come_before_any_file_is_opened(extra):
    """the content and style paths do not exist: a ValueError (not a FileNotFoundError) shows the order"""
    import run_strotss as RS
    with pytest.raises(ValueError):
        RS.run(_args(*extra))


@pytest.mark.parametrize("extra", [("--photo_weight", "1"), ("--photo_weight", "1", "--video")])
def test_refused_under_torchrun_with_several_ranks(extra, monkeypatch):
    import run_strotss as RS
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(_args(*extra))


def test_engine_target_and_parameter_check():
    from nn import engine
    t = engine.PhotoTarget(torch.zeros(4, 4, 3), 1, 1e-4, 2.0)
    assert (t.radius, t.eps, t.weight) == (1, 1e-4, 2.0)
    engine.check_photo(4, 1.0)
    for r, e in ((0, 1e-2), (5, 1e-2), (1.0, 1e-2), (True, 1e-2), (1, 0.0), (1, 2.0), (1, float("nan")), (1, "x")):
        with pytest.raises(ValueError):
            engine.check_photo(r, e)
