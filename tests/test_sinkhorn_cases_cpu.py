"""CPU checks of the Sinkhorn and pairwise-distance cases (tests/_sinkhorn_cases.py) and of what tests/test_hip_sinkhorn.py
holds the HIP entries to (tests/_sinkhorn_ref.py): every case meets its conditioning with the l pinned for it, the float32
yardstick is what is pinned, torch's own float32 run passes the tolerances made from it, and every planted error misses them
by at least ten times on a case of at most five iterations."""
import functools

import numpy as np
import pytest
import torch

import _sinkhorn_cases as SC
import _sinkhorn_ref as SR
from _loss_ref import TOL_SCALAR

RUNS = SC.runs()


@functools.lru_cache(maxsize=None)
def ref64(label, metric):
    c = SC.make_case(label)
    return SR.sinkhorn(c.x, c.y, metric, SR.l_of(label, metric), c.T)


def zero_gradient(label, metric):
    return label == "n50_ns40_d1" and metric == "cosine"     # one column: every cosine distance is 0


def test_every_case_is_conditioned_with_its_l():
    for label, metric in RUNS:
        c = SC.make_case(label)
        l = SR.choose_l(c, metric)
        print(f"MEASURE l {label}:{metric} {l}")
        assert l is not None and l == SR.l_of(label, metric), (label, metric, l)
        kv, ktu = SR.clamp_arguments(c.x, c.y, metric, l, c.T)
        if c.kind == "all_clamped":
            assert (kv <= SC.CLAMPED_BELOW).all()
            assert ((ktu <= SC.CLAMPED_BELOW) | (ktu >= SC.CLAMPED_ABOVE)).all()
            assert (ktu <= SC.CLAMPED_BELOW).any(), "no K^T u clamp acts"
        else:
            assert min(kv.min(), ktu.min()) >= SC.CLAMP_CLEAR, (label, metric, kv.min(), ktu.min())
        if metric != "cosine":
            margin = SC.l2_margin(c.x, c.y, c.kind)
            assert (margin >= 0).all(), (label, "an l2 clamp within f32 rounding")
    c = SC.make_case("n48_ns40_clamp_pair")
    for (j, i), m in ((SC.CLAMP_PAIR, 0.0), (SC.NEAR_PAIR, 2.0 ** -24)):
        for dt in (np.float32, np.float64):
            x, y = c.x[i].astype(dt), c.y[j].astype(dt)
            assert (x * x).sum() + (y * y).sum() - 2 * (x * y).sum() == m
    c = SC.make_case("n200_ns200_dup_rows")
    assert np.array_equal(c.y[SC.DUP_ROWS[0]], c.y[SC.DUP_ROWS[1]])


def test_restatement_with_no_switch_is_the_oracle():
    for label, metric in (("n65_ns31_T2", "cosine"), ("n48_ns40_clamp_pair", "l2"), ("n17_ns1", "both")):
        c = SC.make_case(label)
        l, g = SR.sinkhorn(c.x, c.y, metric, SR.l_of(label, metric), c.T, fn=SR.variant)
        l0, g0 = ref64(label, metric)
        assert l == l0 and np.array_equal(g, g0)


def test_float32_yardstick_is_what_is_pinned():
    worst = {}
    for label, metric in RUNS:
        c = SC.make_case(label)
        l64, g64 = ref64(label, metric)
        l32, g32 = SR.sinkhorn(c.x, c.y, metric, SR.l_of(label, metric), c.T, torch.float32)
        if zero_gradient(label, metric):
            assert np.abs(g64).max() <= 1e-6 and np.abs(g32).max() <= 1e-6 and abs(l64) <= 1e-6
            continue
        fam = SR.family(c, metric)
        e = SR.err_over_max(g32, g64)
        rel = abs(l32 - l64) / abs(l64)
        print(f"MEASURE err32 {label}:{metric} {e:.3e} loss {rel:.3e} family {fam}")
        worst[fam] = max(worst.get(fam, 0.0), e)
        assert e <= SR.TOL_SK[fam]
        assert rel <= SR.loss_tolerance(c, SR.l_of(label, metric))
        if c.kind != "all_clamped":
            assert SR.loss_tolerance(c, SR.l_of(label, metric)) == TOL_SCALAR
    print("MEASURE err32 worst", worst)
    assert set(worst) == set(SR.ERR32)
    for fam, e in worst.items():
        assert SR.ERR32[fam] / 4.0 <= e <= 2.0 * SR.ERR32[fam], (fam, e)
        assert SR.TOL_SK[fam] == 8.0 * SR.ERR32[fam]


def test_pairwise_float32_yardstick_is_what_is_pinned():
    worst = {}
    for label in SC.PAIR_LABELS:
        x, y, G = SC.make_pair(label)
        assert (SC.l2_margin(x, y, "plain") >= 0).all()
        for kind in SC.PAIR_KINDS:
            a64, a32 = SR.pair_grads(x, y, G, kind), SR.pair_grads(x, y, G, kind, torch.float32)
            e = max(SR.err_over_max(a32[0], a64[0]), SR.err_over_max(a32[1], a64[1]))
            fam = SR.pair_family(x.shape[1], kind)
            print(f"MEASURE err32 {label}:{kind} {e:.3e} family {fam}")
            worst[fam] = max(worst.get(fam, 0.0), e)
    for fam, e in worst.items():
        assert SR.ERR32_PAIR[fam] / 4.0 <= e <= 2.0 * SR.ERR32_PAIR[fam], (fam, e)
        assert SR.TOL_PAIR[fam] == 8.0 * SR.ERR32_PAIR[fam]


MUTANTS = {
    "one_iteration_less": None,
    "second_marginal_1_over_ns": dict(second_marginal_ns=True),
    "v0_1_over_n": dict(v0_over_n=True),
    "l2_gradient_through_the_clamp": dict(l2_through_clamp=True),
    "cosine_chain_dropped_from_both": dict(drop_cosine_chain=True),
}


def _mutant_runs(name):
    for label, metric in RUNS:
        c = SC.make_case(label)
        if c.T > 5 or zero_gradient(label, metric):
            continue
        if name == "one_iteration_less" and c.T < 2:
            continue
        if name == "second_marginal_1_over_ns" and c.n == c.ns:
            continue
        if name == "l2_gradient_through_the_clamp" and c.kind != "clamp_pair":
            continue
        if name == "cosine_chain_dropped_from_both" and metric != "both":
            continue
        yield c, metric


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_errors_miss_the_tolerance_tenfold(name):
    """in float64 on the CPU, so that nothing but the planted error separates the two sides"""
    shown = []
    for c, metric in _mutant_runs(name):
        l = SR.l_of(c.label, metric)
        _, g64 = ref64(c.label, metric)
        if MUTANTS[name] is None:
            _, gm = SR.sinkhorn(c.x, c.y, metric, l, c.T - 1)
        else:
            _, gm = SR.sinkhorn(c.x, c.y, metric, l, c.T, fn=functools.partial(SR.variant, **MUTANTS[name]))
        times = SR.err_over_max(gm, g64) / SR.TOL_SK[SR.family(c, metric)]
        print(f"MEASURE mutant {name} {c.label}:{metric} {times:.3g} x tolerance")
        if times >= 10.0:
            shown.append((c.label, metric))
    assert shown, name
    if name == "v0_1_over_n":
        # u -> c u, v -> v / c leaves every later scaling and the loss unchanged while no clamp acts, and where K v clamps from
        # v_0 = 1 it clamps from 1 / n too: only a row whose K v_0 a start of 1 / n pushes under the clamp tells the two apart
        assert shown == [("n4096_ns2_far_row", "l2")]


def test_rows_gemm_reference_is_the_formula():
    W, B, x, r, q = SC.rows_gemm_problem(5, 3, 32, 1, beyond_k=True)
    base = np.zeros_like(x)
    out, bound = SR.rows_gemm(W, B, x, r, q, -0.5, 32, base)
    for i in range(5):
        acc = sum(W[i, j] * B[j] for j in range(32))
        assert np.allclose(out[i], -0.5 * r[i] * (acc - x[i] * r[i] * q[i]), rtol=1e-13, atol=0)
    assert (bound > 0).all() and (bound < 1e-4 * np.abs(out).max()).all()
    W0 = SC.rows_gemm_problem(5, 3, 32, 1)[0]
    assert np.array_equal(W0[:, :3], W[:, :3]) and not W0[:, 3:].any() and W[:, 3:].all()
