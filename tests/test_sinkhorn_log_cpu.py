"""CPU checks of the log-domain Sinkhorn term: the float64 restatement (tests/_sinkhorn_log_ref.py)
against the linear statement where that engages no clamp, the case at which the linear statement fails, the float32
yardstick tests/test_hip_sinkhorn_log.py takes its tolerances from, the planted errors, the command line's flag and
refusals, the two entries in the header and in nn/_hip.py, and the float32 run of the whole step.

Two of the checks are narrower than a first reading of them, because of what the iteration is:

* Marginals.  A half-step enforces ONE marginal: after phi_T, sum_j exp(phi_T[i] + psi_{T-1}[j] - L M) = px for every i, and
  after psi_T the column sums equal py.  Both hold to 1e-9 in the log form and are asserted.  The row sums of the FINAL
  plan equal px only at convergence (the far-row case at L = 100 is 4.2e-3 off after 30 scalings), so that is not asserted
  to 1e-9; what is asserted of the final plan is that the far row carries most of its mass where the linear form gives it
  none.
* psi_0 = log py.  Without a clamp the iteration is invariant under psi_0 -> psi_0 + c: phi_t moves by -c, psi_t by +c, the
  plan, the loss and the gradient not at all (the linear form's v_0 control needed a clamp to show).  The comparison of loss
  and gradient therefore cannot catch this planted error on any case; it is asserted to be invisible there (1e-10), and
  caught where it does show: in phi_T, which moves by log n."""
import functools
import os

import numpy as np
import pytest
import torch

import _sinkhorn_log_cases as LC
import _sinkhorn_log_ref as LR
import _sinkhorn_ref as SR
import _transport_cases as TC
import _transport_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ZERO = "n50_ns40_d1"            # one column: every cosine distance is 0, so are the loss and the gradient


@functools.lru_cache(maxsize=None)
def ref64(label):
    c = LC.make_case(label)
    return LR.run(c.x, c.y, c.l, c.T)


@functools.lru_cache(maxsize=None)
def run32(label):
    c = LC.make_case(label)
    return LR.run(c.x, c.y, c.l, c.T, torch.float32)


# ------------------------------------------------------------------ 1: the same function where no clamp acts
@pytest.mark.parametrize("c", LC.conditioned_linear_cases(), ids=lambda c: c.label)
def test_log_form_equals_the_linear_statement_where_no_clamp_acts(c):
    L, T = 10.0, 30
    kv, ktu = SR.clamp_arguments(c.x, c.y, "cosine", L, T)
    assert min(kv.min(), ktu.min()) >= LC.SC.CLAMP_CLEAR
    l_lin, g_lin = SR.sinkhorn(c.x, c.y, "cosine", L, T)
    l_log, g_log = LR.run(c.x, c.y, L, T)
    scale = max(np.abs(g_lin).max(), 1e-6 if c.label == ZERO else 0.0)
    print(f"MEASURE log_vs_linear {c.label} loss {abs(l_log - l_lin):.3e} grad {np.abs(g_log - g_lin).max() / scale:.3e}")
    assert abs(l_log - l_lin) <= 1e-10 * max(abs(l_lin), 1e-6 if c.label == ZERO else 0.0)
    assert (np.abs(g_log - g_lin) <= 1e-10 * scale).all()


# ------------------------------------------------------------------ 2: where the linear statement fails
def test_linear_statement_clamps_at_L100_and_the_log_form_does_not():
    c = LC.make_case(LC.FAR_ROW_LABEL)
    assert c.l == 100.0
    lin_rows, least = LR.linear_row_marginals(c.x, c.y, c.l, c.T)
    assert least < LC.SC.CLAMP_EPS, "the linear float64 statement engages its first clamp here"
    (l_lin, g_lin), (l_log, g_log) = SR.sinkhorn(c.x, c.y, "cosine", c.l, c.T), ref64(c.label)
    tol = LR.TOL_SK[LR.family(c)]
    dist = LR.err_over_max(g_lin, g_log)
    print(f"MEASURE linear_vs_log {c.label} grad {dist:.3e} loss {abs(l_lin - l_log) / l_log:.3e} clamp argument {least:.3e}")
    assert dist > 100.0 * tol and abs(l_lin - l_log) / l_log > 100.0 * LR.TOL_SCALAR
    # the marginal each half-step enforces
    px, py = 1.0 / c.ns, 1.0 / c.n
    with torch.no_grad():
        x, y = LR._t(c.x, torch.float64), LR._t(c.y, torch.float64)
        M, phi, psi = LR.potentials(x, y, c.l, c.T)
        _, _, psi_before = LR.potentials(x, y, c.l, c.T - 1)
        after_phi = torch.exp(phi + psi_before - c.l * M).sum(1).numpy()
        plan = torch.exp(phi + psi - c.l * M)
        # the linear statement at the same point: u_T (K v_{T-1})
        K = torch.exp(-c.l * M)
        v = torch.ones(c.n, 1, dtype=torch.float64)
        for t in range(c.T):
            a = K @ v
            u = px / torch.clamp(a, min=1e-12)
            v = py / torch.clamp(K.t() @ u, min=1e-12)
        lin_after_u = (u * a).numpy().ravel()
    print(f"MEASURE marginals {c.label} log rows after phi {np.abs(after_phi - px).max():.3e} linear {np.abs(lin_after_u - px).max():.3e} "
          f"log columns after psi {np.abs(plan.sum(0).numpy() - py).max():.3e} final rows log {np.abs(plan.sum(1).numpy() - px).max():.3e} "
          f"linear {np.abs(lin_rows - px).max():.3e}")
    assert np.abs(after_phi - px).max() <= 1e-9 and np.abs(plan.sum(0).numpy() - py).max() <= 1e-9
    assert np.abs(lin_after_u - px).max() > 0.99 * px            # the clamped row gets no mass at all
    assert float(plan.sum(1)[0]) > 0.5 * px and lin_rows[0] < 1e-9 * px


# ------------------------------------------------------------------ 3: the yardstick
@pytest.mark.parametrize("label", LC.LABELS)
def test_float32_run_lies_within_the_pinned_yardstick_and_the_cap(label):
    c = LC.make_case(label)
    (l64, g64), (l32, g32) = ref64(label), run32(label)
    fam = LR.family(c)
    e, rel = LR.err_over_max(g32, g64), abs(l32 - l64) / abs(l64)
    print(f"MEASURE err32 {label} {e:.3e} loss {rel:.3e} family {fam}")
    assert np.isfinite(g64).all() and np.abs(g64).max() > 0
    assert LR.TOL_SK[fam] == LR.MARGIN * LR.ERR32[fam] <= LR.CAP
    assert LR.MARGIN * LR.ERR32_LOSS[fam] <= LR.TOL_SCALAR
    # twice the pinned value, as tests/test_sinkhorn_cases_cpu.py: the float32 sums depend on the machine's thread count
    assert e <= 2.0 * LR.ERR32[fam] and rel <= 2.0 * LR.ERR32_LOSS[fam], (label, e, rel)


def test_every_family_pin_is_reached_by_one_of_its_cases():
    """a pin far above what its cases give would be a loose tolerance: the worst case of a family reaches a quarter of it"""
    worst = {}
    for label in LC.LABELS:
        fam = LR.family(LC.make_case(label))
        worst[fam] = max(worst.get(fam, 0.0), LR.err_over_max(run32(label)[1], ref64(label)[1]))
    assert set(worst) == set(LR.ERR32)
    for fam, e in worst.items():
        assert e >= LR.ERR32[fam] / 4.0, (fam, e)


@pytest.mark.parametrize("label", [lb for lb in LC.LABELS if not LC.make_case(lb).full])
def test_pinned_seed_is_the_first_that_meets_the_cap(label):
    k, eg, el = LC.search(label)
    assert k == LC.make_case(label).seed_try and k < LC.TRIES


def test_cases_cover_the_reduction_edges():
    by = {c.label: c for c in LC.all_cases()}
    assert any(c.n < LR.COL_CHUNKS for c in by.values()) and any(c.n == 1 and c.ns == 1 for c in by.values())
    assert any(c.n % LR.COL_CHUNKS and c.n > LR.COL_CHUNKS and -(-c.n // LR.COL_CHUNKS) * (LR.COL_CHUNKS - 1) >= c.n for c in by.values())
    assert {c.T for c in by.values()} >= {1, 30, 64} and {c.l for c in by.values()} >= {1.0, 10.0, 100.0, LC.L_MAX}
    assert by[LC.FAR_ROW_EMPTY_LABEL].n < LR.COL_CHUNKS and LC.L_MAX <= 1000.0


# ------------------------------------------------------------------ 4: planted errors
def _passes(got, ref, tol):
    return bool(np.isfinite(got).all() and (np.abs(got - ref) <= tol * np.abs(ref).max()).all())


MUTANTS = {"log_px_and_log_py_swapped": dict(swap_marginals=True), "lse_without_max_shift": dict(shift=False)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_errors_fail_the_comparison(name):
    """the GPU test's comparison (every gradient element within TOL_SK[family] of max|ref|, float64 reference) applied to
    the restatement's float32 run -- the precision the kernels work in -- with one error planted; unswitched, that run
    passes on every case (test_float32_run_lies_within_the_pinned_yardstick_and_the_cap)"""
    caught = []
    for c in LC.all_cases():
        if c.full:
            continue
        _, g64 = ref64(c.label)
        with np.errstate(all="ignore"):
            _, gm = LR.run(c.x, c.y, c.l, c.T, torch.float32, **MUTANTS[name])
        tol = LR.TOL_SK[LR.family(c)]
        assert _passes(run32(c.label)[1], g64, tol)
        if not _passes(gm, g64, tol):
            caught.append(c.label)
    print(f"MEASURE mutant {name} caught on {caught}")
    assert caught, name
    if name == "lse_without_max_shift":      # exp(-L M) of the far row underflows in float32 at L = 100
        assert LC.FAR_ROW_LABEL in caught


def test_planted_psi0_shows_in_the_potentials_only():
    """see the head of this file: invariant in loss and gradient, log n in phi_T"""
    for c in LC.all_cases():
        if c.full:
            continue
        (l64, g64), (lm, gm) = ref64(c.label), LR.run(c.x, c.y, c.l, c.T, psi0_log_py=True)
        assert abs(lm - l64) <= 1e-10 * abs(l64) and (np.abs(gm - g64) <= 1e-10 * np.abs(g64).max()).all(), c.label
        with torch.no_grad():
            x, y = LR._t(c.x, torch.float64), LR._t(c.y, torch.float64)
            phi, phim = LR.potentials(x, y, c.l, c.T)[1], LR.potentials(x, y, c.l, c.T, psi0_log_py=True)[1]
        assert np.abs((phim - phi).numpy() - np.log(c.n)).max() <= 1e-9 * max(1.0, np.log(c.n))
        assert c.n == 1 or np.abs((phim - phi).numpy()).min() > 0.5


def test_planted_empty_chunk_pair_fails_the_chunked_reduction():
    """the column pass restated in NumPy float32 (16 row chunks, (max, sum) pairs combined in order): with (-inf, 0) for a
    chunk without rows phi_T lies within the float32 yardstick of the float64 potentials on every case; with (0, 0) the
    combined maximum is 0 where every term is below exp(-87), the sum underflows and phi_T is not finite"""
    caught = []
    for c in LC.all_cases():
        if c.full:
            continue
        with torch.no_grad():
            phi = LR.potentials(LR._t(c.x, torch.float64), LR._t(c.y, torch.float64), c.l, c.T)[1].numpy().ravel()
        good = LR.run_chunked32(c.x, c.y, c.l, c.T)
        bad = LR.run_chunked32(c.x, c.y, c.l, c.T, empty=(0.0, 0.0))
        # phi is a logarithm: an absolute bound, 2 L 2^-24 of the exponent's rounding per scaling and 8 for the sums
        bound = 8.0 * 2.0 * max(c.l, 10.0) * 2.0 ** -24 * 4.0
        print(f"MEASURE chunked {c.label} good {np.abs(good - phi).max():.3e} bound {bound:.3e}")
        assert np.isfinite(good).all() and np.abs(good - phi).max() <= bound, c.label
        if not (np.isfinite(bad).all() and np.abs(bad - phi).max() <= bound):
            caught.append(c.label)
    print(f"MEASURE mutant empty_chunk_0_0 caught on {caught}")
    assert LC.FAR_ROW_EMPTY_LABEL in caught
    assert all(LC.make_case(lb).n < LR.COL_CHUNKS or LC.make_case(lb).n % LR.COL_CHUNKS for lb in caught)


def test_chunk_combine_of_two_empty_pairs_is_empty():
    a = np.full((3, 5), -1.0, np.float32)              # 3 rows: chunks 3 .. 15 are empty and combine with each other last
    out = LR.chunked_column_lse(a)
    assert np.isfinite(out).all() and np.abs(out - (-1.0 + np.log(3.0))).max() <= 1e-6


# ------------------------------------------------------------------ 5: command line, engine check, ABI
def _args(*extra, tmp=None):
    import run_strotss as RS
    base = [str(tmp / "no_content.jpg"), str(tmp / "no_style.jpg"), "-o", str(tmp / "out.jpg")] if tmp is not None else ["c", "s"]
    return RS.build_parser().parse_args(base + list(extra))


SK = ["--style_transport", "sinkhorn"]


def test_parser_accepts_the_flag():
    import run_strotss as RS
    assert _args().sinkhorn_log is False
    assert RS._style_transport_input(_args(*SK)) == dict(style_transport="sinkhorn", sinkhorn_l=10.0, sinkhorn_iters=30)
    a = _args(*SK, "--sinkhorn_log", "--sinkhorn_reg", "1000", "--sinkhorn_iters", "64")
    assert RS._style_transport_input(a) == dict(style_transport="sinkhorn", sinkhorn_l=1000.0, sinkhorn_iters=64, sinkhorn_log=True)
    assert "--sinkhorn_log" in {n for names, _ in RS._FLAGS for n in names} and "--sinkhorn_log" in RS.__doc__
    help_ = " ".join(RS.build_parser().format_help().split())
    assert "--sinkhorn_log" in help_ and "(0, 1000]" in help_


REFUSALS = [(["--sinkhorn_log"], "needs --style_transport sinkhorn"),
            (["--style_transport", "sliced", "--sinkhorn_log"], "needs --style_transport sinkhorn"),
            (["--style_transport", "remd", "--sinkhorn_log"], "needs --style_transport sinkhorn"),
            (SK + ["--sinkhorn_log", "--sinkhorn_reg", "1000.5"], "at most 1000"),
            (SK + ["--sinkhorn_log", "--sinkhorn_reg", "0"], "sinkhorn_l"),
            (SK + ["--sinkhorn_log", "--sinkhorn_iters", "65"], "1..64"),
            (SK + ["--sinkhorn_log", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match=match):
        RS.run(_args(*extra, tmp=tmp_path))
    with pytest.raises(ValueError, match=match):
        RS.run(_args(*(extra + ["--video", "--compute_flow"]), tmp=tmp_path))
    assert not (tmp_path / "out.jpg").exists()


def test_refused_on_several_ranks(monkeypatch, tmp_path):
    import run_strotss as RS
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(_args(*SK, "--sinkhorn_log", tmp=tmp_path))


def test_engine_argument_check():
    from nn import engine as E
    assert E.STYLE_TRANSPORTS == ("remd", "sinkhorn", "sliced") and E.SINKHORN_LOG_MAX_L == 1000.0
    E.check_style_transport("sinkhorn", 100.0, 30, sinkhorn_log=True)
    E.check_style_transport("sinkhorn", 1000.0, 64, sinkhorn_log=True)
    E.check_style_transport("sinkhorn", 5000.0, 30, sinkhorn_log=False)         # the linear form's range is unchanged
    E.check_style_transport("sinkhorn", 5000.0, 30)
    E.check_style_transport("remd", 10.0, 30, sinkhorn_log=False)
    for bad in (("remd", 10.0, 30), ("sliced", 10.0, 30), ("sinkhorn", 1000.5, 30), ("sinkhorn", 0.0, 30),
                ("sinkhorn", float("nan"), 30), ("sinkhorn", float("inf"), 30), ("sinkhorn", 10.0, 65)):
        with pytest.raises(ValueError):
            E.check_style_transport(*bad, sinkhorn_log=True)
    with pytest.raises(ValueError):
        E.check_style_transport("sinkhorn", 10.0, 30, sinkhorn_log="yes")


def test_header_declares_and_table_lists_the_entries():
    from test_abi_exports import declared_symbols
    from nn import _hip
    syms = declared_symbols()
    for name in ("strotss_sinkhorn_log_step_workspace_bytes", "strotss_sinkhorn_log_cos_fwd_bwd_panels"):
        assert name in syms and name in _hip.SIGNATURES
    assert _hip.SIGNATURES["strotss_sinkhorn_log_cos_fwd_bwd_panels"] == _hip.SIGNATURES["strotss_sinkhorn_cos_fwd_bwd_panels"]
    assert _hip.SIGNATURES["strotss_sinkhorn_log_step_workspace_bytes"] == _hip.SIGNATURES["strotss_sinkhorn_step_workspace_bytes"]
    assert sorted(_hip.SIGNATURES) == syms


# ------------------------------------------------------------------ 6: the step's bounds
def test_step_restatement_is_the_linear_one_with_the_term_swapped():
    rng = np.random.default_rng(0)
    x, y = torch.as_tensor(LC.SC._rows(rng, 40, 35)), torch.as_tensor(LC.SC._rows(rng, 50, 35))
    a, b = LR.style_loss_sinkhorn_log(x, y, 8.0, 10.0, 7), TR.style_loss_sinkhorn(x, y, 8.0, 10.0, 7)
    assert abs(float(a) - float(b)) <= 1e-12 * abs(float(b))
    assert TR.style_loss_sinkhorn.__module__ == "_transport_ref"


@pytest.mark.parametrize("L", [10.0, 100.0])
def test_float32_step_stays_within_a_quarter_of_the_bounds(L):
    worst_s = worst_g = 0.0
    for label, h, w, n, seed, masked in TC.STEPS + [TC.BLEND_STEP]:
        blend = TC.BLEND_WEIGHTS if label == TC.BLEND_STEP[0] else None
        P = TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None, n_styles=2 if blend else 1)
        r64 = LR.reference_step(P, L, 30, blend_weights=blend)
        r32 = LR.reference_step(P, L, 30, torch.float32, blend_weights=blend)
        sc, gr = TR.step_distance(r32, r64)
        print(f"MEASURE step32 L{L:g} {label} scalar {sc:.3e} grad {gr:.3e}")
        worst_s, worst_g = max(worst_s, sc), max(worst_g, gr)
    assert worst_s <= LR.step_bounds(L)[0] / 4 and worst_g <= LR.step_bounds(L)[1] / 4
