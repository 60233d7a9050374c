"""CPU checks of the Sinkhorn style term: the command line's flags and refusals, the two new entries
in the header and in nn/_hip.py, the float64 restatement of the step's style loss, and what tests/test_hip_transport.py
holds the GPU to -- every case conditioned, torch's own float32 run within the pinned yardstick, each planted error
caught, and the float32 run of the whole step within a quarter of the step's bounds."""
import functools
import os

import numpy as np
import pytest
import torch

import _sinkhorn_cases as SC
import _sinkhorn_ref as SR
import _transport_cases as TC
import _transport_ref as TR
from oracle import strotss_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = TC.all_cosine()
ZERO = "n50_ns40_d1"


@functools.lru_cache(maxsize=None)
def ref64(label):
    c, l = [(c, l) for c, l in CASES if c.label == label][0]
    return SR.sinkhorn(c.x, c.y, "cosine", l, c.T)


# ------------------------------------------------------------------ command line
def _args(*extra, tmp=None):
    import run_strotss as RS
    base = [str(tmp / "no_content.jpg"), str(tmp / "no_style.jpg"), "-o", str(tmp / "out.jpg")] if tmp is not None else ["c", "s"]
    return RS.build_parser().parse_args(base + list(extra))


def test_parser_accepts_the_three_flags():
    import run_strotss as RS
    a = _args()
    assert a.style_transport == "remd" and a.sinkhorn_reg is None and a.sinkhorn_iters is None
    assert RS._style_transport_input(a) == dict(style_transport="remd", sinkhorn_l=10.0, sinkhorn_iters=30)
    a = _args("--style_transport", "sinkhorn")
    assert RS._style_transport_input(a) == dict(style_transport="sinkhorn", sinkhorn_l=10.0, sinkhorn_iters=30)
    a = _args("--style_transport", "sinkhorn", "--sinkhorn_reg", "4.5", "--sinkhorn_iters", "64")
    assert RS._style_transport_input(a) == dict(style_transport="sinkhorn", sinkhorn_l=4.5, sinkhorn_iters=64)
    with pytest.raises(SystemExit):
        _args("--style_transport", "emd")
    assert {"--style_transport", "--sinkhorn_reg", "--sinkhorn_iters"} <= {n for names, _ in RS._FLAGS for n in names}


SK = ["--style_transport", "sinkhorn"]
REFUSALS = [(["--sinkhorn_reg", "5"], "need --style_transport sinkhorn"), (["--sinkhorn_iters", "5"], "need --style_transport"),
            (["--style_transport", "remd", "--sinkhorn_iters", "5"], "need --style_transport"),
            (SK + ["--sinkhorn_reg", "0"], "sinkhorn_l"), (SK + ["--sinkhorn_reg", "-2"], "sinkhorn_l"),
            (SK + ["--sinkhorn_reg", "inf"], "sinkhorn_l"), (SK + ["--sinkhorn_reg", "nan"], "sinkhorn_l"),
            (SK + ["--sinkhorn_iters", "0"], "1..64"), (SK + ["--sinkhorn_iters", "65"], "1..64"),
            (SK + ["--strips"], "--strips"), (SK + ["--video", "--compute_flow"], None)]


@pytest.mark.parametrize("extra,match", REFUSALS[:-1])
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
        RS.run(_args(*SK, tmp=tmp_path))
    assert not (tmp_path / "out.jpg").exists()


def test_engine_argument_check():
    from nn import engine as E
    E.check_style_transport("remd", 10.0, 30)
    E.check_style_transport("sinkhorn", 0.5, 1)
    E.check_style_transport("sinkhorn", 3, 64)
    for bad in (("emd", 10.0, 30), (None, 10.0, 30), ("sinkhorn", 0.0, 30), ("sinkhorn", -1.0, 30),
                ("sinkhorn", float("nan"), 30), ("sinkhorn", float("inf"), 30), ("sinkhorn", "10", 30), ("sinkhorn", 10.0, 0),
                ("sinkhorn", 10.0, 65), ("sinkhorn", 10.0, 2.5), ("sinkhorn", 10.0, True)):
        with pytest.raises(ValueError):
            E.check_style_transport(*bad)


# ------------------------------------------------------------------ ABI
def test_header_declares_and_table_lists_the_entries():
    from test_abi_exports import declared_symbols
    from nn import _hip
    syms = declared_symbols()
    for name in ("strotss_sinkhorn_step_workspace_bytes", "strotss_sinkhorn_cos_fwd_bwd_panels"):
        assert name in syms and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["strotss_sinkhorn_cos_fwd_bwd_panels"][1]) == 18
    assert len(_hip.SIGNATURES["strotss_sinkhorn_step_workspace_bytes"][1]) == 3
    assert sorted(_hip.SIGNATURES) == syms and _hip.ABI_VERSION == 8


# ------------------------------------------------------------------ the restatement and its cases
def test_restatement_is_style_loss_with_the_transport_swapped():
    rng = np.random.default_rng(0)
    x, y = torch.as_tensor(SC._rows(rng, 40, 35)), torch.as_tensor(SC._rows(rng, 50, 35))
    for alpha in (0.5, 8.0):
        a = TR.style_loss_sinkhorn(x, y, alpha, 10.0, 7)
        b = O.style_loss(x, y, alpha) - O.relaxed_emd(x, y) + O.sinkhorn_knopp(x, y, "cosine", 10.0, 7)
        assert abs(float(a) - float(b)) <= 1e-14 * abs(float(b))


def test_every_case_is_conditioned():
    for c, l in CASES:
        assert SR.conditioned(c, "cosine", l), (c.label, l)
    c = TC.make_case(TC.FAR_ROW_LABEL)
    kv, _ = SR.clamp_arguments(c.x, c.y, "cosine", TC.l_of(c.label), 1)
    assert kv.min() < 2.0 * SC.FAR_ROW_SUM and kv.min() / c.n < SC.CLAMP_EPS        # from v_0 = 1 / n it would clamp


def test_float32_run_lies_within_the_pinned_yardstick():
    for c, l in CASES:
        l64, g64 = ref64(c.label)
        l32, g32 = SR.sinkhorn(c.x, c.y, "cosine", l, c.T, torch.float32)
        if c.label == ZERO:
            assert np.abs(g64).max() <= 1e-6 and np.abs(g32).max() <= 1e-6
            continue
        fam = SR.family(c, "cosine")
        e, rel = SR.err_over_max(g32, g64), abs(l32 - l64) / abs(l64)
        print(f"MEASURE err32 {c.label} {e:.3e} loss {rel:.3e} family {fam}")
        # the bound tests/test_sinkhorn_cases_cpu.py puts on a run's worst value: twice the pinned one (the float32 run's
        # sums depend on the machine's thread count: t_n1024_ns1024_T30 gives 1.1e-6 with eight threads, 2.4e-6 with one)
        assert e <= 2.0 * SR.ERR32[fam] and SR.TOL_SK[fam] == TR.MARGIN * SR.ERR32[fam], (c.label, e)
        assert rel <= SR.loss_tolerance(c, l)


MUTANTS = {"second_marginal_1_over_ns": dict(second_marginal_ns=True), "v0_1_over_n": dict(v0_over_n=True)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_errors_fail_the_comparison(name):
    """in float64, the comparison of tests/test_hip_transport.py: every element within TOL_SK[family] of max|ref|"""
    caught = []
    for c, l in CASES:
        if c.label == ZERO or c.n * c.ns > 100000:
            continue
        _, g64 = ref64(c.label)
        _, gm = SR.sinkhorn(c.x, c.y, "cosine", l, c.T, fn=functools.partial(SR.variant, **MUTANTS[name]))
        tol = SR.TOL_SK[SR.family(c, "cosine")]
        if not (np.abs(gm - g64) <= tol * np.abs(g64).max()).all():
            caught.append(c.label)
    print(f"MEASURE mutant {name} caught on {caught}")
    assert caught, name
    if name == "v0_1_over_n":       # invariant under a rescaling of v_0 while no clamp acts: only the far row tells
        assert TC.FAR_ROW_LABEL in caught


# ------------------------------------------------------------------ the step's bounds
@pytest.mark.parametrize("threads", [1, None], ids=["one_thread", "default_threads"])
def test_float32_step_stays_within_a_quarter_of_the_bounds(threads):
    """with one thread and with the machine's own count: the float32 sums, and with them which near-ties flip, depend on it"""
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        _float32_steps()
    finally:
        torch.set_num_threads(before)


def _float32_steps():
    worst_s = worst_g = 0.0
    for label, h, w, n, seed, masked in TC.STEPS + [TC.BLEND_STEP]:
        blend = TC.BLEND_WEIGHTS if label == TC.BLEND_STEP[0] else None
        P = TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None, n_styles=2 if blend else 1)
        if masked:                           # the first region has ns != n
            assert (len(P["s_idx"][0][0]), len(P["idx"][0])) == (600, 768) and len(P["idx"][1]) == 1024
        r64 = TR.reference_step(P, 10.0, 30, blend_weights=blend)
        r32 = TR.reference_step(P, 10.0, 30, torch.float32, blend_weights=blend)
        sc, gr = TR.step_distance(r32, r64)
        print(f"MEASURE step32 {label} scalar {sc:.3e} grad {gr:.3e}")
        worst_s, worst_g = max(worst_s, sc), max(worst_g, gr)
    assert worst_s <= TR.TOL_SCALAR / 4 and worst_g <= TR.GRAD_TOL / 4
