"""CPU checks of the sliced palette term: the directions, the float64 restatement's gradient, scale and
mass conservation, what tests/test_hip_palette_sliced.py holds the GPU to -- every tie-free case's gap, the float32 run within
the pinned yardsticks, each planted error caught, the float32 run of the whole step within a quarter of the step's bounds --
the command line's flags and refusals, the engine's argument checks, and the two new entries in the header and in nn/_hip.py."""
import os

import numpy as np
import pytest
import torch

import _palette_sliced_cases as PC
import _palette_sliced_ref as PR
import _palette_step_cases as PS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the directions
@pytest.mark.parametrize("P", (1, 2, 8, 64, 1024))
def test_directions_are_the_stated_lattice(P):
    from nn import rand
    th = rand.palette_directions(P)
    assert th.shape == (P, 3) and th.dtype == np.float32
    k = np.arange(P, dtype=np.float64)
    z, phi = (k + 0.5) / P, k * np.pi * (3.0 - np.sqrt(5.0))
    want = np.stack([np.sqrt(1 - z * z) * np.cos(phi), np.sqrt(1 - z * z) * np.sin(phi), z], 1)
    assert np.array_equal(th, want.astype(np.float32))
    assert np.abs(np.linalg.norm(th.astype(np.float64), axis=1) - 1.0).max() <= 1e-7
    assert (th[:, 2] > 0).all()
    assert np.array_equal(th, rand.palette_directions(P)), "no seed, no state"


@pytest.mark.parametrize("P,lo,hi", [(64, 0.984, 1.016), (256, 0.996, 1.004)])
def test_lattice_estimates_a_vectors_length(P, lo, hi):
    """(2 / P) sum_p |<theta_p, v>| for 2000 random unit v: the margin the scale rests on.  This draw gives 0.9849 .. 1.0146 at
    P = 64 and 0.9970 .. 1.0031 at P = 256 (another draw of 2000 gave 0.985 .. 1.015 and 0.997 .. 1.003): held to the next
    thousandth outside"""
    from nn import rand
    th = rand.palette_directions(P).astype(np.float64)
    v = np.random.default_rng(0).standard_normal((2000, 3))
    v /= np.linalg.norm(v, axis=1, keepdims=True)
    est = 2.0 / P * np.abs(v @ th.T).sum(1)
    print(f"MEASURE lattice P={P} {est.min():.4f} .. {est.max():.4f}")
    assert lo <= est.min() and est.max() <= hi


# ------------------------------------------------------------------ the restatement
def test_gradient_matches_central_differences():
    """the loss is piecewise linear: far below the cases' gap the two agree to rounding"""
    h = 1e-7
    for label in ("n37_ns64_p8", "n64_ns37_p8", "n65_ns33_p8", "n64_ns64_p8"):
        c = PC.make_case(label)
        _, g = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)
        rng = np.random.default_rng(3)
        for _ in range(4):
            dy = rng.standard_normal(c.y.shape)
            up = PR.palette_sliced(c.x, c.y + h * dy, c.dirs, c.rgb_to_yuv)[0]
            down = PR.palette_sliced(c.x, c.y - h * dy, c.dirs, c.rgb_to_yuv)[0]
            fd, an = (up - down) / (2 * h), float((g * dy).sum())
            assert abs(fd - an) <= 1e-7 * max(abs(an), 1e-6), (label, fd, an)


@pytest.mark.parametrize("label", ["n1_ns1_p1", "n2_ns1_p1", "n1_ns64_p8", "n37_ns64_p1", "n64_ns37_p8", "n64_ns64_p8",
                                   "n65_ns33_p1", PC.DUP_LABEL])
def test_restatement_agrees_with_autograd_through_torch_sort(label):
    c = PC.make_case(label)
    assert c.rgb_to_yuv, "the torch form converts to YUV"
    loss, g = PR.palette_sliced(c.x, c.y, c.dirs, True)
    y = torch.as_tensor(c.y).requires_grad_(True)
    lt = PS.palette_sliced_loss(torch.as_tensor(c.x), y, torch.as_tensor(c.dirs, dtype=torch.float64))
    gt, = torch.autograd.grad(lt, y)
    assert abs(float(lt) - loss) <= 1e-13 * abs(loss)
    assert np.abs(gt.numpy() - g).max() <= 1e-13 * np.abs(g).max()


def test_equal_sets_and_permutations_give_zero():
    c = PC.equal_case()
    loss, g = PR.palette_sliced(c.x, c.y, c.dirs)
    assert loss == 0.0 and not g.any()
    perm = np.random.default_rng(1).permutation(c.n)
    loss, g = PR.palette_sliced(c.x[perm], c.y, c.dirs)
    assert loss == 0.0 and not g.any()


def test_scale_is_the_l2_part_of_the_cost_it_replaces():
    """n = ns, P = 1024, the prediction the style set shifted by a constant colour v: every direction's sorted sets differ by
    <theta, M v>, so the loss is the lattice's estimate of |M v| / sqrt(3)"""
    from nn import rand
    x = np.random.default_rng(5).random((96, 3))
    v = np.array([0.11, -0.07, 0.05])
    loss, _ = PR.palette_sliced(x, x + v, rand.palette_directions(1024))
    want = np.linalg.norm(v @ PR.RGB2YUV) / np.sqrt(3.0)
    print(f"MEASURE scale {loss / want:.5f}")
    assert abs(loss - want) <= 1e-3 * want


def test_mass_conservation_where_the_relaxed_emd_sees_none():
    """A style of 32 rows of one colour and 32 of another.  Against 64 rows of the first colour the new term gives half the
    colours' distance over sqrt(3).  The relaxed EMD is max(R_X, R_Y): at that prediction the 32 style rows of the second
    colour find no match and it gives 0.749, not the "at most 1e-3" first expected of it.  Where it IS blind is one row
    further: 63 rows of the first colour and ONE of the second leave every row of both sets an exact match, and only the
    1e-6 clamp of l2_distance (sqrt(1e-6 / 3) = 5.8e-4) is left of the relaxed EMD, while the new term still gives 31/64 of
    the colours' distance.  Both predictions are held here."""
    c, red, blue = PC.two_colour_case()
    dist = np.linalg.norm((red - blue) @ PR.RGB2YUV) / np.sqrt(3.0)
    loss, g = PR.palette_sliced(c.x, c.y, c.dirs)
    print(f"MEASURE mass all-first: remd {_palette_remd(c.x, c.y):.3e} sliced {loss:.5f} want {0.5 * dist:.5f}")
    assert abs(loss - 0.5 * dist) <= 0.015 * 0.5 * dist        # the lattice's margin at P = 64
    assert np.abs(g).max() > 0
    y = c.y.copy()
    y[-1] = blue
    remd = _palette_remd(c.x, y)
    loss, g = PR.palette_sliced(c.x, y, c.dirs)
    print(f"MEASURE mass 63 + 1: remd {remd:.3e} sliced {loss:.5f} want {31 / 64 * dist:.5f}")
    assert remd <= 1e-3, "every colour of both sets has an exact match: only the 1e-6 clamp of l2_distance is left"
    assert abs(loss - 31 / 64 * dist) <= 0.015 * 31 / 64 * dist
    assert np.abs(g).max() > 0


def _palette_remd(x, y):
    """the palette relaxed EMD through the oracle: relaxed_emd(yuv(style), yuv(pred), 'both')"""
    from oracle import strotss_oracle as O
    xt, yt = torch.as_tensor(x), torch.as_tensor(y)
    return float(O.relaxed_emd(O.convert_rgb_to_yuv(xt), O.convert_rgb_to_yuv(yt), "both"))


# ------------------------------------------------------------------ the cases and the bounds
def test_every_tie_free_case_holds_its_gap():
    for label in PC.ELEMENTWISE:
        c = PC.make_case(label)
        gap = PC.gap_of(c)
        print(f"MEASURE gap {label} {gap:.3e} after {c.row_seed - c.seed} tries")
        assert gap >= PC.MIN_GAP and c.row_seed - c.seed < PC.TRIES
        assert c.n_proj in (1, 8) or c.kind == "dup"
        assert c.ld in (32, 2208) and c.rgb_to_yuv in (0, 1)
    assert {(PC.make_case(lb).n, PC.make_case(lb).ns) for lb in PC.TIE_FREE} == \
        {(1, 1), (2, 1), (1, 64), (37, 64), (64, 37), (64, 64), (65, 33)}
    assert {c[4] for c in PC.SPECS} == {32, 2208} and {c[5] for c in PC.SPECS} == {0, 1}
    c = PC.make_case(PC.DUP_LABEL)
    assert np.array_equal(c.y[PC.DUP_PRED[0]], c.y[PC.DUP_PRED[1]]) and np.array_equal(c.x[PC.DUP_STYLE[0]], c.x[PC.DUP_STYLE[1]])
    assert PC.tie_shows(c)


def test_elementwise_cases_cover_every_sort_width():
    """S = the power of two >= max(n, ns), clamped to [64, 1024]: 0, 1, 3, 6 and 10 cross-wave stages"""
    def width(n, ns):
        return min(1024, max(64, 1 << (max(n, ns) - 1).bit_length()))
    by_width = {}
    for label, n, ns, P, ld, convert, kind in PC.SPECS:
        assert width(n, ns) == PC.width(n, ns)
        by_width.setdefault(width(n, ns), []).append((label, ld, convert))
    assert sorted(by_width) == [64, 128, 256, 512, 1024]
    assert {lb for S in (256, 512, 1024) for lb, _, _ in by_width[S]} == set(PC.CONSTRUCTED)
    for S in (512, 1024):
        assert {ld for _, ld, _ in by_width[S]} == {32, 2208} and {cv for _, _, cv in by_width[S]} == {0, 1}
    assert {(s[1], s[2], s[3]) for s in PC.SPECS if s[0] in PC.CONSTRUCTED} >= {
        (130, 130, 8), (256, 200, 8), (257, 512, 8), (512, 512, 8), (513, 300, 8), (1024, 1024, 8), (1024, 1024, 1),
        (1023, 1024, 8), (1024, 513, 8)}


@pytest.mark.parametrize("label", PC.CONSTRUCTED)
def test_constructed_cases_lie_on_their_line(label):
    c = PC.make_case(label)
    u = PC.line_direction(c.n_proj, c.rgb_to_yuv, c.seed)
    assert np.abs(u).max() == 1.0
    margin = PC.line_margin(u, c.n_proj, c.rgb_to_yuv)
    print(f"MEASURE line {label} margin {margin:.3f} gap {PC.gap_of(c):.3e}")
    assert margin >= (0.27 if c.rgb_to_yuv else 0.45)
    pts = np.concatenate([c.x, c.y])
    assert pts.min() >= 0.01 and pts.max() <= 0.99
    t = (pts - 0.5) @ u / (u @ u)
    assert np.abs(pts - 0.5 - t[:, None] * u[None, :]).max() <= 1e-15
    assert np.diff(np.sort(t)).min() >= 0.98 * 0.5 / len(t) * (1 - 1e-9), "neighbours are at least half a grid step apart"
    # the sides interleave: neither is a block of the line
    side = np.r_[np.zeros(c.ns), np.ones(c.n)][np.argsort(t)]
    assert np.count_nonzero(np.diff(side)) > min(c.n, c.ns) // 2
    if c.label == PC.INTEGER_LABEL:
        d0 = c.dirs[0].astype(np.float64)
        assert c.n_proj == 1 and not c.rgb_to_yuv and np.abs(np.cross(u, d0)).max() <= 1e-15


def test_float32_yardstick_is_what_is_pinned():
    worst = {}
    for label in PC.ELEMENTWISE:
        c = PC.make_case(label)
        l64, g64 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)
        l32, g32 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv, dtype=np.float32)
        e, rel = PR.err_over_max(g32, g64), abs(l32 - l64) / abs(l64)
        fam = PR.family(c)
        print(f"MEASURE err32 {label} {e:.3e} loss {rel:.3e} family {fam}")
        worst[fam] = max(worst.get(fam, 0.0), e)
        assert rel <= PR.LOSS_TOL
    assert set(worst) == set(PR.ERR32)
    for fam, e in worst.items():
        assert PR.ERR32[fam] / 4 <= e <= 2.0 * PR.ERR32[fam], (fam, e)
        assert PR.TOL_GRAD[fam] == 8.0 * PR.ERR32[fam]


@pytest.mark.parametrize("label", PC.FULL_LABELS)
def test_float32_yardstick_of_the_full_shapes_is_what_is_pinned(label):
    c = PC.make_full(label)
    l64, g64 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)
    l32, g32 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv, dtype=np.float32)
    e = PR.rel_fro(g32, g64)
    print(f"MEASURE fro32 {label} {e:.3e} loss {abs(l32 - l64) / abs(l64):.3e} gap {PC.gap_of(c):.3e}")
    assert PR.FRO32[label] / 4 <= e <= 2.0 * PR.FRO32[label] and PR.TOL_FRO[label] == 8.0 * PR.FRO32[label]
    assert abs(l32 - l64) <= PR.LOSS_TOL * abs(l64)


def test_full_shapes_are_the_stated_ones():
    assert sorted((s[1], s[2], s[3]) for s in PC.FULL) == sorted(
        [(1024, 1024, 64), (1024, 1024, 1024), (1000, 1024, 33), (768, 600, 64), (1024, 1, 64), (1, 1024, 64)])


MUTANTS = {"weights_1_over_max": dict(weights="max"), "no_scale": dict(scale=False), "m_for_m_transposed": dict(transpose=False),
           "descending_ties": dict(descending_ties=True)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_errors_fail_the_comparison(name):
    """in float64, the comparison of tests/test_hip_palette_sliced.py: every element within TOL_GRAD[family] of max|ref|"""
    caught = []
    for label in PC.ELEMENTWISE:
        c = PC.make_case(label)
        _, g64 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)
        _, gm = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv, **MUTANTS[name])
        if not (np.abs(gm - g64) <= PR.TOL_GRAD[PR.family(c)] * np.abs(g64).max()).all():
            caught.append(label)
    print(f"MEASURE mutant {name} caught on {caught}")
    # one atom against several: every overlap is 1 / max(n, ns) already, the two weightings coincide
    unequal = [s[0] for s in PC.SPECS if s[1] != s[2] and min(s[1], s[2]) > 1]
    if name == "descending_ties":             # only exact ties tell
        assert caught == [PC.DUP_LABEL]
    elif name == "weights_1_over_max":        # equal sizes have len_ij = 1 / n on the diagonal: only unequal ones tell
        assert set(caught) == set(unequal) and len(unequal) == 7 + 5
        assert {"line_n256_ns200_p8", "line_n257_ns512_p8", "line_n513_ns300_p8", "line_n1023_ns1024_p8",
                "line_n1024_ns513_p8"} <= set(unequal)
    elif name == "m_for_m_transposed":        # only where the matrix is applied
        assert set(caught) == {s[0] for s in PC.SPECS if s[5]}
    else:
        assert set(caught) == set(PC.ELEMENTWISE)


def _swap_slots(c, p, g64, tol):
    """the slots r >= S / 2 of direction p at which exchanging the sorted prediction ranks r and r + 1 moves some gradient
    element by more than tol of max|ref|, with the largest such move and the largest relative Frobenius size"""
    slots, worst, fro = [], 0.0, 0.0
    for r in range(PC.width(c.n, c.ns) // 2, c.n - 1):
        _, gm = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv, swap_rank=(p, r))
        moved = PR.err_over_max(gm, g64)
        if moved > tol:
            slots.append(r)
            worst, fro = max(worst, moved), max(fro, PR.rel_fro(gm, g64))
    return slots, worst, fro


def test_one_swapped_rank_at_full_width_is_caught_element_by_element():
    """Two adjacent sorted prediction ranks of ONE direction exchanged at a slot >= S / 2, planted in the float64 restatement.
    The coefficients are sums of +-len, so an exchange shows only where the two ranks' coefficients differ: at 14 of the 511
    upper slots of the randomly dealt 1024 x 1024 case (the first is slot 959) and at 375 of the pair-dealt one.  Where it
    shows it moves a gradient element by up to 0.37 (0.67 pair-dealt) of max|ref| at P = 8, against a TOL_GRAD of 9.6e-7.  In
    relative Frobenius norm the exchange is worth up to 1.6e-2, which does NOT fall under the full shapes' TOL_FRO (8.0e-7 at
    1024 x 1024, P = 64): the palette term's float32 yardstick is itself only 1e-7, so the norm comparison saw such an
    exchange already -- wherever float32 did not decide the sign itself.  What the constructed cases add for this term is
    the width S = 256, the element-wise bound at 512 and 1024, and inputs at which float32 decides no rank and no sign."""
    counts = {}
    for label in (PC.SWAP_LABEL, "line_n1024_ns1024_p8_pairs"):
        c = PC.make_case(label)
        assert (c.n, c.ns, PC.width(c.n, c.ns)) == (1024, 1024, 1024)
        _, g64 = PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)
        tol = PR.TOL_GRAD[PR.family(c)]
        slots, worst, fro = _swap_slots(c, 0, g64, tol)
        print(f"MEASURE swap {label}: {len(slots)} of {c.n - 1 - 512} slots show, first {slots[:3]}, max {worst:.3e} of tol "
              f"{tol:.3e}, fro {fro:.3e} of TOL_FRO {PR.TOL_FRO['full_n1024_ns1024_p64']:.3e}")
        counts[label] = len(slots)
        assert slots and slots[0] >= 512 and worst > tol
    assert counts["line_n1024_ns1024_p8_pairs"] > 510 // 3


# ------------------------------------------------------------------ the step's bounds
@pytest.mark.parametrize("lb", PS.LABELS)
def test_float32_step_stays_within_a_quarter_of_the_bounds(lb):
    r64 = PS.reference_step(lb)
    r32 = PS.reference_step(lb, torch.float32)
    sc, gr = PS.step_distance(r32, r64)
    print(f"MEASURE step32 {lb} scalar {sc:.3e} grad {gr:.3e} l_palette_sliced {float(r64['l_palette_sliced']):.4f}")
    assert float(r64["l_palette_sliced"]) > 0
    assert sc <= PS.TOL_SCALAR / 4 and gr <= PS.GRAD_TOL / 4


def test_step_table_covers_what_it_claims():
    rows = PS.TABLE
    assert {r[0] for r in rows} == {"remd", "sliced"} and {r[1] for r in rows} == {"one", "regions", "blend"}
    assert {r[2] for r in rows} == {False, True} and {r[4] for r in rows} == {(64, 64), (42, 64)}
    for t in ("remd", "sliced"):
        assert {r[1] for r in rows if r[0] == t} == {"one", "regions", "blend"}


# ------------------------------------------------------------------ command line
def _args(*extra, tmp=None):
    import run_strotss as RS
    base = [str(tmp / "no_content.jpg"), str(tmp / "no_style.jpg"), "-o", str(tmp / "out.jpg")] if tmp is not None else ["c", "s"]
    return RS.build_parser().parse_args(base + list(extra))


def test_parser_and_keywords():
    import run_strotss as RS
    from nn import engine as E
    assert E.PALETTE_TRANSPORTS == ("remd", "sliced")
    assert E.DEFAULT_PALETTE_PROJECTIONS == 64 and E.PALETTE_MAX_PROJECTIONS == 1024
    assert _args().palette_transport == "remd" and _args().palette_projections is None
    assert RS._palette_transport_input(_args()) == {}, "a run without the flag builds the engine it always built"
    assert RS._palette_transport_input(_args("--palette_transport", "remd")) == {}
    assert RS._palette_transport_input(_args("--palette_transport", "sliced")) == \
        dict(palette_transport="sliced", palette_projections=64)
    assert RS._palette_transport_input(_args("--palette_transport", "sliced", "--palette_projections", "1024", "--seed", "7")) == \
        dict(palette_transport="sliced", palette_projections=1024)
    flags = {n for names, _ in RS._FLAGS for n in names}
    assert {"--palette_transport", "--palette_projections"} <= flags
    assert "--palette_transport" in RS.__doc__ and "--palette_projections" in RS.__doc__
    help_text = RS.build_parser().format_help()
    assert "not tuned" in " ".join(help_text.split())
    # every style transport goes with it
    for t in ("remd", "sinkhorn", "sliced"):
        a = _args("--palette_transport", "sliced", "--style_transport", t)
        assert dict(RS._style_transport_input(a), **RS._palette_transport_input(a))["palette_transport"] == "sliced"


PT = ["--palette_transport", "sliced"]
REFUSALS = [(["--palette_projections", "32"], "--palette_projections needs --palette_transport sliced"),
            (["--palette_transport", "remd", "--palette_projections", "32"], "--palette_projections needs"),
            (PT + ["--palette_projections", "0"], "--palette_projections must be a whole number in 1..1024"),
            (PT + ["--palette_projections", "1025"], "--palette_projections must be"),
            (PT + ["--palette_projections", "-3"], "--palette_projections must be"),
            (PT + ["--strips"], "--strips")]


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
    with pytest.raises(ValueError, match="--palette_transport sliced runs on one GPU"):
        RS.run(_args(*PT, tmp=tmp_path))
    assert not (tmp_path / "out.jpg").exists()


def test_engine_argument_check():
    from nn import engine as E
    E.check_palette_transport("remd")
    E.check_palette_transport("sliced")
    E.check_palette_transport("sliced", 1)
    E.check_palette_transport("remd", np.int64(1024))
    for bad in (0, 1025, -1, 2.5, True, "32", None):
        with pytest.raises(ValueError, match="palette_projections"):
            E.check_palette_transport("sliced", bad)
    for bad in ("sinkhorn", "", None, 1):
        with pytest.raises(ValueError, match="palette_transport"):
            E.check_palette_transport(bad)
    import inspect
    sig = inspect.signature(E.StepEngine.__init__).parameters
    assert sig["palette_transport"].default == "remd" and sig["palette_projections"].default == 64


# ------------------------------------------------------------------ ABI
def test_header_declares_table_lists_and_library_exports_the_entries():
    import ctypes
    from test_abi_exports import declared_symbols
    from nn import _hip
    syms = declared_symbols()
    for name in ("strotss_palette_sliced_workspace_bytes", "strotss_palette_sliced_fwd_bwd"):
        assert name in syms and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["strotss_palette_sliced_fwd_bwd"][1]) == 14
    assert len(_hip.SIGNATURES["strotss_palette_sliced_workspace_bytes"][1]) == 3
    assert sorted(_hip.SIGNATURES) == syms and _hip.ABI_VERSION == 8
    so = os.path.join(ROOT, "strotss-tensorflow_amd", "libstrotss_hip.so")
    if os.path.exists(so):                    # built trees: the symbols resolve (tests/test_abi_exports.py holds the full match)
        lib = ctypes.CDLL(so)
        assert lib.strotss_palette_sliced_fwd_bwd
        ver = lib.strotss_abi_version
        ver.restype = ctypes.c_int
        assert ver() == 8
        q = lib.strotss_palette_sliced_workspace_bytes
        q.restype, q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
        assert q(1024, 1024, 1024) >= 1024 * 1024 * 4 and q(1, 1, 1) > 0
        for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-1, 1, 1), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025)):
            assert q(*bad) == 0, bad
