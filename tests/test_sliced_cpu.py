"""CPU checks of the sliced Wasserstein style term: the host twin of the direction bits, the float64
restatement's properties, what tests/test_hip_sliced.py holds the GPU to -- every tie-free case's gap, torch's own float32
run within the pinned yardsticks, each planted error caught, the float32 run of the whole step within a quarter of the
step's bounds -- the command line's flags and refusals, and the two new entries in the header and in nn/_hip.py."""
import os

import numpy as np
import pytest
import torch

import _sliced_cases as SC
import _sliced_ref as SR
import _transport_cases as TC
import _transport_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ------------------------------------------------------------------ the direction bits
def test_signs_are_plus_minus_one_and_depend_on_every_input():
    from nn import rand
    s = rand.sliced_signs(5, 2, 7, 300)
    assert s.shape == (7, 300) and set(np.unique(s)) == {-1.0, 1.0}
    assert abs(float(s.mean())) < 0.1
    assert len({tuple(r) for r in s}) == 7, "directions differ"
    assert not np.array_equal(s, rand.sliced_signs(5, 3, 7, 300)) and not np.array_equal(s, rand.sliced_signs(6, 2, 7, 300))
    assert not np.array_equal(s, rand.sliced_signs(5 + (1 << 32), 2, 7, 300)), "the key's high word counts"
    # a prefix in d and in the direction count: the bits of (p, k) do not depend on the matrix's size
    assert np.array_equal(s[:3, :35], rand.sliced_signs(5, 2, 3, 35))


def test_sign_bits_are_the_documented_philox_bits():
    """bit k & 31 of word (k >> 5) & 3 of philox4x32_10(ctr = (k >> 7, 2, t, p), key = seed); eight literal bits at two points,
    computed from philox4x32_10 once"""
    from nn import rand
    for seed, t, p, k in ((0, 0, 0, 0), (7, 5, 3, 299), ((9 << 32) | 5, 2, 1, 130), (1, 1 << 20, 1023, 2178)):
        word = int(rand.philox4x32_10(k >> 7, 2, t, p, seed & 0xFFFFFFFF, seed >> 32)[(k >> 5) & 3])
        assert rand.sliced_signs(seed, t, p + 1, k + 1)[p, k] == (1.0 if (word >> (k & 31)) & 1 else -1.0)
    assert rand.sliced_signs(0, 0, 1, 8)[0].tolist() == PINNED[0]
    assert rand.sliced_signs(0x123456789A, 17, 6, 2179)[5, 2171:2179].tolist() == PINNED[1]


PINNED = ([1.0, 1.0, -1.0, -1.0, 1.0, -1.0, 1.0, 1.0], [1.0, -1.0, -1.0, -1.0, -1.0, 1.0, 1.0, 1.0])


def test_sign_blocks_are_disjoint_from_the_index_draws():
    """the index draw uses counters (j >> 2, 0, t, 0) and (0, 1, t, 0); the directions (k >> 7, 2, t, p): another c1.  The
    words differ where c0, c2, c3 and the key agree"""
    from nn import rand
    for t in (0, 3):
        mine = [int(w) for w in rand.philox4x32_10(0, 2, t, 0, 11, 0)]
        for c1 in (0, 1):
            theirs = [int(w) for w in rand.philox4x32_10(0, c1, t, 0, 11, 0)]
            assert not set(mine) & set(theirs)
    stream = rand.PhiloxStream(11, 3)
    first = int(stream.keys(4)[0])
    assert first == int(rand.philox4x32_10(0, 0, 3, 0, 11, 0)[0]) and first not in mine


# ------------------------------------------------------------------ the restatement
SHAPES = sorted({(s[1], s[2]) for s in SC.SPECS} | {(s[1], s[2]) for s in SC.FULL})


@pytest.mark.parametrize("n,ns", SHAPES)
def test_overlaps_are_a_coupling_of_the_uniform_marginals(n, ns):
    m = SR.len_matrix(n, ns)
    assert m.sum() == n * ns and (m.sum(1) == ns).all() and (m.sum(0) == n).all() and (m >= 0).all()
    I, J, _ = SR.overlaps(n, ns)
    assert len(I) <= n + ns - 1 and np.bincount(I).max() <= -(-ns // n) + 1
    # the definition, entry by entry
    i, j = np.arange(n)[:, None], np.arange(ns)[None, :]
    assert np.array_equal(m, np.maximum(0, np.minimum((i + 1) * ns, (j + 1) * n) - np.maximum(i * ns, j * n)))


def test_permuted_rows_give_zero_loss_and_gradient():
    c = SC.make_case("n64_ns64_p8")
    perm = np.random.default_rng(1).permutation(c.n)
    loss, g = SR.sliced(c.y[perm], c.y, c.signs)
    assert loss == 0.0 and not g.any()


def test_equal_sizes_agree_with_plain_rank_matching():
    c = SC.make_case("n130_ns130_p4")
    s = torch.as_tensor(c.signs, dtype=torch.float64)
    a = torch.sort(SR.projections(torch.as_tensor(c.y), s), dim=1)[0]
    b = torch.sort(SR.projections(torch.as_tensor(c.x), s), dim=1)[0]
    plain = float(((a - b) ** 2).sum() / c.n / (2 * c.n_proj))
    assert abs(SR.sliced(c.x, c.y, c.signs)[0] - plain) <= 1e-14 * plain


def test_expectation_over_directions_is_the_cosine_cost_of_the_coupling():
    """n = ns = 1: E[(a - b)^2] / 2 = 1 - cos(x, s); 4096 directions hold it to a few per cent"""
    rng = np.random.default_rng(2)
    x, y = SC._rows(rng, 1, 35), SC._rows(rng, 1, 35)
    loss = SR.sliced(x, y, SR.signs_of(0, 0, 4096, 35))[0]
    cos = float(x[0] @ y[0] / np.linalg.norm(x[0]) / np.linalg.norm(y[0]))
    assert abs(loss - (1.0 - cos)) <= 0.05 * (1.0 - cos)


def test_gradient_matches_a_finite_difference():
    c = SC.make_case("n65_ns40_p4")
    _, g = SR.sliced(c.x, c.y, c.signs)
    rng = np.random.default_rng(3)
    h = 1e-7                                  # far below the case's gap: no rank changes
    for _ in range(6):
        dy = rng.standard_normal(c.y.shape)
        up, down = SR.sliced(c.x, c.y + h * dy, c.signs)[0], SR.sliced(c.x, c.y - h * dy, c.signs)[0]
        fd, an = (up - down) / (2 * h), float((g * dy).sum())
        assert abs(fd - an) <= 1e-6 * max(abs(an), 1e-6), (fd, an)


# ------------------------------------------------------------------ the cases and the bounds
def test_every_tie_free_case_holds_its_gap():
    for label in SC.ELEMENTWISE:
        c = SC.make_case(label)
        gap = SC.gap_of(c)
        print(f"MEASURE gap {label} {gap:.3e} after {c.row_seed - c.seed} tries")
        assert gap >= SC.MIN_GAP and c.row_seed - c.seed < SC.TRIES
    c = SC.make_case(SC.SIGN_LABEL)
    a = SR.projections(torch.as_tensor(c.y), torch.as_tensor(c.signs, dtype=torch.float64))
    assert float(a[0, 0]) == 0.0 and bool((a[0] < 0).any()) and bool((a[0] > 0).any())
    c = SC.make_case(SC.DUP_LABEL)
    assert np.array_equal(c.y[SC.DUP_PRED[0]], c.y[SC.DUP_PRED[1]]) and np.array_equal(c.x[SC.DUP_STYLE[0]], c.x[SC.DUP_STYLE[1]])
    c = SC.make_case(SC.ARC_DUP_LABEL)
    i, j = SC.ARC_DUP
    assert np.array_equal(c.y[i], c.y[j]) and np.array_equal(c.x[i], c.x[j]) and i // 64 != j // 64


def test_elementwise_cases_cover_every_sort_width():
    """S = the power of two >= max(n, ns), clamped to [64, 1024]: 0, 1, 3, 6 and 10 cross-wave stages"""
    def width(n, ns):
        return min(1024, max(64, 1 << (max(n, ns) - 1).bit_length()))
    assert [width(*m) for m in ((1, 1), (64, 3), (65, 1), (128, 128), (129, 2), (256, 256), (257, 1), (512, 512), (513, 1),
                                (1024, 1024))] == [64, 64, 128, 128, 256, 256, 512, 512, 1024, 1024]
    by_width = {}
    for label, n, ns, d, P, kind in SC.SPECS:
        assert width(n, ns) == SC.width(n, ns)
        by_width.setdefault(width(n, ns), []).append(label)
    assert sorted(by_width) == [64, 128, 256, 512, 1024]
    assert set(by_width[512] + by_width[1024]) == set(SC.CONSTRUCTED) and len(SC.CONSTRUCTED) == 10
    assert {(s[1], s[2], s[3]) for s in SC.SPECS if s[0] in SC.CONSTRUCTED} >= {
        (257, 512, 3), (512, 512, 35), (513, 300, 35), (1024, 1024, 3), (1024, 1024, 35), (1023, 1024, 3), (1024, 513, 35),
        (1024, 1, 3), (1, 1024, 35)}


@pytest.mark.parametrize("label", SC.CONSTRUCTED)
def test_constructed_cases_sort_in_both_directions(label):
    """the projection of an arc row falls with its angle where the direction's first sign is +1 and rises where it is -1:
    every case holds both, and two such directions sort the rows in exactly opposite orders"""
    c = SC.make_case(label)
    s = c.signs
    assert c.n_proj >= 4 and set(s[:, 0]) == {-1.0, 1.0}
    if c.kind == "arc_dup":
        return
    rows = c.y if c.n > 1 else c.x
    a = SR.projections(torch.as_tensor(rows), torch.as_tensor(s, dtype=torch.float64)).numpy()
    up, down = int(np.flatnonzero(s[:, 0] < 0)[0]), int(np.flatnonzero(s[:, 0] > 0)[0])
    assert np.array_equal(np.argsort(a[up]), np.argsort(a[down])[::-1])
    theta = np.arctan2(rows[:, 1], rows[:, 0])
    assert SC.ARC_LO < theta.min() and theta.max() < SC.ARC_HI and np.array_equal(np.argsort(a[up]), np.argsort(theta))
    norms = np.linalg.norm(rows, axis=1)
    assert norms.max() / norms.min() > 1.5 or len(rows) < 8, "the reciprocal norms differ"


def test_float32_yardstick_is_what_is_pinned():
    worst = {}
    for label in SC.ELEMENTWISE:
        c = SC.make_case(label)
        l64, g64 = SR.sliced(c.x, c.y, c.signs)
        l32, g32 = SR.sliced(c.x, c.y, c.signs, torch.float32)
        e, rel = SR.err_over_max(g32, g64), abs(l32 - l64) / abs(l64)
        fam = SR.family(c)
        print(f"MEASURE err32 {label} {e:.3e} loss {rel:.3e} family {fam}")
        worst[fam] = max(worst.get(fam, 0.0), e)
        assert rel <= TR.TOL_SCALAR
    for fam, e in worst.items():
        assert SR.ERR32[fam] / 4 <= e <= 2.0 * SR.ERR32[fam], (fam, e)
        assert SR.TOL_GRAD[fam] == 8.0 * SR.ERR32[fam]


@pytest.mark.parametrize("label", SC.FULL_LABELS)
def test_float32_yardstick_of_the_full_shapes_is_what_is_pinned(label):
    c = SC.make_full(label)
    l64, g64 = SR.sliced(c.x, c.y, c.signs)
    l32, g32 = SR.sliced(c.x, c.y, c.signs, torch.float32)
    e = SR.rel_fro(g32, g64)
    print(f"MEASURE fro32 {label} {e:.3e} loss {abs(l32 - l64) / abs(l64):.3e} gap {SR.min_gap(c.x, c.y, c.signs):.3e}")
    assert SR.FRO32[label] / 4 <= e <= 2.0 * SR.FRO32[label] and SR.TOL_FRO[label] == 8.0 * SR.FRO32[label]
    assert abs(l32 - l64) <= TR.TOL_SCALAR * abs(l64)


MUTANTS = {"weights_1_over_max": dict(weights="max"), "no_half": dict(half=False), "descending_ties": dict(descending_ties=True)}


@pytest.mark.parametrize("name", list(MUTANTS))
def test_planted_errors_fail_the_comparison(name):
    """in float64, the comparison of tests/test_hip_sliced.py: every element within TOL_GRAD[family] of max|ref|"""
    caught = []
    for label in SC.ELEMENTWISE:
        c = SC.make_case(label)
        _, g64 = SR.sliced(c.x, c.y, c.signs)
        _, gm = SR.sliced(c.x, c.y, c.signs, **MUTANTS[name])
        if not (np.abs(gm - g64) <= SR.TOL_GRAD[SR.family(c)] * np.abs(g64).max()).all():
            caught.append(label)
    print(f"MEASURE mutant {name} caught on {caught}")
    if name == "descending_ties":             # only exact ties tell
        assert caught == [SC.DUP_LABEL, SC.ARC_DUP_LABEL]
    elif name == "weights_1_over_max":        # equal sizes have len_ij = 1 / n on the diagonal: only unequal ones tell
        assert "n65_ns40_p4" in caught and "n3_ns200_p2" in caught and "n64_ns64_p8" not in caught
        assert {"arc_n257_ns512_p8", "arc_n513_ns300_p4", "arc_n1023_ns1024_p4", "arc_n1024_ns513_p4"} <= set(caught)
        assert "arc_n1024_ns1024_p4" not in caught
    else:
        assert set(caught) == set(SC.ELEMENTWISE)


def test_one_swapped_rank_at_full_width_is_caught_element_by_element():
    """Two adjacent sorted prediction ranks of ONE direction exchanged at a slot >= S / 2 -- what a cross-wave exchange that
    reads a slot one stage late leaves behind -- planted in the float64 restatement.  At the constructed 1024 x 1024 case the
    swap moves a gradient element by 6.4e-2 .. 3.3e-1 of max|ref|, against the family's TOL_GRAD of 4.9e-3: the element-wise
    comparison catches it.  The same swap at the full-shape case 1024 x 1024, P = 256 is worth 5.4e-5 of relative Frobenius
    norm, a hundredth of that case's TOL_FRO of 5.4e-3: the norm comparison, the only one the suite held at this width
    before, lets it pass."""
    c = SC.make_case(SC.SWAP_LABEL)
    assert (c.n, c.ns, SC.width(c.n, c.ns)) == (1024, 1024, 1024)
    _, g64 = SR.sliced(c.x, c.y, c.signs)
    tol = SR.TOL_GRAD[SR.family(c)]
    for r in (512, 777, 1022):
        _, gm = SR.sliced(c.x, c.y, c.signs, swap_rank=(1, r))
        moved = SR.err_over_max(gm, g64)
        print(f"MEASURE swap {c.label} slot {r}: max {moved:.3e} of tol {tol:.3e}, fro {SR.rel_fro(gm, g64):.3e}")
        assert moved > tol
        assert np.count_nonzero(np.abs(gm - g64).max(1)) == 2, "two rows move, no other"
    label = "full_n1024_ns1024_p256"
    f = SC.make_full(label)
    _, g64 = SR.sliced(f.x, f.y, f.signs)
    _, gm = SR.sliced(f.x, f.y, f.signs, swap_rank=(1, 777))
    fro = SR.rel_fro(gm, g64)
    print(f"MEASURE swap {label} slot 777: fro {fro:.3e} of TOL_FRO {SR.TOL_FRO[label]:.3e}, max {SR.err_over_max(gm, g64):.3e}")
    assert 0.0 < fro < SR.TOL_FRO[label], "the gap the constructed cases close"


# ------------------------------------------------------------------ the step's bounds
def test_float32_step_stays_within_a_quarter_of_the_bounds():
    worst_s = worst_g = 0.0
    for label, h, w, n, seed, masked in SC.STEPS + [SC.BLEND_STEP]:
        blend = SC.BLEND_WEIGHTS if label == SC.BLEND_STEP[0] else None
        P = TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None, n_styles=2 if blend else 1)
        if masked:                           # the first region has ns != n
            assert (len(P["s_idx"][0][0]), len(P["idx"][0])) == (600, 768) and len(P["idx"][1]) == 1024
        r64 = SR.reference_step(P, SC.STEP_PROJECTIONS, SC.STEP_SEED, blend_weights=blend)
        r32 = SR.reference_step(P, SC.STEP_PROJECTIONS, SC.STEP_SEED, torch.float32, blend_weights=blend)
        sc, gr = TR.step_distance(r32, r64)
        print(f"MEASURE step32 {label} scalar {sc:.3e} grad {gr:.3e}")
        worst_s, worst_g = max(worst_s, sc), max(worst_g, gr)
    assert worst_s <= SR.TOL_SCALAR / 4 and worst_g <= SR.GRAD_TOL / 4


# ------------------------------------------------------------------ command line
def _args(*extra, tmp=None):
    import run_strotss as RS
    base = [str(tmp / "no_content.jpg"), str(tmp / "no_style.jpg"), "-o", str(tmp / "out.jpg")] if tmp is not None else ["c", "s"]
    return RS.build_parser().parse_args(base + list(extra))


def test_parser_and_keywords():
    import run_strotss as RS
    from nn import engine as E
    assert E.STYLE_TRANSPORTS == ("remd", "sinkhorn", "sliced")
    assert E.DEFAULT_SLICED_PROJECTIONS == 256 and E.SLICED_MAX_PROJECTIONS == 1024
    assert _args().sliced_projections is None
    # what the other transports returned before the flag existed, key for key
    assert RS._style_transport_input(_args()) == dict(style_transport="remd", sinkhorn_l=10.0, sinkhorn_iters=30)
    assert RS._style_transport_input(_args("--style_transport", "sinkhorn", "--sinkhorn_reg", "4.5")) == \
        dict(style_transport="sinkhorn", sinkhorn_l=4.5, sinkhorn_iters=30)
    assert RS._style_transport_input(_args("--style_transport", "sliced")) == \
        dict(style_transport="sliced", sinkhorn_l=10.0, sinkhorn_iters=30, sliced_projections=256, sliced_seed=0)
    assert RS._style_transport_input(_args("--style_transport", "sliced", "--sliced_projections", "32", "--seed", "7")) == \
        dict(style_transport="sliced", sinkhorn_l=10.0, sinkhorn_iters=30, sliced_projections=32, sliced_seed=7)
    assert "--sliced_projections" in {n for names, _ in RS._FLAGS for n in names}
    assert RS._LOGGED["sliced"] == "l_sliced"

    class Eng:
        style_transport = "sliced"
    assert RS._logged_terms(Eng) == ("loss", "loss_c", "loss_s", "sliced")
    Eng.style_transport = "remd"
    assert RS._logged_terms(Eng) == ("loss", "loss_c", "loss_s")


SW = ["--style_transport", "sliced"]
REFUSALS = [(["--sliced_projections", "32"], "--sliced_projections needs --style_transport sliced"),
            (["--style_transport", "sinkhorn", "--sliced_projections", "32"], "--sliced_projections needs"),
            (SW + ["--sliced_projections", "0"], "--sliced_projections must be a whole number in 1..1024"),
            (SW + ["--sliced_projections", "1025"], "--sliced_projections must be"),
            (SW + ["--sinkhorn_reg", "5"], "--sinkhorn_reg and --sinkhorn_iters need --style_transport sinkhorn"),
            (SW + ["--sinkhorn_iters", "5"], "--sinkhorn_reg and --sinkhorn_iters need"),
            (SW + ["--strips"], "--strips")]


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
    with pytest.raises(ValueError, match="--style_transport sliced runs on one GPU"):
        RS.run(_args(*SW, tmp=tmp_path))
    assert not (tmp_path / "out.jpg").exists()


def test_engine_argument_check():
    from nn import engine as E
    E.check_style_transport("sliced", 10.0, 30)
    E.check_style_transport("sliced", 10.0, 30, 1)
    E.check_style_transport("remd", 10.0, 30, np.int64(1024))
    for bad in (0, 1025, -1, 2.5, True, "32", None):
        with pytest.raises(ValueError, match="sliced_projections"):
            E.check_style_transport("sliced", 10.0, 30, bad)


# ------------------------------------------------------------------ ABI
def test_header_declares_table_lists_and_library_exports_the_entries():
    import ctypes
    from test_abi_exports import declared_symbols
    from nn import _hip
    syms = declared_symbols()
    for name in ("strotss_sliced_workspace_bytes", "strotss_sliced_cos_fwd_bwd"):
        assert name in syms and name in _hip.SIGNATURES
    assert len(_hip.SIGNATURES["strotss_sliced_cos_fwd_bwd"][1]) == 20
    assert len(_hip.SIGNATURES["strotss_sliced_workspace_bytes"][1]) == 4
    assert sorted(_hip.SIGNATURES) == syms and _hip.ABI_VERSION == 8
    so = os.path.join(ROOT, "strotss-tensorflow_amd", "libstrotss_hip.so")
    if os.path.exists(so):                    # built trees: the symbols resolve (tests/test_abi_exports.py holds the full match)
        lib = ctypes.CDLL(so)
        assert lib.strotss_sliced_workspace_bytes and lib.strotss_sliced_cos_fwd_bwd
        q = lib.strotss_sliced_workspace_bytes
        q.restype, q.argtypes = ctypes.c_size_t, [ctypes.c_int] * 4
        assert q(1024, 1024, 2208, 256) > 0 and q(1025, 1, 64, 1) == 0 and q(1, 1, 48, 1) == 0 and q(1, 1, 64, 1025) == 0
