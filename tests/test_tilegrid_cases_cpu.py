"""CPU half of the tile-grid sweeps (tests/_tilegrid_cases.py): the case lists enumerate what they claim, the grouped
sweep reaches the kinds of grid it is meant to reach, and the float64 references can tell a misplaced tile."""
import numpy as np

import _loss_ref as LR
import _tilegrid_cases as TG


# ------------------------------------------------------------------ the sweeps enumerate what they claim
def test_every_grid_is_present_in_every_variant():
    want = {(g, gs) for g in range(1, 17) for gs in range(1, 34)}
    assert len(want) == 528
    for v in TG.VARIANTS:
        cases = TG.cosine_cases(v)
        assert len(cases) == 528 and {(g, gs) for g, gs, _, _ in cases} == want
        for g, gs, n, ns in cases:
            assert (TG.tiles(n), TG.tiles(ns)) == (g, gs), (v, g, gs, n, ns)
            assert 1 <= n <= TG.N_PRED == 1024 and 1 <= ns <= TG.N_STYLE == 2112


def test_both_edge_variants_at_every_grid():
    exact = {(g, gs): (n, ns) for g, gs, n, ns in TG.cosine_cases("exact")}
    single = {(g, gs): (n, ns) for g, gs, n, ns in TG.cosine_cases("single")}
    mixed = {(g, gs): (n, ns) for g, gs, n, ns in TG.cosine_cases("mixed")}
    for key in exact:
        g, gs = key
        assert exact[key] == (64 * g, 64 * gs)                              # last tile full on both sides
        assert single[key] == (64 * (g - 1) + 1, 64 * (gs - 1) + 1)         # one row / one column in the last tile
        n, ns = mixed[key]
        assert 2 <= n - 64 * (g - 1) <= 63 and 2 <= ns - 64 * (gs - 1) <= 63
    # the mixed offsets are not all alike, and cover odd counts and counts that are no multiple of 4
    offs = {n % 64 for _, _, n, _ in TG.cosine_cases("mixed")} | {ns % 64 for _, _, _, ns in TG.cosine_cases("mixed")}
    assert len(offs) >= 16 and any(o % 2 for o in offs) and any(o % 4 for o in offs)
    assert TG.cosine_cases("mixed") == TG.cosine_cases("mixed")             # seeded


def test_symmetric_cases_cover_every_g():
    cases = TG.symm_cases()
    for v in TG.VARIANTS:
        assert sorted(g for vv, g, _ in cases if vv == v) == list(range(1, 17))
    assert all(TG.tiles(n) == g for _, g, n in cases)


def test_output_buffer_layout():
    assert TG.SENTINEL_BITS >> 23 == 0xFF and TG.SENTINEL_BITS & 0x400000 and TG.SENTINEL_BITS & 0x3FFFFF    # quiet NaN + payload
    assert np.isnan(np.array([TG.SENTINEL_BITS], dtype=np.uint32).view(np.float32)[0])
    assert TG.SENTINEL_BITS < 2 ** 31                                       # fits an int32 fill
    assert TG.D_SWEEP == 35 and TG.pad32(TG.D_SWEEP) == 64


# ------------------------------------------------------------------ coverage accounting of the grouped sweep
def test_grouped_sweep_reaches_blocked_and_row_order_grids():
    cases = TG.group_cases()
    assert len(cases) == 64 and set(cases) == {(n, ns) for n in (1, 37, 63, 64, 65, 449, 1000, 1024)
                                               for ns in (33, 64, 65, 300, 777, 1024, 1500, 2048)}
    kinds = {}
    for n, ns in cases:
        kinds.setdefault(TG.host_block(TG.tiles(n), TG.tiles(ns))[2], []).append((n, ns))
    assert len(kinds.get("blocked", [])) >= 8 and len(kinds.get("rows_mod8", [])) >= 8, {k: len(v) for k, v in kinds.items()}
    # blocks of more than one tile row AND of more than one tile column occur, and so does a single-row block
    shapes = {TG.host_block(TG.tiles(n), TG.tiles(ns))[:2] for n, ns in kinds["blocked"]}
    assert any(bh > 1 and bw > 1 for bh, bw in shapes) and any(bh == 1 for bh, bw in shapes) and any(bw == 1 for bh, bw in shapes)
    # the symmetric pair's share of the grid ends off a multiple of 8 workgroups (the next problem starts at a padded offset)
    assert any(TG.pad8(TG.symm_workgroups(n)) != TG.symm_workgroups(n) for n, _ in cases)
    assert any(TG.pad8(TG.symm_workgroups(n)) == TG.symm_workgroups(n) for n, _ in cases)


def test_a_grid_of_a_multiple_of_8_tiles_always_blocks():
    """The host's fall-back to row order 'because no (bh, bw) divides the grid' cannot be reached: with g gs % 8 == 0 take
    a = 2^min(v2(g), 3) and b = 8 / a; then a | g, b | gs, and bh = g / a, bw = gs / b is a divisor pair with bh bw = tiles / 8.
    So a launch is blocked exactly when its tile count is a multiple of 8, and the sweeps need no third kind of grid."""
    for g in range(1, 65):
        for gs in range(1, 65):
            bh, bw, kind = TG.host_block(g, gs)
            assert kind == ("rows_mod8" if (g * gs) % 8 else "blocked"), (g, gs, kind)
            if kind == "blocked":
                assert bh * bw * 8 == g * gs and g % bh == 0 and gs % bw == 0


def test_blend_cases_end_problems_off_a_multiple_of_8():
    assert {len(ns) for _, ns in TG.BLEND_CASES} == {1, 2, 3, 4}
    assert {n for n, _ in TG.BLEND_CASES} >= {37, 1000}
    assert (37, (65, 1000, 129, 2048)) in TG.BLEND_CASES and (1000, (2048, 64, 777)) in TG.BLEND_CASES
    ragged = 0
    for n, ns in TG.BLEND_CASES:
        inner = [TG.tiles(n) * TG.tiles(s) for s in ns[:-1]]               # every problem but the last is followed by another
        ragged += sum(1 for t in inner if t % 8)
        assert all(33 <= s <= 2048 for s in ns) and len(ns) == len(set(ns))
    assert ragged >= 6
    w, g = TG.BLEND_WEIGHTS, TG.GROUP_G
    assert abs(sum(w) - 1.0) < 1e-15
    for a in w:                                                              # g * w is exact in f32 on both sides
        for b in g:
            assert float(np.float32(a) * np.float32(b)) == a * b


# ------------------------------------------------------------------ the references can tell a misplaced tile
def test_no_two_rows_of_a_sweep_matrix_are_close():
    pred, style = TG.sweep_rows()
    assert pred.shape == (1024, 35) and style.shape == (2112, 35)
    assert TG.SEPARATION == 100.0 * LR.EPS_COST
    for x in (pred, style):
        D = LR.cos_dist(x, x)
        np.fill_diagonal(D, np.inf)
        assert D.min() > TG.SEPARATION, D.min()
        assert (x >= 0).all() and (np.linalg.norm(x, axis=1) > 1e-3).all()


def test_a_misplaced_or_transposed_tile_is_visible():
    """every 64 x 64 tile of the reference differs from every other tile of its tile row and tile column, and from its own
    transpose, by far more than EPS_COST in most entries: a tile written in another's place cannot pass"""
    cross, self_ = TG.sweep_refs()
    assert cross.shape == (1024, 2112) and self_.shape == (1024, 1024)
    assert not cross.flags.writeable and not self_.flags.writeable
    assert cross.min() > 0.0 and cross.max() - cross.min() > 0.5          # spread over most of [0, 1]
    T = cross.reshape(16, 64, 33, 64).transpose(0, 2, 1, 3)               # (g, gs, 64, 64)
    worst = 1.0
    for i in range(16):
        for j in range(33):
            others = np.concatenate([np.delete(T[i], j, 0), np.delete(T[:, j], i, 0), T[i, j].T[None]])
            frac = (np.abs(others - T[i, j]) > 100.0 * LR.EPS_COST).mean(axis=(1, 2))
            worst = min(worst, frac.min())
    assert worst > 0.9, worst
    assert np.abs(np.diag(self_)).max() < 1e-12 and np.array_equal(self_, self_.T)


def test_group_and_moment_rows():
    y, c, x = TG.group_rows()
    assert y.shape == c.shape == (1024, 67) and x.shape == (2048, 67)
    assert not np.array_equal(y, c)
    assert [TG.pad32(d) // 128 + (TG.pad32(d) % 128 > 0) for d in TG.MOMENT_D] == [1, 1, 2, 3, 5, 8, 11, 15, 18]
    assert {TG.pad32(d) % 128 == 0 for d in TG.MOMENT_D} == {True, False}   # exact and ragged last tiles
    for d in (35, 259):
        xs, yp = TG.moment_rows(d)
        assert xs.shape == yp.shape == (96, d)
        bc, bm = TG.cov_bound(xs, 96)
        _, S = LR.moment_stats(xs)
        # the bound is a rounding bound: far below what a misplaced covariance tile changes
        assert bc.shape == (d, d) and (bc > 0).all() and bc.max() < 1e-3 * np.abs(S).max()
        assert bm.shape == (d,) and (bm > 0).all()
    assert TG.cov_terms(96) == 6 * 96 + 5
