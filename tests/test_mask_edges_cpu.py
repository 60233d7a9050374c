"""The mask kernels' edge cases without a GPU ("Mask kernel edges"): every case of
tests/_mask_edge_cases.py reaches the edge it claims (computed from the kernels' own formulas, restated), the LDS footprint of
refine_vote_kernel stays inside its array for every size up to 64 x 160 at the largest radius, the references alone meet the caps
on ambiguous pixels and rows, the stand-ins without a plant pass the comparisons the GPU file calls, and each planted error
fails them -- by the margin printed."""
import os
import sys
import time

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as KR  # noqa: E402
import _mask_edge_cases as M  # noqa: E402
import _refine_ref as R  # noqa: E402
import _track_ref as TR  # noqa: E402

SMALL = [name for name in M.REFINE_CASES if name != "walks"]


# ------------------------------------------------------------------ 1. refinement
@pytest.mark.parametrize("name", M.REFINE_CASES)
def test_refine_case_reaches_its_footprint(name):
    (h, w, gh, gw, k), radius, kind, seed, claim, _ = M.REFINE_CASES[name]
    fh, fw = M.footprints(h, w, gh, gw, radius)
    assert len(fh) == -(-h // M.RF_TILE_H) and len(fw) == -(-w // M.RF_TILE_W)
    assert (max(fh), max(fw)) == claim
    assert max(fh) <= M.RF_FOOT_H and max(fw) <= M.RF_FOOT_W
    trips = -(-max(fh) * max(fw) // M.RF_THREADS)
    print(f"{name}: footprints fh {sorted(set(fh))} x fw {sorted(set(fw))}, {max(fh) * max(fw)} cells at most = {trips} trips")


def test_refine_cases_reach_the_edges_claimed():
    fp = {name: M.footprints(*c[0][:4], c[1]) for name, c in M.REFINE_CASES.items()}
    for name in ("full-k16", "full-k5"):                              # an INTERIOR tile holds the whole array: three trips
        fh, fw = fp[name]
        assert fh[1] * fw[1] == 640 == M.RF_FOOT_H * M.RF_FOOT_W and -(-640 // M.RF_THREADS) == 3
        assert M.REFINE_CASES[name][0][1] % M.RF_TILE_W == 4 and fw[-1] == 8      # a 4-pixel last tile column: 4 + 4 cells
    assert max(fp["trip2-r2"][0]) * max(fp["trip2-r2"][1]) == 432 > M.RF_THREADS
    assert M.REFINE_CASES["trip2-r2"][1] == R.RADIUS
    for name in ("ragged-r4", "ragged-r3"):                           # cells of one or two pixels; fh differs among tile rows
        h, w, gh, gw = M.REFINE_CASES[name][0][:4]
        for n, g in ((h, gh), (w, gw)):
            sizes = np.diff(TR.cell_starts(g, n))
            assert set(sizes.tolist()) == {1, 2}
        assert len(set(fp[name][0][1:-1])) >= 2 or len(set(fp[name][0])) >= 3
    assert [M.REFINE_CASES[n][0][4] for n in M.REFINE_CASES] == [16, 5, 8, 4, 9, 3]       # KP = 16, 8, 8, 4, 16, 4
    h, w, gh, gw = M.REFINE_CASES["walks"][0][:4]
    tiles, cells, groups, one_pass = M.refine_counts(h, w, gh, gw)
    assert (tiles, cells, h * w) == (16385, 98313, 393240)
    assert groups == M.RF_MAX_GRID < tiles and one_pass == 4 * M.RF_MAX_GRID < cells
    # the existing shapes reach none of this: at most 84 staged cells at radius 2 and 35 at radius 4, one trip each
    for (shape, radius, _) in R.CASES:
        fh, fw = M.footprints(*shape[:4], radius)
        assert max(fh) * max(fw) <= M.RF_THREADS and M.refine_counts(*shape[:4])[0] <= M.RF_MAX_GRID


def test_footprint_fits_the_lds_array_at_every_size():
    """rows: every gh <= h <= 64; columns: every gw <= w <= 160; radius 4.  The two axes are independent in the kernel"""
    worst_h = max(f for h in range(1, 65) for gh in range(1, h + 1) for _, f in M.axis_footprints(h, gh, M.RF_MAX_RADIUS, M.RF_TILE_H))
    worst_w = max(f for w in range(1, 161) for gw in range(1, w + 1) for _, f in M.axis_footprints(w, gw, M.RF_MAX_RADIUS, M.RF_TILE_W))
    print(f"largest footprint over the sweep: {worst_h} x {worst_w} cells, the array holds {M.RF_FOOT_H} x {M.RF_FOOT_W}")
    assert worst_h == M.RF_FOOT_H and worst_w == M.RF_FOOT_W         # reached and never passed
    for n, g in ((64, 64), (64, 37), (160, 160), (131080, 32771)):    # first cell + cells stays inside the grid
        for tile in (M.RF_TILE_H, M.RF_TILE_W):
            assert all(lo >= 0 and lo + f <= g for lo, f in M.axis_footprints(n, g, M.RF_MAX_RADIUS, tile))


@pytest.mark.parametrize("name", M.REFINE_CASES)
def test_refine_reference_alone_meets_the_cap_on_ambiguous_pixels(name):
    t0 = time.time()
    img, grid, ref, (k, radius, sigma_s, sigma_r) = M.refine_case(name)
    share = M.ambiguous_share(ref, sigma_r)
    print(f"{name}: {100 * share:.4f} % of the pixels admit more than one label (cap {100 * M.AMBIGUOUS_CAP} %); reference in "
          f"{time.time() - t0:.1f} s; labels {np.bincount(ref['label'].reshape(-1), minlength=k).tolist()}")
    assert share <= M.AMBIGUOUS_CAP
    assert (np.bincount(grid.reshape(-1), minlength=k) > 0).all() and (ref["best"] > 0).all()
    assert 0 <= img.min() and img.max() <= 1 and sigma_s == radius / 2 and sigma_r in (R.SIGMA_R, R.SIGMA_RANGE[1])


@pytest.mark.parametrize("name", SMALL)
def test_refine_standin_passes_and_its_plants_fail(name):
    img, grid, ref, (k, radius, sigma_s, sigma_r) = M.refine_case(name)
    fig = M.refine_figures(M.refine_standin(img, grid, k, radius, sigma_s, sigma_r), ref, k, sigma_r)
    assert M.refine_failures(fig) == [], fig
    origin = M.refine_figures(M.refine_standin(img, grid, k, radius, sigma_s, sigma_r, "origin"), ref, k, sigma_r)
    print(f"{name}: footprint origin off by one cell row: best {origin['best']:.3g} of its bound, {origin['inadmissible']} labels")
    assert origin["best"] > 100 and M.refine_failures(origin)
    stage = M.refine_figures(M.refine_standin(img, grid, k, radius, sigma_s, sigma_r, "stage256"), ref, k, sigma_r)
    print(f"{name}: staging stops after 256 cells: best {stage['best']:.3g} of its bound, {stage['inadmissible']} labels")
    assert stage["best"] > 100 and stage["inadmissible"] > 0 and M.refine_failures(stage)


def test_refine_standin_equals_the_reference_on_the_existing_shapes():
    """the tile-by-tile stand-in is a second statement of the votes: on _refine_ref.SHAPES (but the 1024 x 683 one, 2752 tiles of
    Python) it gives the reference's labels and votes"""
    for case in R.CASES[:5] + R.CASES[6:]:
        (h, w, gh, gw, k), radius, sigma_r = case
        img, grid, ref = R.case_result(case)
        got = M.refine_standin(img, grid, k, radius, R.SIGMA_S, sigma_r)
        assert M.refine_failures(M.refine_figures(got, ref, k, sigma_r)) == [] and np.array_equal(got["label"], ref["label"])


def test_a_tile_walk_that_stops_fails():
    img, grid, ref, (k, radius, sigma_s, sigma_r) = M.refine_case("walks")
    assert M.refine_failures(M.refine_figures(M.refine_walk_standin(img, grid, ref, k), ref, k, sigma_r)) == []
    fig = M.refine_figures(M.refine_walk_standin(img, grid, ref, k, "walk_stops"), ref, k, sigma_r)
    print(f"walk stops after {M.RF_MAX_GRID} tiles: {fig['unwritten']} pixels never written, best {fig['best']:.3g} of its bound")
    assert fig["unwritten"] == 8 * 3 == fig["inadmissible"] and not fig["count_ok"] and len(M.refine_failures(fig)) >= 3


# ------------------------------------------------------------------ 2. assignment
def test_assign_ranges_sit_on_the_kernel_edges():
    assert {d % 256 for d in M.ASSIGN_D} >= {252, 255, 0, 1, 4} and {d // 512 for d in M.ASSIGN_D} == {0, 1, 2}
    assert [M.kp_of(k) for k in M.ASSIGN_K] == [4, 8, 8, 16, 16]
    assert [(-(-n // 32), n % 32) for n in M.ASSIGN_N] == [(1, 31), (1, 0), (2, 1), (3, 1)]
    for d in M.ASSIGN_D:
        x, inv, c32, prior = M.assign_data(d, 5)
        ld = KR.pad32(d)
        assert x.shape == (96, ld) and c32.shape == (5, ld) and not x[:, d:].any() and np.isposinf(c32[:, d:]).all()
        assert (d % 4 == 0) == (d in (252, 256, 260, 508, 512, 516, 1024))      # the others end inside a float4


@pytest.mark.parametrize("d", M.ASSIGN_D)
def test_assign_references_meet_the_cap_and_the_standin_passes(d):
    E = KR.assign_bound(d)
    worst = np.inf
    for k in M.ASSIGN_K:
        x, inv, c32, prior = M.assign_data(d, k)
        for n in M.ASSIGN_N:
            for pr, beta in ((None, 0.0), (prior, M.ASSIGN_BETA)):
                ref = M.assign_reference(x, inv, n, d, c32, pr, beta)
                margin = M.assign_margin(ref[3])
                worst = min(worst, float(margin.min()))
                assert float((margin <= E).mean()) <= M.ASSIGN_AMBIGUOUS_CAP
                assert len(set(ref[0].tolist())) == k or pr is not None          # every centre wins a row: none may be lost
                fig = M.assign_figures(M.assign_standin(x, inv, n, d, c32, k, pr, beta), ref, d)
                assert M.assign_failures(fig) == [], (k, n, beta, fig)
            plain = M.assign_reference(x, inv, n, d, c32)
            zero = M.assign_reference(x, inv, n, d, c32, prior, 0.0)
            none = M.assign_reference(x, inv, n, d, c32, np.full_like(prior, -1), M.ASSIGN_BETA)
            assert all(np.array_equal(a, b) for a, b in zip(zero[:3], plain[:3]))
            assert all(np.array_equal(a, b) for a, b in zip(none[:3], plain[:3]))
    print(f"d {d}: smallest margin {worst:.3e}, E {E:.2e}")


def test_assign_plants_fail():
    rows = []
    for d, k, n, plant in ((257, 5, 33, "half"), (512, 5, 33, "half"), (1027, 16, 65, "half"), (255, 4, 31, "unmasked"),
                           (513, 9, 65, "unmasked"), (1027, 16, 33, "unmasked"), (256, 5, 32, "kp"), (516, 9, 33, "kp"),
                           (1024, 16, 65, "kp")):
        x, inv, c32, prior = M.assign_data(d, k)
        for pr, beta in ((None, 0.0), (prior, M.ASSIGN_BETA)):
            ref = M.assign_reference(x, inv, n, d, c32, pr, beta)
            fig = M.assign_figures(M.assign_standin(x, inv, n, d, c32, k, pr, beta, plant), ref, d)
            rows.append((plant, d, k, n, beta, fig))
            print(f"{plant} d {d} k {k} n {n} beta {beta}: best {fig['best']:.3g} of its tolerance, {fig['inadmissible']} labels "
                  f"not admissible")
            assert M.assign_failures(fig), (plant, d, k, n)
            if plant == "kp":
                assert fig["inadmissible"] > 0
            else:
                assert fig["best"] > 100
    # a second half that is not there cannot be dropped: d = 252 and 256 pass the plant, which is why 257 and 260 are cases
    for d in (252, 256):
        x, inv, c32, prior = M.assign_data(d, 5)
        ref = M.assign_reference(x, inv, 33, d, c32)
        assert M.assign_failures(M.assign_figures(M.assign_standin(x, inv, 33, d, c32, 5, plant="half"), ref, d)) == []


# ------------------------------------------------------------------ 3. update
def test_update_ranges_sit_on_the_kernel_edges():
    assert [M.row_blocks(n) for n in M.UPDATE_N] == [(1, 63), (1, 64), (2, 33), (32, 64), (32, 65), (32, 67)]
    assert [-(-d // 256) for d in M.UPDATE_D] == [1, 1, 2, 3] and [d % 256 for d in M.UPDATE_D] == [255, 0, 1, 1]
    for n in M.UPDATE_N:                                              # the ignored labels sit in the first and the last block
        x, inv, label, start, want, count = M.update_data(255, n, 5)
        nb, rows = M.row_blocks(n)
        assert label[5] == 5 and label[6] == -1 and label[n - 3] == 5 and label[n - 2] == -1 and (n - 3) // rows == nb - 1
        assert count[4] == 0 and count[:4].all() and count.sum() == n - 4 and (start[:, 255:] == 7).all()


@pytest.mark.parametrize("d", M.UPDATE_D)
def test_update_standin_passes_and_a_skipped_block_fails(d):
    for n in M.UPDATE_N:
        for k in M.UPDATE_K:
            x, inv, label, start, want, want_count = M.update_data(d, n, k)
            centres, count = M.update_standin(x, inv, label, n, d, k, start)
            fig = M.update_figures(centres, count, want, want_count, start, d)
            assert M.update_failures(fig) == [], (n, k, fig)
            if n >= 65:
                centres, count = M.update_standin(x, inv, label, n, d, k, start, "last_block")
                fig = M.update_figures(centres, count, want, want_count, start, d)
                if k == 5:
                    print(f"last row block skipped, d {d} n {n} k {k}: centres {fig['centres']:.3g} of their bound")
                assert fig["centres"] > 100 and M.update_failures(fig), (n, k)


# ------------------------------------------------------------------ 4. label warp
@pytest.mark.parametrize("shape", M.WARP_EDGE_SHAPES)
def test_warp_edge_cases_are_exact_and_reach_the_borders(shape):
    h, w, gh, gw = shape
    cells = gh * gw
    assert cells > 256 and cells % 256 != 0                           # full workgroups and a ragged one
    assert all(c % 256 == 0 or c < 256 for c in (a * b for _, _, a, b in TR.WARP_SHAPES))      # which no shape had
    for name, grid, flow, cert in M.warp_edge_cases(h, w, gh, gw):
        a = TR.label_warp(grid, TR.WARP_K, flow, cert, np.float32)
        assert np.array_equal(a, TR.label_warp(grid, TR.WARP_K, flow, cert, np.float64)), name
        if name == "huge-none":
            assert (a == -1).all()
        if name in ("border-y-none", "border-x-none"):
            axis, g, n = (0, gh, h) if "y" in name else (1, gw, w)
            kept = np.moveaxis(a, axis, 0) >= 0
            valid = (grid >= 0) & (grid < TR.WARP_K)
            for i in range(g):
                if i % 4 in (1, 3):                                   # one pixel outside: no prior
                    assert not kept[i].any(), (name, i)
                else:                                                 # row 0 or row n - 1 of the earlier frame: its cell's label
                    src = np.moveaxis(grid, axis, 0)[0 if i % 4 == 0 else g - 1]
                    assert np.array_equal(np.moveaxis(a, axis, 0)[i], np.where((src >= 0) & (src < TR.WARP_K), src, -1)), (name, i)
            assert valid.any() and kept.any()
