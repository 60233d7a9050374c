"""Region clustering without a GPU: the float64 restatement (tests/_cluster_ref.py) against itself --
the objective never decreases, the planted labels come back exactly, farthest-first breaks ties toward the lowest index, the
upsampled masks partition the image -- the margin conditions on the data of the GPU tests (those tests are exact, not
statistical), the refusals of the two C entries before any launch, and the parser / refusals of --auto_masks."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _cluster_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G, H = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000)   # aligned, never touched
ODD = C.c_void_p(0x10004)                                                                          # not 16-byte aligned
NULL = None


# ------------------------------------------------------------------ 1. the restatement
def test_the_bound_at_the_two_widths():
    assert abs(R.assign_bound(2179) - 2.6e-4) < 0.05e-4
    assert abs(R.assign_bound(35) - 4.4e-6) < 0.05e-6


@pytest.mark.parametrize("case", R.PLANTED)
def test_planted_labels_come_back_and_every_margin_is_wide(case):
    """the condition of the GPU test of spherical_kmeans: no row's float64 margin is within E at any of the 1 + 16
    assignments, so the kernels' labels must EQUAL the reference's; and the reference finds the planted labels"""
    n, d, k = case[:3]
    x, planted = R.planted_rows(*case)
    out = R.planted_result(case)
    E = R.assign_bound(d)
    assert len(out["margins"]) == R.ITERS + 1 and len(out["objective"]) == R.ITERS
    shares = [float((m <= E).mean()) for m in out["margins"]]
    print(f"planted n {n} d {d} k {k}: smallest margin {min(float(m.min()) for m in out['margins']):.3f}, E {E:.2e}")
    assert max(shares) == 0.0
    assert all(b >= a for a, b in zip(out["objective"], out["objective"][1:]))       # never decreases
    assert R.same_partition(out["label"], planted, k)
    assert out["count"].sum() == n and (out["count"] > 0).all()


@pytest.mark.parametrize("case", R.UNSTRUCTURED)
def test_unstructured_margins_and_objective(case):
    """the condition of the GPU tests on unstructured rows: at the centres those tests use (the reference's after its 16
    iterations) at most 5 % of the rows have a float64 margin within E"""
    n, d, k = case[:3]
    out = R.planted_result(case)
    E = R.assign_bound(d)
    share = float((out["margins"][-1] <= E).mean())
    print(f"unstructured n {n} d {d} k {k}: {100 * share:.2f} % of the rows within E = {E:.2e}")
    assert share <= 0.05
    assert all(b >= a - 1e-15 for a, b in zip(out["objective"], out["objective"][1:]))


def test_update_keeps_an_empty_cluster_and_skips_foreign_labels():
    x, _ = R.planted_rows(40, 35, 3, 1.0, 5)
    inv = R.inv_norm(x, 40)
    start = np.random.default_rng(0).random((4, 35))
    label = np.array([0, 2] * 20, dtype=np.int32)
    label[7], label[8] = 9, -1                                       # outside 0..3: skipped
    centres, count = R.update(x, inv, label, 40, 35, 4, start)
    assert count.tolist() == [19, 0, 19, 0]                     # rows 7 (a 2) and 8 (a 0) left
    assert np.array_equal(centres[1], start[1]) and np.array_equal(centres[3], start[3])
    assert np.allclose(np.linalg.norm(centres[[0, 2]], axis=1), 1.0, rtol=0, atol=1e-15)


def test_farthest_first_takes_the_lowest_index_on_ties():
    rows = np.zeros((32, 32), dtype=np.float32)
    rows[:6, :3] = [[1, 0, 0], [0, 1, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [0, 0, 1]]
    inv = R.inv_norm(rows, 6)
    _, chosen = R.farthest_first(rows, inv, 6, 3, 3)
    assert chosen == [0, 1, 4]                                       # rows 0 / 3, 1 / 2 and 4 / 5 tie pairwise
    same = np.zeros((32, 32), dtype=np.float32)
    same[:5, :3] = [0.2, 0.5, 0.1]
    _, chosen = R.farthest_first(same, R.inv_norm(same, 5), 5, 3, 3)
    assert chosen == [0, 0, 0]                                       # one constant colour: every centre is row 0
    label, best, second, _ = R.assign(same, R.inv_norm(same, 5), 5, 3, np.tile(same[:1, :3] / np.linalg.norm(same[0]), (3, 1)))
    assert label.tolist() == [0] * 5 and np.array_equal(best, second)


def test_assign_zero_rows_and_one_centre():
    x, _ = R.planted_rows(9, 3, 2, 1.0, 1)
    x[4] = 0
    inv = R.inv_norm(x, 9)
    inv[5] = 0
    centres, _ = R.farthest_first(x, inv, 9, 3, 2)
    label, best, second, _ = R.assign(x, inv, 9, 3, centres)
    assert label[4] == 0 and best[4] == 0 and second[4] == 0         # a zero row: every score is 0, the lowest j
    assert label[5] == 0 and best[5] == 0 and second[5] == 0         # inv_norm == 0
    _, _, second, _ = R.assign(x, inv, 9, 3, centres[:1])
    assert np.isneginf(second[[0, 1, 2, 3, 6, 7, 8]]).all()


@pytest.mark.parametrize("hw", [(21, 32), (1, 1), (300, 7)])
def test_upsampled_masks_partition_the_image(hw):
    H, W = hw
    for gh, gw in ((5, 9), (1, 1), (64, 43)):
        grid = np.random.default_rng(gh * 100 + gw).integers(0, 3, size=(gh, gw))
        labels = R.upsample_labels(grid, H, W)
        assert labels.shape == (H, W)
        for y, x in ((0, 0), (H - 1, W - 1), (H // 2, W // 3)):
            assert labels[y, x] == grid[min(y * gh // H, gh - 1), min(x * gw // W, gw - 1)]
        masks = R.masks_from_labels(labels, 3)
        assert all(m.shape == (H, W, 1) and m.dtype == np.float32 for m in masks)
        assert np.array_equal(sum(masks), np.ones((H, W, 1), dtype=np.float32))


def test_grid_has_at_most_64_points_a_side():
    for h, w in ((192, 256), (256, 171), (42, 64), (1, 1), (65, 3), (255, 256)):
        ys, xs = R.grid_points(h, w)
        g = -(-max(h, w) // 64)
        assert 1 <= len(ys) <= 64 and 1 <= len(xs) <= 64 and ys[0] == xs[0] == g // 2
        assert ys[-1] < h and xs[-1] < w
    from nn import strotss_utils as U
    for h, w in ((192, 256), (42, 64), (1, 1)):
        assert all(np.array_equal(a, b) for a, b in zip(U.auto_mask_grid(h, w), R.grid_points(h, w)))
    assert (U.AUTO_MASK_ITERS, U.AUTO_MASK_SIZE, U.AUTO_MASK_MIN_SHARE) == (R.ITERS, 256, 1 / 32)
    assert [tuple(c) for c in U.MASK_COLOURS] == R.CORNER_COLOURS == sorted(R.CORNER_COLOURS)


# ------------------------------------------------------------------ 2. the C ABI refuses before it launches
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_abi_version_is_unchanged(lib):
    from nn import _hip
    assert lib.strotss_abi_version() == 8 == _hip.ABI_VERSION
    assert _hip.KMEANS_MAX_K == 16


def test_workspace_bytes(lib):
    size = lib.strotss_kmeans_update_workspace_bytes
    assert size(1, 32, 1) == 1 * 1 * 32 * 8                          # one row block
    assert size(64, 32, 2) == 2 * 32 * 8 and size(65, 32, 2) == 2 * 2 * 32 * 8
    assert size(8192, 2208, 16) == 32 * 16 * 2208 * 8 == size(2 ** 17 + 37, 2208, 16)      # 32 row blocks at most
    for bad in ((0, 32, 1), (-1, 32, 1), (8, 0, 1), (8, 33, 1), (8, 32, 0), (8, 32, 17), (2 ** 26, 64, 1)):
        assert size(*bad) == 0, bad


def test_kmeans_assign_refuses_bad_arguments(lib):
    call = lambda x=P, inv=Q, n=8, d=35, ld=64, c=G, k=3, lab=H, best=P, second=Q: \
        lib.strotss_kmeans_assign(x, inv, n, d, ld, c, k, lab, best, second, NULL)
    for name in ("x", "inv", "c", "lab", "best", "second"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(n=0) == EINVAL and call(n=-4) == EINVAL
    assert call(d=0) == EINVAL and call(d=65) == EINVAL
    assert call(n=2 ** 26, ld=64) == EINVAL                          # n ld > INT_MAX
    assert call(k=0) == EINVAL and call(k=17) == EINVAL and call(k=-1) == EINVAL
    assert call(ld=48) == EALIGN and call(d=3, ld=4) == EALIGN


def test_kmeans_update_refuses_bad_arguments(lib):
    nbytes = lib.strotss_kmeans_update_workspace_bytes(8, 64, 3)
    assert nbytes == 3 * 64 * 8
    call = lambda x=P, inv=Q, lab=H, n=8, d=35, ld=64, k=3, c=G, count=P, ws=Q, nb=nbytes: \
        lib.strotss_kmeans_update(x, inv, lab, n, d, ld, k, c, count, ws, nb, NULL)
    for name in ("x", "inv", "lab", "c", "count", "ws"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(n=0) == EINVAL and call(n=-4) == EINVAL
    assert call(d=0) == EINVAL and call(d=65) == EINVAL
    assert call(n=2 ** 26, ld=64, nb=2 ** 62) == EINVAL
    assert call(k=0) == EINVAL and call(k=17, nb=2 ** 62) == EINVAL
    assert call(nb=nbytes - 1) == EINVAL and call(nb=0) == EINVAL
    assert call(ld=48, nb=2 ** 62) == EALIGN


# ------------------------------------------------------------------ 3. the command line
def test_parser_knows_the_two_flags():
    import argparse
    import run_strotss as RS
    parser = RS.build_parser()
    ns = parser.parse_args(["c.jpg", "s.jpg"])
    assert ns.auto_masks is None and ns.save_masks is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "5", "--save_masks", "out"])
    assert ns.auto_masks == 5 and ns.save_masks == "out"
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "2.5"])
    for flag in ("--auto_masks", "--save_masks"):
        assert flag in RS.__doc__
    assert RS._auto_masks_input(parser.parse_args(["c.jpg", "s.jpg"])) is None
    assert RS._auto_masks_input(ns) == (5, "out")
    assert RS._auto_masks_input(parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "2"])) == (2, None)
    assert RS._auto_masks_input(parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "8"])) == (8, None)
    assert RS._auto_masks_input(argparse.Namespace()) is None       # a namespace from before the flags existed


REFUSALS = [(["--auto_masks", "1"], "2..8"), (["--auto_masks", "9"], "2..8"), (["--auto_masks", "0"], "2..8"),
            (["--auto_masks", "-3"], "2..8"), (["--save_masks", "dir"], "needs --auto_masks"),
            (["--auto_masks", "3", "--content_mask", "cm.png", "--style_mask", "sm.png"], "--content_mask"),
            (["--auto_masks", "3", "--style_mask", "sm.png"], "--content_mask"),
            (["--auto_masks", "3", "--style_mix", "other.jpg"], "--style_mix"),
            (["--auto_masks", "3", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_auto_masks_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out.jpg"
    with pytest.raises(ValueError, match=match):
        RS.run(RS.build_parser().parse_args([str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(out)]
                                            + extra))
    assert not out.exists() and not (tmp_path / "dir").exists()


def test_auto_masks_is_refused_with_video_and_on_several_ranks(monkeypatch, tmp_path):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    video = [str(tmp_path / "no_frames"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    with pytest.raises(ValueError, match="--video"):
        RS.run(RS.build_parser().parse_args(video + ["--auto_masks", "3"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    single = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(single + ["--auto_masks", "3"]))
    assert not (tmp_path / "out").exists() and not (tmp_path / "out.jpg").exists()
