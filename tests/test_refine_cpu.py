"""Mask refinement without a GPU: the float64 restatement (tests/_refine_ref.py) against itself -- the
margin conditions on the data of the GPU tests (those tests are exact, not statistical), what the vote does on constant and
two-colour images, the point of the feature on an edge that runs through the cells -- the refusals of the C entry before any
launch, and the parser / refusals of --refine_masks and --refine_sigma."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _refine_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G, H, S = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))   # aligned, never touched
ODD = C.c_void_p(0x10004)                                                                # not 16-byte aligned
NULL = None


# ------------------------------------------------------------------ 1. the restatement
def test_the_bound_at_three_sigmas():
    assert abs(R.vote_eps(1.0) - 1.79e-7) < 0.01e-7
    assert abs(R.vote_eps(0.1) - 1.79e-5) < 0.01e-5
    assert abs(R.vote_eps(0.01) - 1.79e-3) < 0.01e-3
    assert R.bound(2.0, 0.1) == 2 * R.vote_eps(0.1) * 2.0 + 1e-300 and R.bound(-np.inf, 0.1) == 1e-300


def test_constants_match_the_product():
    from nn import strotss_utils as U
    assert (U.REFINE_RADIUS, U.REFINE_SIGMA_S, U.REFINE_SIGMA_R) == (R.RADIUS, R.SIGMA_S, R.SIGMA_R) == (2, 1.0, 0.1)
    assert U.REFINE_SIGMA_RANGE == R.SIGMA_RANGE == (0.01, 1.0)
    assert U.REFINE_SIGMA_R ** 2 == pytest.approx(U.DEFAULT_SMOOTH_EPS)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_every_margin_of_the_planted_cases_is_wide(case):
    """the condition of the GPU comparison: no pixel's float64 margin is within E, so the kernel's labels must EQUAL these"""
    (Hh, W, gh, gw, k), radius, sigma_r = case
    img, grid, out = R.case_result(case)
    assert img.shape == (Hh, W, 3) and grid.shape == (gh, gw) and 0 <= img.min() and img.max() <= 1
    margin = out["best"] - out["second"]
    E = R.bound(out["best"], sigma_r)
    finite = np.isfinite(out["second"])
    smallest = float((margin[finite] / out["best"][finite]).min()) if finite.any() else float("inf")
    print(f"{R.case_id(case)}: smallest margin {smallest:.3e} of best, E {2 * R.vote_eps(sigma_r):.2e} of best, "
          f"{int((out['label'] != R.upsample_labels(grid, Hh, W)).sum())} of {Hh * W} labels differ from nearest neighbour")
    assert int((margin <= E).sum()) == 0
    assert (out["best"] > 0).all() and out["count"].sum() == Hh * W


def test_unstructured_margins():
    """a uniform-noise image with random labels: the share of pixels within E is printed and at most 5 %"""
    (Hh, W, gh, gw, k), radius, sigma_r = R.UNSTRUCTURED
    img, grid, out = R.case_result(R.UNSTRUCTURED)
    share = float(((out["best"] - out["second"]) <= R.bound(out["best"], sigma_r)).mean())
    print(f"unstructured {R.case_id(R.UNSTRUCTURED)}: {100 * share:.3f} % of the pixels within E = "
          f"{2 * R.vote_eps(sigma_r):.2e} of best")
    assert share <= 0.05


def test_cell_means_are_the_means_of_the_cells_own_pixels():
    rng = np.random.default_rng(3)
    img = rng.random((33, 47, 3)).astype(np.float32)
    m = R.cell_means(img, 5, 7)
    nn = R.upsample_labels(np.arange(35).reshape(5, 7), 33, 47)
    for cell in (0, 11, 34):
        assert np.allclose(m.reshape(-1, 3)[cell], img[nn == cell].astype(np.float64).mean(axis=0), rtol=0, atol=1e-15)
    assert np.array_equal(R.cell_means(img, 33, 47), img.astype(np.float64))       # one pixel per cell


def test_constant_image_votes_by_position_alone():
    """colour factor 1 everywhere: a lone wrong cell inside a uniform neighbourhood is voted away; a straight boundary
    between two half-planes stays where it is; a pixel exactly between two cells goes to the lower label"""
    img = np.full((40, 40, 3), 0.5, dtype=np.float32)
    grid = np.zeros((10, 10), dtype=np.int32)
    grid[4, 6] = 1
    out = R.refine(img, grid, 2)
    assert not out["label"].any() and out["count"].tolist() == [1600, 0]
    assert R.upsample_labels(grid, 40, 40).sum() == 16
    half = np.zeros((10, 10), dtype=np.int32)
    half[:, 5:] = 1
    out = R.refine(img, half, 2)
    assert np.array_equal(out["label"], R.upsample_labels(half, 40, 40))
    # 2 x 2 pixels on a 1 x 2 grid ... the pixel centres sit at v = -0.25 and 0.75; on a 1 x 3 image over a 1 x 2 grid the
    # middle pixel sits at v = 0.5, exactly between the cells: equal votes, the lower label
    out = R.refine(np.full((1, 3, 3), 0.25, dtype=np.float32), np.array([[1, 0]], dtype=np.int32), 2)
    assert out["vote"][0, 1, 0] == out["vote"][0, 1, 1] and out["label"].tolist() == [[1, 0, 0]]
    assert out["best"][0, 1] == out["second"][0, 1]


def test_absent_and_foreign_labels():
    img = np.full((6, 6, 3), 0.5, dtype=np.float32)
    grid = np.full((6, 6), 2, dtype=np.int32)
    grid[0, 0] = 7                                                    # outside 0..3: no vote, no index
    grid[5, 5] = -1
    out = R.refine(img, grid, 4)
    assert (out["label"] == 2).all() and np.isneginf(out["second"]).all()       # labels 0, 1, 3 are absent: they cannot win
    assert out["vote"][0, 0, 2] < out["vote"][3, 3, 2]                           # the corner lost a cell's vote
    out = R.refine(img, np.full((6, 6), 9, dtype=np.int32), 4)
    assert not out["label"].any() and np.isneginf(out["best"]).all()


def test_refined_labels_follow_a_colour_edge_that_cuts_through_the_cells():
    """the point of the feature: a two-colour image whose edge runs through the middle of a column of cells, every cell
    labelled by its majority colour -- every pixel's refined label is its own colour's, the nearest-neighbour label is not"""
    Hh = W = 64
    dark, light = (0.2, 0.2, 0.2), (0.8, 0.8, 0.8)
    own = (np.arange(W) >= 29).astype(np.int32)[None, :].repeat(Hh, axis=0)      # the edge: 5 dark + 3 light columns in cell 3
    img = np.where(own[..., None] == 1, light, dark).astype(np.float32)
    grid = np.zeros((8, 8), dtype=np.int32)
    grid[:, 4:] = 1                                                   # cell column 3 is mostly dark: label 0
    out = R.refine(img, grid, 2)
    nearest = R.upsample_labels(grid, Hh, W)
    assert np.array_equal(out["label"], own)
    assert int((nearest != own).sum()) == 3 * Hh and (nearest[:, 29:32] == 0).all()
    assert out["count"].tolist() == [29 * Hh, 35 * Hh]


# ------------------------------------------------------------------ 2. the C ABI refuses before it launches
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_the_two_symbols_are_exported_and_the_abi_version_is_unchanged(lib):
    from nn import _hip
    assert lib.strotss_abi_version() == 8 == _hip.ABI_VERSION
    for name in ("strotss_refine_labels_workspace_bytes", "strotss_refine_labels"):
        assert name in _hip.SIGNATURES and hasattr(C.CDLL(_hip.LIB_PATH), name)
    assert _hip.REFINE_MAX_RADIUS == 4


def test_workspace_bytes(lib):
    size = lib.strotss_refine_labels_workspace_bytes
    assert size(1, 1, 1, 1) == 256                                    # 12 bytes, in 256-byte slices
    assert size(1024, 683, 64, 43) == 64 * 43 * 12 == 33024
    assert size(1024, 1024, 64, 64) == 64 * 64 * 12
    assert size(7, 5, 7, 5) == 512
    for bad in ((0, 5, 1, 1), (5, 0, 1, 1), (-1, 5, 1, 1), (5, 5, 0, 1), (5, 5, 1, 0), (5, 5, 6, 1), (5, 5, 1, 6), (5, 5, -2, 1),
                (2 ** 15, 2 ** 15, 4, 4)):
        assert size(*bad) == 0, bad


def test_refine_labels_refuses_bad_arguments(lib):
    nbytes = lib.strotss_refine_labels_workspace_bytes(33, 47, 5, 7)
    assert nbytes == 512
    inf, nan = float("inf"), float("nan")

    def call(img=P, h=33, w=47, grid=Q, gh=5, gw=7, k=3, radius=2, sigma_s=1.0, sigma_r=0.1, label=G, best=H, second=S,
             count=P, ws=Q, nb=nbytes):
        return lib.strotss_refine_labels(img, h, w, grid, gh, gw, k, radius, sigma_s, sigma_r, label, best, second, count, ws, nb,
                                         NULL)
    for name in ("img", "grid", "label", "count", "ws"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    for name in ("best", "second"):                                   # optional, but aligned when given
        assert call(**{name: ODD}) == EALIGN, name
    big = 2 ** 62
    assert call(h=0, nb=big) == EINVAL and call(w=-3, nb=big) == EINVAL and call(gh=0, nb=big) == EINVAL and call(gw=0, nb=big) == EINVAL
    assert call(gh=34, nb=big) == EINVAL and call(gw=48, nb=big) == EINVAL
    assert call(h=2 ** 15, w=2 ** 15, nb=big) == EINVAL               # 3 h w > INT_MAX
    assert call(k=0) == EINVAL and call(k=17) == EINVAL and call(k=-1) == EINVAL
    assert call(radius=0) == EINVAL and call(radius=5) == EINVAL and call(radius=-2) == EINVAL
    for name in ("sigma_s", "sigma_r"):
        for bad in (0.0, -0.1, inf, nan, 1e-200):
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert call(nb=nbytes - 1) == EINVAL and call(nb=0) == EINVAL


# ------------------------------------------------------------------ 3. the command line
def test_parser_knows_the_two_flags():
    import argparse
    import run_strotss as RS
    parser = RS.build_parser()
    ns = parser.parse_args(["c.jpg", "s.jpg"])
    assert ns.refine_masks is False and ns.refine_sigma is None
    assert RS._refine_masks_input(ns) is None and RS._auto_masks_input(ns) is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "5", "--refine_masks"])
    assert ns.refine_masks is True and RS._refine_masks_input(ns) == 0.1 and RS._auto_masks_input(ns) == (5, None)
    ns = parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "5", "--refine_masks", "--refine_sigma", "0.05", "--save_masks", "d"])
    assert ns.refine_sigma == 0.05 and RS._refine_masks_input(ns) == 0.05 and RS._auto_masks_input(ns) == (5, "d")
    for edge in ("0.01", "1"):
        ns = parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "2", "--refine_masks", "--refine_sigma", edge])
        assert RS._refine_masks_input(ns) == float(edge)
    ns = parser.parse_args(["c.jpg", "s.jpg", "--auto_masks", "5"])
    assert RS._refine_masks_input(ns) is None                         # --auto_masks alone: nothing is refined
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--refine_sigma", "wide"])
    for flag in ("--refine_masks", "--refine_sigma"):
        assert flag in RS.__doc__
    assert RS._refine_masks_input(argparse.Namespace()) is None      # a namespace from before the flags existed


REFUSALS = [(["--refine_masks"], "needs --auto_masks"),
            (["--refine_sigma", "0.1"], "needs --refine_masks"),
            (["--auto_masks", "3", "--refine_sigma", "0.1"], "needs --refine_masks"),
            (["--auto_masks", "3", "--refine_masks", "--refine_sigma", "0.009"], "0.01..1"),
            (["--auto_masks", "3", "--refine_masks", "--refine_sigma", "1.5"], "0.01..1"),
            (["--auto_masks", "3", "--refine_masks", "--refine_sigma", "nan"], "0.01..1"),
            (["--auto_masks", "3", "--refine_masks", "--refine_sigma", "-0.1"], "0.01..1"),
            (["--auto_masks", "9", "--refine_masks"], "2..8"),                              # inherited
            (["--auto_masks", "3", "--refine_masks", "--style_mix", "other.jpg"], "--style_mix"),
            (["--auto_masks", "3", "--refine_masks", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_refine_masks_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out.jpg"
    with pytest.raises(ValueError, match=match):
        RS.run(RS.build_parser().parse_args([str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(out)]
                                            + extra))
    assert not out.exists()


def test_host_entry_points_refuse_bad_arguments_without_a_gpu():
    import torch
    from nn import strotss_utils as U
    image, grid = torch.zeros((8, 8, 3)), torch.zeros((2, 2), dtype=torch.int32)
    for sigma in (0.0, 0.009, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="sigma"):
            U.refine_labels(image, grid, 2, sigma)
        with pytest.raises(ValueError, match="sigma"):
            U.auto_masks(None, image, image, 3, refine=sigma)
    for k in (0, 17):
        with pytest.raises(ValueError, match="regions"):
            U.refine_labels(image, grid, k)
