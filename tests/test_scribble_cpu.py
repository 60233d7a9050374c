"""Scribble masks without a GPU: the float64 restatement (tests/_scribble_ref.py) against itself and
against hand-written expressions, the conditions on the seeded cases of the GPU tests (the float32 yardstick Y and the label
margins), the seeds of the cell grid, the stroke loader, the workspace size and the refusals of the C entries before any
launch, and the parser / refusals of the scribble flags."""
import ctypes as C
import math
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _scribble_cases as S  # noqa: E402
import _scribble_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G, H, T = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))   # aligned, never touched
ODD = C.c_void_p(0x10004)                                                                # not 16-byte aligned
NULL = None
CASES = [(h, w, k) for (h, w) in S.SHAPES for k in S.KS]


# ------------------------------------------------------------------ 1. the restatement and the cases
def test_constants_match_the_product():
    from nn import _hip
    from nn import strotss_utils as U
    assert (U.SCRIBBLE_TAU, U.SCRIBBLE_LAMBDA, U.SCRIBBLE_ITERS, U.SCRIBBLE_SIGMA) == (R.TAU, R.LAMBDA, R.ITERS, R.SIGMA)
    assert (R.TAU, R.LAMBDA, R.ITERS, R.SIGMA) == (0.05, 0.05, 128, 0.1) and U.SCRIBBLE_SIGMA == U.REFINE_SIGMA_R
    assert U.SCRIBBLE_RANGE == (2, R.MAX_K) == (2, _hip.SCRIBBLE_MAX_K) and U.SCRIBBLE_ITERS_RANGE == (1, R.MAX_ITERS)
    assert _hip.SCRIBBLE_MAX_ITERS == R.MAX_ITERS == 1024 and U.SCRIBBLE_SIGMA_RANGE == (0.01, 1.0)
    assert list(U.MASK_COLOURS) == R.CORNER_COLOURS


@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-k%d" % c)
def test_case_conditions(case):
    """per case and sweep count: the planes sum to 1 and lie in [0, 1], fixed pixels never move, the yardstick
    Y = max |x_f32ref - x_f64ref| lies in (0, 5e-6), at most 1 % of the pixels have a float64 margin below 8 Y"""
    h, w, k = case
    img, stroke, scores = S.make(h, w, k)
    assert img.shape == (h, w, 3) and img.dtype == np.float32 and 0 <= img.min() and img.max() <= 1
    assert scores.shape[2] == k and stroke.shape == (h, w) and (stroke[0, 0] >= 0) and stroke[-1, -1] == -1
    ref = S.run(h, w, k)
    fixed = ref["fixed"]
    assert np.array_equal(fixed, stroke >= 0) and 0 < fixed.sum() < h * w
    assert abs(ref["q"].sum(axis=0) - 1).max() <= 1e-12
    for n in S.sweeps_of((h, w)):
        x = ref[n]["x"]
        assert abs(x.sum(axis=0) - 1).max() <= 1e-12 and x.min() >= 0 and x.max() <= 1
        assert np.array_equal(x[:, fixed], (np.arange(k)[:, None] == stroke[fixed][None]).astype(np.float64))
        assert np.array_equal(ref[n]["label"][fixed], stroke[fixed]) and ref[n]["count"].sum() == h * w
        Y = S.yardstick(h, w, k, n)
        share = float((ref[n]["margin"] < S.MARGIN_FACTOR * Y).mean())
        print(f"{h} x {w}, k {k}, {n} sweeps: Y {Y:.2e}, {100 * share:.2f} % of the pixels with a margin below 8 Y")
        assert 0 < Y < S.Y_CAP
        assert share <= S.MARGIN_SHARE


def test_one_sweep_on_a_1x2_image_by_hand():
    """pixel 0 carries a stroke of region 1; pixel 1 has one neighbour, to its west"""
    img = np.array([[[0.2, 0.4, 0.6], [0.25, 0.4, 0.5]]], dtype=np.float32)
    stroke = np.array([[1, -1]], dtype=np.int32)
    scores = np.array([[[0.5, 0.4], [0.3, 0.45]]], dtype=np.float32)             # a 1 x 2 grid: the pixels sit on the cells
    out = R.diffuse(img, stroke, scores, iters=1)
    i = img.astype(np.float64)
    wgt = math.exp(-(((i[0, 0] - i[0, 1]) ** 2).sum()) / (2 * 0.1 ** 2))
    s = scores.astype(np.float64)[0, 1] / 0.05
    q = np.exp(s - s.max()) / np.exp(s - s.max()).sum()
    assert np.allclose(out["q"][:, 0, 1], q, rtol=0, atol=1e-15) and np.isclose(out["wE"][0, 0], wgt, rtol=0, atol=1e-15)
    assert out["wE"][0, 1] == 0 and not out["wS"].any()
    want = (0.05 * q + wgt * np.array([0.0, 1.0])) / (0.05 + wgt)
    assert np.allclose(out[1]["x"][:, 0, 1], want, rtol=0, atol=1e-15)
    assert out[1]["x"][:, 0, 0].tolist() == [0.0, 1.0]


def test_one_sweep_on_a_2x2_image_by_hand():
    """the grid is the image (u = y, v = x): q is the softmax of the cell's own scores; pixel (1, 1) has a north and a west
    neighbour, pixel (0, 0) carries a stroke"""
    rng = np.random.default_rng(5)
    img = rng.random((2, 2, 3)).astype(np.float32)
    scores = rng.random((2, 2, 3)).astype(np.float32)
    stroke = np.array([[2, -1], [-1, -1]], dtype=np.int32)
    out = R.diffuse(img, stroke, scores, iters=1, lam=0.2, tau=0.5, sigma=0.7)
    i, s = img.astype(np.float64), scores.astype(np.float64) / 0.5
    q = np.exp(s - s.max(axis=2, keepdims=True))
    q = np.moveaxis(q / q.sum(axis=2, keepdims=True), 2, 0)
    assert np.allclose(out["q"], q, rtol=0, atol=1e-15)
    wgt = lambda a, b: math.exp(-((i[a] - i[b]) ** 2).sum() / (2 * 0.7 ** 2))
    wn, ww = wgt((1, 1), (0, 1)), wgt((1, 1), (1, 0))
    want = (0.2 * q[:, 1, 1] + wn * q[:, 0, 1] + ww * q[:, 1, 0]) / (0.2 + wn + ww)
    assert np.allclose(out[1]["x"][:, 1, 1], want, rtol=0, atol=1e-15)
    onehot = np.array([0.0, 0.0, 1.0])
    we, ws = wgt((0, 1), (0, 0)), wgt((0, 1), (1, 1))                              # pixel (0, 1): west is the stroke
    want = (0.2 * q[:, 0, 1] + we * onehot + ws * q[:, 1, 1]) / (0.2 + we + ws)
    assert np.allclose(out[1]["x"][:, 0, 1], want, rtol=0, atol=1e-15)
    assert out[1]["x"][:, 0, 0].tolist() == onehot.tolist()


def test_bilinear_sampling_clamps_to_the_grid():
    g = np.arange(6, dtype=np.float32).reshape(2, 3, 1)
    s = R.sample_scores(g, 4, 6)[0]
    assert s[0, 0] == 0 and s[3, 5] == 5                               # u = -0.25 and 1.25: the edge cells
    assert np.isclose(s[1, 2], 0.25 * 3 + 0.75 * 1.0)                  # u = 0.25, v = 0.75
    assert np.array_equal(R.sample_scores(g, 2, 3)[0], g[..., 0].astype(np.float64))


def test_seeds_take_the_majority_and_the_lowest_label_on_a_tie():
    from nn import strotss_utils as U
    stroke = np.full((256, 192), -1, dtype=np.int32)                   # g = 4: cells of 4 x 4 pixels, a 64 x 48 grid
    stroke[0, 0:3] = 1
    stroke[1, 0:2] = 0                                                 # cell (0, 0): three 1s, two 0s
    stroke[4, 4:6] = 2
    stroke[5, 4:6] = 1                                                 # cell (1, 1): a tie between 1 and 2
    stroke[255, 191] = 0
    stroke[8, 8] = 9                                                   # outside 0..k-1: no stroke
    seeds = U.scribble_seeds(stroke, 3)
    assert seeds.shape == (64, 48) and seeds.dtype == np.int32
    assert seeds[0, 0] == 1 and seeds[1, 1] == 1 and seeds[63, 47] == 0 and seeds[2, 2] == -1
    assert (seeds >= 0).sum() == 3
    rng = np.random.default_rng(11)
    for h, w in ((256, 170), (42, 64), (7, 5), (171, 256)):
        strokes = np.where(rng.random((h, w)) < 0.03, rng.integers(0, 4, (h, w)), -1).astype(np.int32)
        g = -(-max(h, w) // U.AUTO_MASK_GRID)
        ys, xs = U.auto_mask_grid(h, w)
        assert np.array_equal(U.scribble_seeds(strokes, 4), R.seeds(strokes, g, len(ys), len(xs), 4))
    a = np.arange(12, dtype=np.int32).reshape(3, 4)
    assert np.array_equal(U.resize_strokes(a, 7, 9), R.nearest(a, 7, 9)) and np.array_equal(U.resize_strokes(a, 3, 4), a)


def _save(path, pixels):
    from PIL import Image
    Image.fromarray(np.asarray(pixels, dtype=np.uint8), "RGB").save(path, format="PNG")
    return str(path)


def test_load_scribbles(tmp_path):
    from nn import strotss_utils as U
    c = np.zeros((6, 8, 3), dtype=np.uint8)
    c[0, :3] = (255, 0, 0)
    c[5, 4:] = (0, 0, 255)
    c[2, 2] = (254, 254, 254)                                          # below the threshold: black, no stroke
    s = np.zeros((4, 4, 3), dtype=np.uint8)
    s[0, 0] = (0, 0, 255)
    s[3, 3] = (255, 0, 0)
    cs, ss, colours = U.load_scribbles(_save(tmp_path / "c.png", c), _save(tmp_path / "s.png", s))
    assert colours == [(0, 0, 255), (255, 0, 0)]                       # ascending (r, g, b)
    assert cs.dtype == np.int32 and cs.shape == (6, 8) and ss.shape == (4, 4)
    assert (cs[0, :3] == 1).all() and (cs[5, 4:] == 0).all() and (cs == -1).sum() == 48 - 7
    assert ss[0, 0] == 0 and ss[3, 3] == 1 and (ss == -1).sum() == 14
    s[1, 1] = (0, 255, 0)
    with pytest.raises(ValueError, match="one file only"):
        U.load_scribbles(str(tmp_path / "c.png"), _save(tmp_path / "s3.png", s))
    one = np.zeros((4, 4, 3), dtype=np.uint8)
    one[0, 0] = (255, 255, 255)
    with pytest.raises(ValueError, match="1 stroke colours"):
        U.load_scribbles(_save(tmp_path / "one.png", one), str(tmp_path / "one.png"))
    with pytest.raises(ValueError, match="0 stroke colours"):
        U.load_scribbles(_save(tmp_path / "none.png", np.zeros((4, 4, 3))), str(tmp_path / "none.png"))


# ------------------------------------------------------------------ 2. the C ABI
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_the_three_symbols_are_exported(lib):
    from nn import _hip
    for name in ("strotss_kmeans_scores", "strotss_scribble_workspace_bytes", "strotss_scribble_labels"):
        assert name in _hip.SIGNATURES and hasattr(C.CDLL(_hip.LIB_PATH), name)


def test_workspace_bytes_hold_the_planes_of_the_restatement(lib):
    size = lib.strotss_scribble_workspace_bytes
    slice_ = lambda h, w: (h * w * 4 + 255) // 256 * 256
    for h, w, k in ((1, 2, 2), (42, 63, 3), (97, 130, 7), (768, 1024, 7), (64, 64, 2)):
        assert size(h, w, k) == R.planes_in_workspace(k) * slice_(h, w), (h, w, k)
    assert size(1, 1, 2) == 8 * 256 and size(64, 64, 2) == 8 * 64 * 64 * 4
    for bad in ((0, 5, 2), (5, 0, 2), (-1, 5, 2), (5, 5, 1), (5, 5, 8), (5, 5, 0), (2 ** 15, 2 ** 15, 2), (2 ** 14, 2 ** 15, 5)):
        assert size(*bad) == 0, bad
    assert size(2 ** 14, 2 ** 15, 3) > 0 and size(2 ** 14, 2 ** 14, 7) > 0      # k h w and 3 h w below 2^31


def test_scribble_labels_refuses_bad_arguments(lib):
    nbytes = lib.strotss_scribble_workspace_bytes(33, 47, 3)
    inf, nan = float("inf"), float("nan")

    def call(img=P, stroke=Q, h=33, w=47, scores=G, gh=9, gw=12, k=3, tau=0.05, lam=0.05, sigma=0.1, iters=8, per=0, label=H,
             count=T, x=NULL, ws=P, nb=nbytes):
        return lib.strotss_scribble_labels(img, stroke, h, w, scores, gh, gw, k, tau, lam, sigma, iters, per, label, count, x, ws,
                                           nb, NULL)
    for name in ("img", "stroke", "scores", "label", "count", "ws"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(x=ODD) == EALIGN                                      # optional, but aligned when given
    big = 2 ** 62
    for name in ("h", "w", "gh", "gw"):
        assert call(**{name: 0}, nb=big) == EINVAL and call(**{name: -3}, nb=big) == EINVAL, name
    assert call(h=2 ** 15, w=2 ** 15, nb=big) == EINVAL               # k h w > INT_MAX
    assert call(gh=2 ** 15, gw=2 ** 15, nb=big) == EINVAL
    for k in (-1, 0, 1, 8, 16):
        assert call(k=k, nb=big) == EINVAL, k
    for name in ("tau", "lam", "sigma"):
        for bad in (0.0, -0.1, inf, nan, 1e-320):                     # 1e-320: positive, but its reciprocal overflows
            assert call(**{name: bad}) == EINVAL, (name, bad)
    assert call(lam=1e-200) == EINVAL and call(sigma=1e-200) == EINVAL  # 0 as float32; 2 sigma^2 underflows
    for iters in (0, -1, 1025):
        assert call(iters=iters) == EINVAL, iters
    for per in (-1, 3, 5, 16):
        assert call(per=per) == EINVAL, per
    assert call(nb=nbytes - 1) == EINVAL and call(nb=0) == EINVAL


def test_kmeans_scores_refuses_bad_arguments(lib):
    def call(x=P, inv=Q, n=40, d=35, ld=64, centres=G, k=3, scores=H):
        return lib.strotss_kmeans_scores(x, inv, n, d, ld, centres, k, scores, NULL)
    for name in ("x", "inv", "centres", "scores"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(n=0) == EINVAL and call(d=0) == EINVAL and call(d=65) == EINVAL and call(n=2 ** 26, ld=64) == EINVAL
    assert call(k=0) == EINVAL and call(k=17) == EINVAL and call(ld=40, d=35) == EALIGN


# ------------------------------------------------------------------ 3. the command line
def test_parser_knows_the_four_flags():
    import argparse
    import run_strotss as RS
    parser = RS.build_parser()
    ns = parser.parse_args(["c.jpg", "s.jpg"])
    assert ns.content_scribbles is None and ns.style_scribbles is None and ns.scribble_sigma is None and ns.scribble_iters is None
    assert RS._scribble_masks_input(ns) is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--content_scribbles", "a.png", "--style_scribbles", "b.png"])
    assert RS._scribble_masks_input(ns) == ("a.png", "b.png", 0.1, 128) and RS._auto_masks_input(ns) is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--content_scribbles", "a.png", "--style_scribbles", "b.png", "--scribble_sigma",
                            "0.05", "--scribble_iters", "7", "--save_masks", "d"])
    assert RS._scribble_masks_input(ns) == ("a.png", "b.png", 0.05, 7) and RS._auto_masks_input(ns) is None
    for sigma, iters in (("0.01", "1"), ("1", "1024")):
        ns = parser.parse_args(["c.jpg", "s.jpg", "--content_scribbles", "a.png", "--style_scribbles", "b.png",
                                "--scribble_sigma", sigma, "--scribble_iters", iters])
        assert RS._scribble_masks_input(ns)[2:] == (float(sigma), int(iters))
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--scribble_iters", "many"])
    for flag in ("--content_scribbles", "--style_scribbles", "--scribble_sigma", "--scribble_iters"):
        assert flag in RS.__doc__
    assert RS._scribble_masks_input(argparse.Namespace()) is None     # a namespace from before the flags existed


BOTH = ["--content_scribbles", "a.png", "--style_scribbles", "b.png"]
REFUSALS = [(["--content_scribbles", "a.png"], "go together"),
            (["--style_scribbles", "b.png"], "go together"),
            (["--scribble_sigma", "0.1"], "needs --content_scribbles"),
            (["--scribble_iters", "8"], "needs --content_scribbles"),
            (["--save_masks", "d"], "needs --auto_masks"),                                 # inherited: nothing to save
            (BOTH + ["--scribble_sigma", "0.009"], "0.01..1"),
            (BOTH + ["--scribble_sigma", "1.5"], "0.01..1"),
            (BOTH + ["--scribble_sigma", "nan"], "0.01..1"),
            (BOTH + ["--scribble_iters", "0"], "1..1024"),
            (BOTH + ["--scribble_iters", "1025"], "1..1024"),
            (BOTH + ["--content_mask", "m.png", "--style_mask", "n.png"], "--content_mask"),
            (BOTH + ["--auto_masks", "3"], "--auto_masks"),
            (BOTH + ["--style_mix", "other.jpg"], "--style_mix"),
            (BOTH + ["--video"], "--video"),
            (BOTH + ["--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_scribbles_are_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out.jpg"
    with pytest.raises(ValueError, match=match):
        RS.run(RS.build_parser().parse_args([str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(out)]
                                            + extra))
    assert not out.exists()


def test_scribbles_are_refused_in_a_multi_process_run(monkeypatch, tmp_path):
    import run_strotss as RS
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args([str(tmp_path / "c.jpg"), str(tmp_path / "s.jpg")] + BOTH))


def test_host_entry_points_refuse_bad_arguments_without_a_gpu():
    from nn import strotss_utils as U
    strokes = np.zeros((4, 4), dtype=np.int32)
    for k in (1, 8):
        with pytest.raises(ValueError, match="regions"):
            U.scribble_regions(None, None, None, strokes, strokes, k)
    for sigma in (0.0, 0.009, 1.01, float("nan")):
        with pytest.raises(ValueError, match="sigma"):
            U.scribble_regions(None, None, None, strokes, strokes, 2, sigma=sigma)
    for iters in (0, 1025, 2.5):
        with pytest.raises(ValueError, match="sweeps"):
            U.scribble_regions(None, None, None, strokes, strokes, 2, iters=iters)
