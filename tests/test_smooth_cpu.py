"""Photo smoothing without a GPU: the two float64 statements of the guided filter against each other,
the filter's identities (constant guide, an image affine in the guide, one-pixel windows), the float32 statement against the
rounding budget of the GPU test (that test is not vacuous), the refusals of the C entry before any launch, the operator
surface and the parser / refusals of --photo_smooth."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _smooth_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000)    # non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)                                                     # not 16-byte aligned
NULL = None


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("r", [1, 3, 40])
@pytest.mark.parametrize("hw", [(13, 17), (21, 32)])
def test_the_two_statements_agree(hw, r):
    rng = np.random.default_rng(hw[0] * 100 + r)
    p, I = rng.random(hw + (3,)), rng.random(hw + (3,))
    for eps in (1e-2, 1e-4):
        direct, separable = R.guided_direct(p, I, r, eps), R.guided_separable(p, I, r, eps)
        err = float(np.abs(direct - separable).max())
        print(f"{hw[0]} x {hw[1]}, r {r}, eps {eps}: statements differ by {err:.2e}")
        assert err <= 1e-12
    p32, I32 = R.test_images(hw[0], hw[1], r)                      # the structured images of the GPU test as well
    assert float(np.abs(R.guided_direct(p32, I32, r, 1e-4) - R.guided_separable(p32, I32, r, 1e-4)).max()) <= 1e-12


def test_window_counts_are_the_clipped_boxes():
    assert R.extents(5, 1).tolist() == [2, 3, 3, 3, 2]
    assert R.extents(3, 64).tolist() == [3, 3, 3]                  # a window larger than the image is the whole image
    assert R.extents(1, 1).tolist() == [1]
    x = np.random.default_rng(0).random((9, 14, 2))
    for r in (1, 2, 5, 20):
        got = R.box_sum(x, r)
        for y, xx in ((0, 0), (4, 7), (8, 13), (2, 12)):
            want = x[max(y - r, 0):y + r + 1, max(xx - r, 0):xx + r + 1].sum((0, 1))
            assert np.allclose(got[y, xx], want, rtol=0, atol=1e-12)
        assert np.allclose(R.box_sum(np.ones((9, 14)), r), R.counts(9, 14, r), rtol=0, atol=0)


@pytest.mark.parametrize("r", [1, 4, 40])
def test_constant_guide_gives_the_twice_averaged_image(r):
    p = np.random.default_rng(r).random((19, 23, 3))
    out = R.guided_separable(p, np.full((19, 23, 3), 0.5), r, 1e-2, full=True)       # 0.5 p is exact: cov(I, p) == 0
    assert not out["a"].any()
    assert float(np.abs(out["q"] - R.box_mean_twice(p, r)).max()) <= 1e-15
    out = R.guided_separable(p, np.full((19, 23, 3), [0.3, 0.6, 0.1]), r, 1e-4, full=True)
    assert float(np.abs(out["a"]).max()) <= 1e-11                  # cov is rounding noise (1e-16) over eps = 1e-4
    assert float(np.abs(out["q"] - R.box_mean_twice(p, r)).max()) <= 1e-11
    assert float(np.abs(R.guided_direct(p, np.full((19, 23, 3), 0.5), r, 1e-2) - R.box_mean_twice(p, r)).max()) <= 1e-14


def _shrinkage(I, M, r, eps):
    """p = M I + t gives a_k = M - eps Sigma_k^{-1} M and q(i) - p(i) = mean_k (a_k - M)(I(i) - mu_k) over the windows k
    around i, so |q_c(i) - p_c(i)| <= mean_k eps |Sigma_k^{-1}|_2 |M_c|_2 |I(i) - mu_k|_2 -- computed here window by window"""
    h, w = I.shape[:2]
    m = R.guided_separable(I, I, r, eps, full=True)
    inv_norm = 1.0 / np.linalg.eigvalsh(m["sigma"])[..., 0]                       # |Sigma_k^{-1}|_2, Sigma_k includes eps
    bound = np.empty((h, w, 3))
    for y in range(h):
        for x in range(w):
            ys, xs = slice(max(y - r, 0), y + r + 1), slice(max(x - r, 0), x + r + 1)
            dist = np.linalg.norm(I[y, x] - m["mu"][ys, xs], axis=-1)
            bound[y, x] = R.eps32(eps) * (inv_norm[ys, xs] * dist).mean() * np.linalg.norm(M, axis=1)
    return bound


@pytest.mark.parametrize("r", [1, 3, 40])
def test_an_image_affine_in_the_guide_comes_back_up_to_the_shrinkage(r):
    rng = np.random.default_rng(7 + r)
    I = rng.random((13, 17, 3))
    M, t = np.eye(3) * 0.8 + 0.3 * rng.standard_normal((3, 3)), np.array([0.1, -0.2, 0.05])
    p = I @ M.T + t
    bound = _shrinkage(I, M, r, 1e-4)
    for q in (R.guided_separable(p, I, r, 1e-4), R.guided_direct(p, I, r, 1e-4)):
        err = np.abs(q - p)
        print(f"r {r}: largest |q - p| {err.max():.3e}, largest shrinkage bound {bound.max():.3e}")
        assert (err <= bound + 1e-12).all()
    assert (np.abs(R.box_mean_twice(p, r) - p) > bound).any()      # the bound tells the filter from a plain blur


@pytest.mark.parametrize("hw", [(1, 1), (1, 3)])
def test_tiny_images_return_the_guide_when_filtered_by_themselves(hw):
    I = np.random.default_rng(3).random(hw + (3,))
    for r in (1, 64):
        for fn in (R.guided_separable, R.guided_direct):
            q = fn(I, I, r, 1e-4)
            if hw == (1, 1):
                assert np.array_equal(q, I)                        # Sigma = eps Id, cov = 0: a = 0, b = p
            else:
                assert (np.abs(q - I) <= _shrinkage(I, np.eye(3), r, 1e-4) + 1e-12).all()


def test_float32_throughout_misses_the_rounding_budget():
    """The guard of the GPU test: its tolerance E_round + E_stat is one that arithmetic in float32 throughout does NOT
    meet, so a kernel that passes it has kept its window sums and its solve in float64.  768 x 1024, eps = 1e-4, r = 4."""
    h, w, r, eps = 768, 1024, 4, 1e-4
    p, I = R.test_images(h, w, h + w)
    ref = R.guided_separable(p, I, r, eps, full=True)
    e_round, e_stat = R.error_budgets(p, I, r, eps, ref)
    err = np.abs(R.guided_float32(p, I, r, eps).astype(np.float64) - ref["q"])
    over = float((err > e_round + e_stat).mean())
    print(f"float32 throughout: largest error {err.max():.3e} = {float((err / e_round).max()):.1f} E_round; "
          f"{100 * over:.1f} % of the elements outside E_round + E_stat; max E_round {e_round.max():.3e}, "
          f"max E_stat {e_stat.max():.3e}")
    assert (err > e_round).any()
    assert over > 0.01
    assert e_stat.max() <= e_round.max()


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


def test_guided_smooth_refuses_bad_arguments(lib):
    big = 26755                                      # 3 * 26755^2 > INT_MAX
    size = lib.strotss_guided_smooth_workspace_bytes
    assert size(48, 64, 4) == 216 * 48 * 64 == size(48, 64, 64)
    assert size(1, 1, 1) == 216
    assert size(0, 8, 4) == 0 and size(8, -1, 4) == 0 and size(big, big, 4) == 0
    assert size(8, 8, 0) == 0 and size(8, 8, 65) == 0
    ws = 216 * 64
    call = lambda img=P, guide=G, h=8, w=8, r=4, eps=1e-2, out=Q, work=P, nbytes=ws: \
        lib.strotss_guided_smooth(img, guide, h, w, r, eps, out, work, nbytes, NULL)
    assert call(img=NULL) == EINVAL
    assert call(guide=NULL) == EINVAL
    assert call(out=NULL) == EINVAL
    assert call(work=NULL) == EINVAL
    assert call(h=0) == EINVAL and call(w=-3) == EINVAL
    assert call(h=big, w=big, nbytes=2 ** 62) == EINVAL
    assert call(r=0) == EINVAL and call(r=65) == EINVAL and call(r=-1) == EINVAL
    for bad in (float("nan"), float("inf"), -1e-2, 0.0, 0.99e-4, 1.0001):
        assert call(eps=bad) == EINVAL, bad
    assert call(nbytes=ws - 1) == EINVAL and call(nbytes=0) == EINVAL
    assert call(out=G) == EINVAL                     # out == guide
    assert call(img=ODD) == EALIGN
    assert call(guide=ODD) == EALIGN
    assert call(out=ODD) == EALIGN
    assert call(work=ODD) == EALIGN


# ------------------------------------------------------------------ 3. the operator surface
def test_default_radius_rule():
    from nn import strotss_utils as U
    assert U.SMOOTH_MAX_RADIUS == R.MAX_RADIUS == 64 and U.DEFAULT_SMOOTH_EPS == 1e-2
    assert [U.default_smooth_radius(h, w) for h, w in ((1, 1), (48, 64), (512, 384), (768, 1024), (4096, 6000), (9000, 2))] \
        == [1, 1, 8, 16, 64, 64]


def test_operator_surface_refuses_on_the_host():
    """refused before a kernel is asked for (there is none to ask for here)"""
    import torch
    from nn import strotss_utils as U
    img, other, grey = torch.rand(1, 6, 8, 3), torch.rand(6, 9, 3), torch.rand(6, 8, 1)
    with pytest.raises(ValueError, match="differ in size"):
        U.guided_smooth(img, other)
    with pytest.raises(ValueError):
        U.guided_smooth(img, grey)
    with pytest.raises(ValueError):
        U.guided_smooth(grey, img)
    for radius in (0, 65, -4, 2.5):
        with pytest.raises(ValueError, match="radius"):
            U.guided_smooth(img, img.clone(), radius=radius)
    for eps in (float("nan"), float("inf"), 0.0, 1e-5, 1.5, -1e-2):
        with pytest.raises(ValueError, match="eps"):
            U.guided_smooth(img, img.clone(), eps=eps)


# ------------------------------------------------------------------ 4. the command line
def test_parser_knows_the_three_flags():
    import run_strotss as RS
    parser = RS.build_parser()
    ns = parser.parse_args(["c.jpg", "s.jpg"])
    assert ns.photo_smooth is False and ns.smooth_radius is None and ns.smooth_eps is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--photo_smooth", "--smooth_radius", "7", "--smooth_eps", "1e-3"])
    assert ns.photo_smooth is True and ns.smooth_radius == 7 and ns.smooth_eps == 1e-3
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--photo_smooth", "--smooth_radius", "2.5"])
    for flag in ("--photo_smooth", "--smooth_radius", "--smooth_eps"):
        assert flag in RS.__doc__
    assert RS._photo_smooth_input(parser.parse_args(["c.jpg", "s.jpg"])) is None
    assert RS._photo_smooth_input(parser.parse_args(["c.jpg", "s.jpg", "--photo_smooth"])) == (None, 1e-2)
    assert RS._photo_smooth_input(ns) == (7, 1e-3)
    import argparse
    assert RS._photo_smooth_input(argparse.Namespace()) is None          # a namespace from before the flags existed


REFUSALS = [(["--smooth_radius", "4"], "need --photo_smooth"), (["--smooth_eps", "1e-2"], "need --photo_smooth"),
            (["--photo_smooth", "--smooth_radius", "0"], "radius"), (["--photo_smooth", "--smooth_radius", "65"], "radius"),
            (["--photo_smooth", "--smooth_eps", "1e-5"], "eps"), (["--photo_smooth", "--smooth_eps", "2"], "eps"),
            (["--photo_smooth", "--smooth_eps", "nan"], "eps"), (["--photo_smooth", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_photo_smooth_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for base in (missing, video):
        with pytest.raises(ValueError, match=match):
            RS.run(RS.build_parser().parse_args(base + extra))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")


def test_photo_smooth_is_refused_on_several_ranks(monkeypatch, tmp_path):
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    for base in (missing, video):
        with pytest.raises(ValueError, match="one GPU"):
            RS.run(RS.build_parser().parse_args(base + ["--photo_smooth"]))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")
