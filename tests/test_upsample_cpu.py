"""Guided upsampling without a GPU: the two float64 statements against each other, the equal-size
identities, the analytic bound for an image affine in the guide (which a plain bilinear upsample violates), the float32
statement against the budget of the GPU test (that test is not vacuous), the refusals of the C entry before any launch, the
operator surface and the parser / refusals of --output_size."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _smooth_ref as S  # noqa: E402
import _upsample_ref as R  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G, B, W_ = (C.c_void_p(a) for a in (0x10000, 0x20000, 0x30000, 0x40000, 0x50000))   # non-null, aligned, never touched
ODD = C.c_void_p(0x10004)                                                                   # not 16-byte aligned
NULL = None
GUIDED, RESIDUAL = 0, 1
# the size pairs of the GPU test (tests/test_hip_upsample.py: SHAPES), and a small anisotropic one
SHAPES = [((12, 16), (48, 64)), ((21, 32), (42, 63)), ((42, 63), (257, 300)), ((5, 7), (5, 7)), ((1, 1), (3, 5)),
          ((1, 3), (1, 300)), ((11, 31), (33, 31)), ((8, 8), (32, 32)), ((5, 41), (25, 41)), ((2, 2), (1024, 2)),
          ((9, 11), (30, 17))]


# ------------------------------------------------------------------ 1. the restatement
def test_taps_are_the_half_pixel_taps():
    lo, hi, t = R.taps(8, 4)                          # scale 0.5: centres at -0.25, 0.25, 0.75, ...
    assert lo.tolist() == [0, 0, 0, 1, 1, 2, 2, 3] and hi.tolist() == [0, 1, 1, 2, 2, 3, 3, 3]
    assert np.array_equal(t, [0.75, 0.25, 0.75, 0.25, 0.75, 0.25, 0.75, 0.25])
    lo, hi, t = R.taps(7, 7)                          # equal sizes: the sample itself, weight 0
    assert lo.tolist() == hi.tolist() == list(range(7)) and not t.any()
    x = np.random.default_rng(0).standard_normal((7, 5, 2))
    assert np.array_equal(R.up(x, 7, 5), x)           # a weight of exactly 0 returns the sample bit for bit


@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("lo,hi", SHAPES)
def test_the_two_statements_agree(lo, hi, mode):
    p, I_lo, I_hi = R.test_images(*lo, *hi, 17 + lo[0] + hi[1])
    # the pixel loops take about 10 s per call at 257 x 300: one parameter pair there, both at every other size
    for r, eps in ((1, 1e-2), (3, 1e-4)) if hi[0] * hi[1] < 50000 else ((3, 1e-4),):
        one, two = R.upsample_loops(p, I_lo, I_hi, r, eps, mode), R.upsample(p, I_lo, I_hi, r, eps, mode)
        assert one.shape == hi + (3,)
        assert float(np.abs(one - two).max()) <= 1e-12


@pytest.mark.parametrize("hw", [(5, 7), (21, 32), (1, 1)])
def test_equal_sizes(hw):
    """guided at equal sizes IS the guided filter of _smooth_ref, bit for bit; residual is p up to the rounding of the
    difference p - q and of the sum q + (p - q)"""
    p, I = S.test_images(*hw, 3)
    for r, eps in ((1, 1e-2), (4, 1e-4)):
        q = S.guided_separable(p, I, r, eps)
        assert np.array_equal(R.upsample(p, I, I, r, eps, "guided"), q)
        back = R.upsample(p, I, I, r, eps, "residual")
        p64 = p.astype(np.float64)
        assert (np.abs(back - p64) <= S.U53 * (np.abs(p64 - q) + np.abs(p64)) * (1 + 1e-9)).all()


@pytest.mark.parametrize("mode", R.MODES)
def test_an_image_affine_in_the_guide_comes_back_at_the_target_size(mode):
    """p = M I_lo + t with I_lo the 2 x 2 block mean of I_hi: the output is M I_hi + t within the shrinkage bound at EVERY
    output pixel, edges finer than the result's grid included; a plain bilinear up(p) is not, on the edge.  The guide's noise
    (amplitude 0.15: variance 1.9e-3 per channel, 4.7e-4 after the block mean, both far above eps = 1e-4) makes every window's
    Sigma well conditioned, so the bound is a few percent of the step; factor 2 puts the edge between result pixels."""
    rng = np.random.default_rng(5)
    h, w, r, eps = 12, 16, 2, 1e-4
    H, W = 2 * h, 2 * w
    yy, xx = np.mgrid[0:H, 0:W]
    edge = xx + yy > (H + W) / 2 + 0.5
    shade = 0.4 + 0.2 * np.sin(xx / 9.0) * np.cos(yy / 7.0)
    I_hi = (shade + 0.25 * edge)[..., None] * np.array([0.9, 0.7, 0.8]) + 0.15 * rng.random((H, W, 3))
    I_lo = R.down2(I_hi)
    M, t = np.eye(3) * 0.8 + 0.3 * rng.standard_normal((3, 3)), np.array([0.1, -0.2, 0.05])
    p = I_lo @ M.T + t
    want = I_hi @ M.T + t
    bound = R.affine_bound(I_lo, I_hi, M, r, eps, mode)
    for fn in (R.upsample, R.upsample_loops):
        err = np.abs(fn(p, I_lo, I_hi, r, eps, mode) - want)
        print(f"{mode}: largest error {err.max():.3e}, largest bound {bound.max():.3e}, largest error / bound "
              f"{float((err / bound).max()):.3f}")
        assert (err <= bound + 1e-12).all()
    plain = np.abs(R.up(p, H, W) - want)
    on_edge = edge ^ np.roll(edge, 1, axis=1)
    on_edge[:, 0] = False
    print(f"plain up(p): largest error {plain.max():.3e}; {int((plain > bound).any(-1)[on_edge].sum())} of "
          f"{int(on_edge.sum())} edge pixels outside the bound")
    assert (plain > bound).any(-1)[on_edge].any()


CASES = [((12, 16), (48, 64), 4, 1e-4), ((21, 32), (42, 63), 1, 1e-2), ((42, 63), (257, 300), 4, 1e-4), ((5, 7), (5, 7), 64, 1e-4)]


@pytest.mark.parametrize("mode", R.MODES)
def test_the_budget_is_positive_and_the_statistics_condition_holds(mode):
    """E_round > 0 and E_stat >= 0 at every element, and section 16's condition max E_stat <= max E_round at every case"""
    for lo, hi, r, eps in CASES:
        p, I_lo, I_hi = R.test_images(*lo, *hi, 29)
        e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, eps, mode)
        assert e_round.shape == hi + (3,) and (e_round > 0).all() and (e_stat >= 0).all()
        assert e_stat.max() <= e_round.max()


@pytest.mark.parametrize("mode", R.MODES)
def test_float32_throughout_misses_the_budget(mode):
    """The guard of the GPU test: arithmetic in float32 throughout does NOT meet E_round + E_stat, so a kernel that passes
    has kept its window sums and its solve in float64 and rounds no more often than section 27 counts.  192 x 256 -> 384 x 512,
    eps = 1e-4, r = 4."""
    (h, w), (H, W), r, eps = (192, 256), (384, 512), 4, 1e-4
    p, I_lo, I_hi = R.test_images(h, w, H, W, h + w)
    ref = R.coefficients(p, I_lo, r, eps)
    e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, eps, mode, ref)
    err = np.abs(R.upsample_float32(p, I_lo, I_hi, r, eps, mode).astype(np.float64) - R.upsample(p, I_lo, I_hi, r, eps, mode, ref=ref))
    over = float((err > e_round + e_stat).mean())
    print(f"{mode}, float32 throughout: largest error {err.max():.3e} = {float((err / e_round).max()):.1f} E_round; "
          f"{100 * over:.1f} % of the elements outside E_round + E_stat; max E_round {e_round.max():.3e}, "
          f"max E_stat {e_stat.max():.3e}")
    assert (err > e_round + e_stat).any()
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


def test_guided_upsample_refuses_bad_arguments(lib):
    big = 26755                                      # 3 * 26755^2 > INT_MAX
    size = lib.strotss_guided_upsample_workspace_bytes
    assert size(48, 64, 4) == 280 * 48 * 64 == size(48, 64, 64)
    assert size(1, 1, 1) == 280
    assert size(0, 8, 4) == 0 and size(8, -1, 4) == 0 and size(big, big, 4) == 0
    assert size(8, 8, 0) == 0 and size(8, 8, 65) == 0
    ws = 280 * 64
    call = lambda img=P, lo=G, h=8, w=8, hi=B, H=16, W=24, r=4, eps=1e-2, mode=RESIDUAL, out=Q, work=W_, nbytes=ws: \
        lib.strotss_guided_upsample(img, lo, h, w, hi, H, W, r, eps, mode, out, work, nbytes, NULL)
    for name in ("img", "lo", "hi", "out", "work"):
        assert call(**{name: NULL}) == EINVAL, name
    assert call(h=0) == EINVAL and call(w=-3) == EINVAL and call(H=0) == EINVAL and call(W=-1) == EINVAL
    assert call(H=7) == EINVAL and call(W=7) == EINVAL                   # a target smaller than the result
    assert call(H=big, W=big) == EINVAL
    assert call(h=big, w=big, H=big, W=big, nbytes=2 ** 62) == EINVAL
    assert call(r=0) == EINVAL and call(r=65) == EINVAL and call(r=-1) == EINVAL
    for bad in (float("nan"), float("inf"), -1e-2, 0.0, 0.99e-4, 1.0001):
        assert call(eps=bad) == EINVAL, bad
    assert call(mode=2) == EINVAL and call(mode=-1) == EINVAL
    assert call(nbytes=ws - 1) == EINVAL and call(nbytes=0) == EINVAL
    assert call(out=B) == EINVAL and call(out=G) == EINVAL and call(out=P) == EINVAL      # out is an input
    assert call(out=C.c_void_p(0x40000 + 16)) == EINVAL and call(out=C.c_void_p(0x40000 - 16)) == EINVAL    # or overlaps one
    for name in ("img", "lo"):
        assert call(**{name: ODD}) == EALIGN, name
    assert call(out=C.c_void_p(0x20004)) == EALIGN
    assert call(hi=C.c_void_p(0x40004)) == EALIGN and call(work=C.c_void_p(0x50008)) == EALIGN


# ------------------------------------------------------------------ 3. the operator surface
def test_defaults_are_the_documented_ones():
    from nn import strotss_utils as U
    assert U.UPSAMPLE_MODES == ("residual", "guided") and set(U.UPSAMPLE_MODES) == set(R.MODES)
    assert U.default_upsample_eps("residual") == 1e-3 and U.default_upsample_eps("guided") == U.DEFAULT_SMOOTH_EPS


def test_operator_surface_refuses_on_the_host():
    """refused before a kernel is asked for (there is none to ask for here)"""
    import torch
    from nn import strotss_utils as U
    img, lo, hi = torch.rand(1, 6, 8, 3), torch.rand(6, 8, 3), torch.rand(12, 16, 3)
    with pytest.raises(ValueError, match="mode"):
        U.guided_upsample(img, lo, hi, mode="bicubic")
    with pytest.raises(ValueError, match="differ in size"):
        U.guided_upsample(img, torch.rand(6, 9, 3), hi)
    for bad in (torch.rand(6, 8, 1), torch.rand(2, 6, 8, 3)):
        for args in ((bad, lo, hi), (img, bad, hi), (img, lo, bad)):
            with pytest.raises(ValueError):
                U.guided_upsample(*args)
    for small in (torch.rand(5, 16, 3), torch.rand(12, 7, 3)):
        with pytest.raises(ValueError, match="smaller than the result"):
            U.guided_upsample(img, lo, small)
    with pytest.raises(ValueError, match="exceeds"):
        U.check_upsample_sizes(6, 8, 26755, 26755)
    for radius in (0, 65, -4, 2.5):
        with pytest.raises(ValueError, match="radius"):
            U.guided_upsample(img, lo, hi, radius=radius)
    for eps in (float("nan"), float("inf"), 0.0, 1e-5, 1.5, -1e-2):
        with pytest.raises(ValueError, match="eps"):
            U.guided_upsample(img, lo, hi, eps=eps)


# ------------------------------------------------------------------ 4. the command line
FLAGS = ("output_size", "upsample_mode", "upsample_radius", "upsample_eps")


def test_parser_knows_the_four_flags():
    import run_strotss as RS
    parser = RS.build_parser()
    ns = parser.parse_args(["c.jpg", "s.jpg"])
    assert all(getattr(ns, f) is None for f in FLAGS)
    assert RS._output_size_input(ns) is None
    bare = argparse.Namespace(**{k: v for k, v in vars(ns).items() if k not in FLAGS})
    assert RS._output_size_input(bare) is None                          # a namespace from before the flags existed
    assert RS._output_size_input(argparse.Namespace()) is None
    ns = parser.parse_args(["c.jpg", "s.jpg", "--output_size", "full"])
    assert RS._output_size_input(ns) == dict(size="full", mode="residual", radius=None, eps=None)
    ns = parser.parse_args(["c.jpg", "s.jpg", "--output_size", "4096", "--upsample_mode", "guided", "--upsample_radius", "7",
                            "--upsample_eps", "1e-3"])
    assert RS._output_size_input(ns) == dict(size=4096, mode="guided", radius=7, eps=1e-3)
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--output_size", "full", "--upsample_mode", "bicubic"])
    for flag in FLAGS:
        assert "--" + flag in RS.__doc__


REFUSALS = [(["--upsample_mode", "guided"], "need --output_size"), (["--upsample_radius", "4"], "need --output_size"),
            (["--upsample_eps", "1e-2"], "need --output_size"),
            (["--output_size", "63"], "--output_size"), (["--output_size", "16385"], "--output_size"),
            (["--output_size", "1024.5"], "--output_size"), (["--output_size", "half"], "--output_size"),
            (["--output_size", "-512"], "--output_size"), (["--output_size", "1e3"], "--output_size"),
            (["--output_size", "full", "--upsample_radius", "0"], "--upsample_radius"),
            (["--output_size", "full", "--upsample_radius", "65"], "--upsample_radius"),
            (["--output_size", "full", "--upsample_eps", "1e-5"], "--upsample_eps"), (["--output_size", "full", "--upsample_eps", "2"], "--upsample_eps"),
            (["--output_size", "full", "--upsample_eps", "nan"], "--upsample_eps"), (["--output_size", "full", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_output_size_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for base in (missing, video):
        with pytest.raises(ValueError, match=match):
            RS.run(RS.build_parser().parse_args(base + extra))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")


def test_output_size_is_refused_on_several_ranks(monkeypatch, tmp_path):
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    monkeypatch.setenv("WORLD_SIZE", "2")
    for base in (missing, video):
        with pytest.raises(ValueError, match="one GPU"):
            RS.run(RS.build_parser().parse_args(base + ["--output_size", "full"]))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")
