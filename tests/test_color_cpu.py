"""Colour preservation without a GPU: the float64 restatement's own identities (mean and covariance of
the recoloured style, degenerate inputs, the luminance merge), the host-side colour_transform against it, the refusals of
the three C entries before any launch, and the parser / refusals of --preserve_color."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _color_ref as R  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EALIGN = -1, -2
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)        # not 16-byte aligned
NULL = None


def _golden_pair():
    from PIL import Image
    read = lambda name: np.asarray(Image.open(os.path.join(GOLDEN, name)).convert("RGB"), dtype=np.float64) / 255.0
    return read("content_im.jpg"), read("style_im.jpg")


def _random_pairs():
    rng = np.random.default_rng(0)
    yield rng.random((40, 56, 3)), rng.random((33, 71, 3))
    # correlated channels, a narrow palette against a wide one
    base = rng.random((48, 64, 1))
    yield 0.2 + 0.1 * base + 0.02 * rng.random((48, 64, 3)), rng.random((21, 32, 3)) ** 2
    yield rng.random((7, 5, 3)).astype(np.float32), rng.random((9, 4, 3)).astype(np.float32)


# ------------------------------------------------------------------ 1. the restatement: match
def _check_identity(style, content, style_mask=None, content_mask=None):
    out, A, b = R.match64(style, content, style_mask, content_mask)
    mu_c, sigma_c = R.stats64(content, content_mask)
    mu, sigma = R.stats64(out, style_mask)
    assert float(np.abs(mu - mu_c).max()) <= 1e-12
    assert float(np.abs(sigma - R.expected_cov(sigma_c, A)).max()) <= 1e-12
    return out, A, b


def test_matched_style_has_the_contents_mean_and_covariance():
    for content, style in _random_pairs():
        _check_identity(style, content)
    rng = np.random.default_rng(1)
    content, style = rng.random((30, 40, 3)), rng.random((24, 36, 3))
    cm, sm = (rng.random((30, 40)) < 0.5).astype(np.float64), (rng.random((24, 36)) < 0.3).astype(np.float64)
    out, _, _ = _check_identity(style, content, sm, cm)
    assert np.array_equal(out[sm == 0], style[sm == 0])          # outside the mask: copied


def test_matched_golden_pair_at_full_size():
    content, style = _golden_pair()
    mu_c, sigma_c = R.stats64(content)
    mu_s, sigma_s = R.stats64(style)
    out, A, _ = _check_identity(style, content)
    mu, sigma = R.stats64(out)
    before = (float(np.linalg.norm(sigma_s - sigma_c)), float(np.linalg.norm(mu_s - mu_c)))
    after = (float(np.linalg.norm(sigma - sigma_c)), float(np.linalg.norm(mu - mu_c)))
    outside = float(((out < 0) | (out > 1)).any(-1).mean())
    print(f"golden pair: covariance / mean distance before {before[0]:.4f} / {before[1]:.4f}, after {after[0]:.2e} / "
          f"{after[1]:.2e}; {100 * outside:.1f} % of the pixels leave [0, 1], lowest {out.min():.4f}")
    assert after[0] < 1e-3 * before[0] and after[1] < 1e-9 * before[1]
    assert after[0] <= R.EPS * np.linalg.norm(np.eye(3) - A @ A.T) + 1e-12      # all of it the eps term
    assert outside > 0          # the reason the kernel does not clamp: a clamp would break the identity above


def test_colour_transform_is_the_restatement():
    from nn import strotss_utils as U
    assert U.COLOUR_EPS == R.EPS
    for content, style in list(_random_pairs()) + [_golden_pair()]:
        ss, sc = R.stats64(style), R.stats64(content)
        A, b = U.colour_transform(*ss, *sc)
        A_ref, b_ref = R.transform64(*ss, *sc)
        assert A.dtype == np.float64 and b.dtype == np.float64
        scale = max(1.0, float(np.abs(A_ref).max()))
        assert float(np.abs(A - A_ref).max()) <= 1e-12 * scale and float(np.abs(b - b_ref).max()) <= 1e-12 * scale


def _transforms():
    from nn import strotss_utils as U
    return (R.transform64, U.colour_transform)


def test_degenerate_statistics_stay_finite():
    rng = np.random.default_rng(2)
    mu_c, sigma_c = R.stats64(rng.random((20, 30, 3)))
    mu_s, sigma_s = R.stats64(rng.random((20, 30, 3)) ** 3)
    flat_mu, zero = np.array([0.3, 0.5, 0.7]), np.zeros((3, 3))
    for transform in _transforms():
        # a flat style: the gain is bounded by 1 / sqrt(eps) = 255
        A, b = transform(flat_mu, zero, mu_c, sigma_c)
        assert np.isfinite(A).all() and np.isfinite(b).all()
        assert float(np.abs(A - 255.0 * R.sym_power(sigma_c, 0.5)).max()) <= 1e-9
        assert float(np.abs(A @ flat_mu + b - mu_c).max()) <= 1e-12
        # a flat content: the style's spread shrinks to below one 8-bit step
        A, b = transform(mu_s, sigma_s, flat_mu, zero)
        assert np.isfinite(A).all() and np.isfinite(b).all()
        assert float(np.abs(A - np.sqrt(R.EPS) * R.sym_power(sigma_s, -0.5)).max()) <= 1e-12
        assert np.linalg.norm(A, 2) <= 1.0 + 1e-12
        # both flat
        A, b = transform(flat_mu, zero, mu_c, zero)
        assert float(np.abs(A - np.eye(3)).max()) <= 1e-12 and float(np.abs(b - (mu_c - flat_mu)).max()) <= 1e-12
        # identical statistics: the identity map
        A, b = transform(mu_s, sigma_s, mu_s, sigma_s)
        assert float(np.abs(A - np.eye(3)).max()) <= 1e-12 and float(np.abs(b).max()) <= 1e-12


def test_colour_transform_refuses_bad_statistics():
    from nn import strotss_utils as U
    mu, sigma = np.full(3, 0.5), np.eye(3) * 0.01
    with pytest.raises(ValueError):
        U.colour_transform(np.zeros(4), sigma, mu, sigma)
    with pytest.raises(ValueError):
        U.colour_transform(mu, np.zeros((3, 2)), mu, sigma)
    with pytest.raises(ValueError):
        U.colour_transform(mu, sigma, np.array([0.1, np.nan, 0.2]), sigma)
    with pytest.raises(ValueError):
        U.colour_transform(mu, sigma, mu, np.full((3, 3), np.inf))


def test_operator_surface_refuses_mismatched_shapes():
    """refused on the host, before a kernel is asked for (there is none to ask for here)"""
    import torch
    from nn import strotss_utils as U
    img, other, grey = torch.rand(1, 6, 8, 3), torch.rand(1, 6, 9, 3), torch.rand(6, 8, 1)
    with pytest.raises(ValueError):
        U.luminance_merge(img, other)
    with pytest.raises(ValueError):
        U.luminance_merge(img, grey)
    with pytest.raises(ValueError):
        U.colour_statistics(grey)
    with pytest.raises(ValueError):
        U.colour_statistics(img, torch.ones(6, 9))
    with pytest.raises(ValueError):
        U.match_colour(img, other, torch.ones(6, 9), None)
    with pytest.raises(ValueError):
        U.match_colour(torch.rand(6, 8), other)


# ------------------------------------------------------------------ 2. the restatement: luminance
def test_luminance_merge_keeps_the_results_luma_and_the_contents_chroma():
    rng = np.random.default_rng(3)
    for shape in ((40, 56, 3), (1, 1, 3), (3, 1, 3)):
        r, c = rng.random(shape), rng.random(shape)
        out = R.luma_merge64(r, c)
        yr, yc = R.luma64(r), R.luma64(c)
        # 1e-15 ~ 9 * 2^-53: the roundings of Y(c), of c + d per channel and of Y(out), each relative to |Y(r)| + |Y(c)|
        assert (np.abs(R.luma64(out) - yr) <= 1e-15 * (np.abs(yr) + np.abs(yc))).all()
        d = out - c
        scale = np.abs(c).max(-1) + np.abs(yr - yc)
        assert (np.abs(d - d[..., :1]).max(-1) <= 1e-15 * scale).all()
        assert np.array_equal(R.luma_merge64(c, c), c)
    # the chroma is the content's: (U, V) of out - c vanish because the inverse of RGB2YUV sends Y to (1, 1, 1)
    assert float(np.abs(np.linalg.inv(R.RGB2YUV)[0] - 1.0).max()) <= 1e-8
    assert float(np.abs((out - c) @ R.RGB2YUV[:, 1:]).max()) <= 1e-8
    assert R.chroma_distance(out, c) <= 1e-8 < R.chroma_distance(r, c)


# ------------------------------------------------------------------ 3. the C ABI refuses before it launches
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


def test_color_entries_refuse_bad_arguments(lib):
    big = 26755                                      # 3 * 26755^2 > INT_MAX
    # statistics
    assert lib.strotss_color_stats(NULL, NULL, 8, 8, P, P, NULL) == EINVAL
    assert lib.strotss_color_stats(P, NULL, 8, 8, NULL, P, NULL) == EINVAL
    assert lib.strotss_color_stats(P, NULL, 8, 8, P, NULL, NULL) == EINVAL
    assert lib.strotss_color_stats(P, P, 0, 8, P, P, NULL) == EINVAL
    assert lib.strotss_color_stats(P, P, 8, -1, P, P, NULL) == EINVAL
    assert lib.strotss_color_stats(P, P, big, big, P, P, NULL) == EINVAL
    assert lib.strotss_color_stats(ODD, NULL, 8, 8, P, P, NULL) == EALIGN
    assert lib.strotss_color_stats(P, ODD, 8, 8, P, P, NULL) == EALIGN
    assert lib.strotss_color_stats(P, NULL, 8, 8, ODD, P, NULL) == EALIGN
    assert lib.strotss_color_stats(P, NULL, 8, 8, P, ODD, NULL) == EALIGN
    assert lib.strotss_color_stats_workspace_bytes(0, 8) == 0
    assert lib.strotss_color_stats_workspace_bytes(big, big) == 0
    assert lib.strotss_color_stats_workspace_bytes(1, 1) == 16 + 80
    assert lib.strotss_color_stats_workspace_bytes(768, 1024) == 16 + 80 * 768
    # the affine map: A and b are host arrays, read before anything else is done with the image pointers
    A, b = (C.c_float * 9)(1, 0, 0, 0, 1, 0, 0, 0, 1), (C.c_float * 3)(0, 0, 0)
    assert lib.strotss_color_affine(NULL, NULL, 8, 8, A, b, P, NULL) == EINVAL
    assert lib.strotss_color_affine(P, NULL, 8, 8, None, b, P, NULL) == EINVAL
    assert lib.strotss_color_affine(P, NULL, 8, 8, A, None, P, NULL) == EINVAL
    assert lib.strotss_color_affine(P, NULL, 8, 8, A, b, NULL, NULL) == EINVAL
    assert lib.strotss_color_affine(P, NULL, 8, 0, A, b, P, NULL) == EINVAL
    assert lib.strotss_color_affine(P, NULL, big, big, A, b, P, NULL) == EINVAL
    for bad in (float("nan"), float("inf"), -float("inf")):
        A_bad, b_bad = (C.c_float * 9)(1, 0, 0, 0, bad, 0, 0, 0, 1), (C.c_float * 3)(0, 0, bad)
        assert lib.strotss_color_affine(P, NULL, 8, 8, A_bad, b, P, NULL) == EINVAL
        assert lib.strotss_color_affine(P, NULL, 8, 8, A, b_bad, P, NULL) == EINVAL
    assert lib.strotss_color_affine(ODD, NULL, 8, 8, A, b, P, NULL) == EALIGN
    assert lib.strotss_color_affine(P, ODD, 8, 8, A, b, P, NULL) == EALIGN
    assert lib.strotss_color_affine(P, NULL, 8, 8, A, b, ODD, NULL) == EALIGN
    # the luminance merge
    assert lib.strotss_luma_merge(NULL, P, 8, 8, P, NULL) == EINVAL
    assert lib.strotss_luma_merge(P, NULL, 8, 8, P, NULL) == EINVAL
    assert lib.strotss_luma_merge(P, P, 8, 8, NULL, NULL) == EINVAL
    assert lib.strotss_luma_merge(P, P, 0, 0, P, NULL) == EINVAL
    assert lib.strotss_luma_merge(P, P, big, big, P, NULL) == EINVAL
    assert lib.strotss_luma_merge(ODD, P, 8, 8, P, NULL) == EALIGN
    assert lib.strotss_luma_merge(P, ODD, 8, 8, P, NULL) == EALIGN
    assert lib.strotss_luma_merge(P, P, 8, 8, ODD, NULL) == EALIGN


# ------------------------------------------------------------------ 4. the command line
def test_parser_takes_the_two_modes_only():
    import run_strotss as RS
    parser = RS.build_parser()
    assert parser.parse_args(["c.jpg", "s.jpg"]).preserve_color is None
    for mode in ("match", "luminance"):
        assert parser.parse_args(["c.jpg", "s.jpg", "--preserve_color", mode]).preserve_color == mode
    with pytest.raises(SystemExit):
        parser.parse_args(["c.jpg", "s.jpg", "--preserve_color", "bogus"])
    assert "--preserve_color" in RS.__doc__


@pytest.mark.parametrize("mode", ["match", "luminance"])
def test_preserve_color_is_refused_on_several_gpus_before_anything_is_loaded(mode, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="--strips"):
        RS.run(RS.build_parser().parse_args(missing + ["--preserve_color", mode, "--strips"]))
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    with pytest.raises(ValueError, match="--strips"):
        RS.run(RS.build_parser().parse_args(video + ["--preserve_color", mode, "--strips"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(missing + ["--preserve_color", mode]))
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(video + ["--preserve_color", mode]))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")
