"""Region tracking without a GPU: the restatement (tests/_track_ref.py) against itself -- inertia only
ever keeps more priors, beta = 2 keeps them all, the float32 and float64 statements of the warp agree on every case of the GPU
tests -- the margin condition on the data of the GPU tests, the refusals of the two C entries before any launch, and the
parser / refusals of --track_masks and --mask_inertia."""
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
import _cluster_ref as R  # noqa: E402
import _track_ref as TR  # noqa: E402

EINVAL, EALIGN = -1, -2
P, Q, G, H = C.c_void_p(0x10000), C.c_void_p(0x20000), C.c_void_p(0x30000), C.c_void_p(0x40000)   # aligned, never touched
ODD = C.c_void_p(0x10004)                                                                          # not 16-byte aligned
NULL = None


# ------------------------------------------------------------------ 1. the restatement
@pytest.mark.parametrize("shape", TR.ASSIGN_SHAPES)
def test_inertia_keeps_more_priors_and_two_keeps_all(shape):
    n, d, k = shape
    x, inv, c32, prior = TR.assign_case(n, d, k)
    valid = (prior[:n] >= 0) & (prior[:n] < k)
    kept = []
    for beta in (0.0, 0.01, 0.05, 0.2, 1.0, 2.0):
        label = TR.assign_prior(x, inv, n, d, c32, prior, beta)[0]
        kept.append(int((label == prior[:n]).sum()))
    print(f"n {n} d {d} k {k}: rows with label == prior {kept} of {int(valid.sum())} valid priors")
    assert all(b >= a for a, b in zip(kept, kept[1:]))
    assert np.array_equal(label[valid], prior[:n][valid])            # beta = 2, the last of the loop
    plain = R.assign(x, inv, n, d, c32)
    zero = TR.assign_prior(x, inv, n, d, c32, prior, 0.0)
    none = TR.assign_prior(x, inv, n, d, c32, np.full_like(prior, -1), 0.05)
    for got in (zero, none):                                         # no bias: the plain assignment
        assert all(np.array_equal(a, b) for a, b in zip(got[:3], plain[:3]))


@pytest.mark.parametrize("shape", TR.ASSIGN_SHAPES)
@pytest.mark.parametrize("beta", TR.BETAS)
def test_gpu_cases_have_few_rows_within_the_bound(shape, beta):
    """the condition of the GPU test: the rows whose biased margin is within E = assign_bound(d) are exempt from label
    equality there, and they are at most 5 % of the rows (the cap of test_cluster_cpu.py); the rows whose scores are exactly
    zero are not exempt, their label is the valid prior when beta > 0 and 0 otherwise"""
    n, d, k = shape
    x, inv, c32, prior = TR.assign_case(n, d, k)
    label, best, second, s, score = TR.assign_prior(x, inv, n, d, c32, prior, beta)
    E = R.assign_bound(d)
    exempt = (TR.biased_margin(score) <= E) & ~TR.exact_rows(x, inv, n, d)
    print(f"n {n} d {d} k {k} beta {beta}: {100 * float(exempt.mean()):.2f} % of the rows within E = {E:.2e}")
    assert float(exempt.mean()) <= 0.05
    if n >= 3:
        assert TR.exact_rows(x, inv, n, d)[[1, 2]].all() and not s[[1, 2]].any()
        want = prior[1] if beta > 0 else 0
        assert label[1] == want and label[2] == want and best[2] == 0 and second[2] == 0
    assert set(np.unique(prior[:n])) <= set(range(-1, k + 1)) and (n < 100 or {-1, k} <= set(np.unique(prior[:n])))


@pytest.mark.parametrize("shape", TR.WARP_SHAPES)
def test_warp_cases_are_exact_in_float32(shape):
    h, w, gh, gw = shape
    cases = TR.warp_cases(h, w, gh, gw)
    outside = set()
    seen = set()
    for name, grid, flow, cert in cases:
        assert np.array_equal(flow[np.isfinite(flow)] * 4, np.round(flow[np.isfinite(flow)] * 4)), name   # multiples of 1/4
        a = TR.label_warp(grid, TR.WARP_K, flow, cert, np.float32)
        b = TR.label_warp(grid, TR.WARP_K, flow, cert, np.float64)
        assert np.array_equal(a, b), name
        assert ((a >= -1) & (a < TR.WARP_K)).all()
        seen |= set(np.unique(a).tolist())
        if "zero-none" in name:                                      # a zero flow: the grid itself, out-of-range labels as -1
            assert np.array_equal(a, np.where((grid >= 0) & (grid < TR.WARP_K), grid, -1))
        if "checker" in name:
            yc, xc = TR.probes(gh, h), TR.probes(gw, w)
            off = cert[yc][:, xc] < 0.5
            assert (a[off] == -1).all()
        if "push" in name:
            yc, xc = TR.probes(gh, h), TR.probes(gw, w)
            f = flow[yc][:, xc]
            sy, sx = np.floor(yc[:, None] + f[..., 1] + 0.5), np.floor(xc[None, :] + f[..., 0] + 0.5)
            outside |= {e for e, m in (("up", sy < 0), ("down", sy >= h), ("left", sx < 0), ("right", sx >= w)) if m.any()}
            assert (a[(sy < 0) | (sy >= h) | (sx < 0) | (sx >= w)] == -1).all()
        if "nonfinite" in name:
            assert np.isnan(flow).sum() == 1 and np.isinf(flow).sum() == 1 and a[0, 0] == -1 and a[-1, -1] == -1
    assert outside == {"up", "down", "left", "right"}
    assert -1 in seen and len(seen) >= 2
    assert np.array_equal(TR.cell_starts(5, 21), [0, 5, 9, 13, 17, 21]) and np.array_equal(TR.probes(5, 21), [2, 6, 10, 14, 18])
    for g, n in ((5, 21), (64, 64), (1, 7), (7, 32)):                # the cells are those of y g // n
        s = TR.cell_starts(g, n)
        assert all((np.arange(s[i], s[i + 1]) * g // n == i).all() for i in range(g)) and s[-1] == n


# ------------------------------------------------------------------ 2. the C ABI refuses before it launches
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_label_warp_refuses_bad_arguments(lib):
    call = lambda grid=P, gh=5, gw=7, k=3, flow=Q, cert=G, h=21, w=32, prior=H: \
        lib.strotss_label_warp(grid, gh, gw, k, flow, cert, h, w, prior, NULL)
    for name in ("grid", "flow", "prior"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(cert=ODD) == EALIGN
    for bad in (dict(gh=0), dict(gw=-1), dict(h=0), dict(w=0), dict(gh=22), dict(gw=33), dict(k=0), dict(k=17),
                dict(h=2 ** 15, w=2 ** 15)):
        assert call(**bad) == EINVAL, bad


def test_kmeans_assign_prior_refuses_bad_arguments(lib):
    call = lambda x=P, inv=Q, n=8, d=35, ld=64, c=G, k=3, prior=H, beta=0.05, lab=H, best=P, second=Q: \
        lib.strotss_kmeans_assign_prior(x, inv, n, d, ld, c, k, prior, beta, lab, best, second, NULL)
    for name in ("x", "inv", "c", "prior", "lab", "best", "second"):
        assert call(**{name: NULL}) == EINVAL, name
        assert call(**{name: ODD}) == EALIGN, name
    assert call(n=0) == EINVAL and call(n=-4) == EINVAL
    assert call(d=0) == EINVAL and call(d=65) == EINVAL
    assert call(n=2 ** 26, ld=64) == EINVAL                          # n ld > INT_MAX
    assert call(k=0) == EINVAL and call(k=17) == EINVAL and call(k=-1) == EINVAL
    for beta in (-0.01, 2.01, math.nan, math.inf, -math.inf):
        assert call(beta=beta) == EINVAL, beta
    assert call(ld=48) == EALIGN and call(d=3, ld=4) == EALIGN


def test_abi_version_is_unchanged(lib):
    from nn import _hip
    assert lib.strotss_abi_version() == 8 == _hip.ABI_VERSION
    assert {"strotss_label_warp", "strotss_kmeans_assign_prior"} <= set(_hip.SIGNATURES)


# ------------------------------------------------------------------ 3. the command line
def test_parser_knows_the_flags():
    import argparse
    import run_strotss as RS
    from nn import strotss_utils as U
    parser = RS.build_parser()
    ns = parser.parse_args(["c", "s.jpg"])
    assert ns.track_masks is False and ns.mask_inertia is None and RS._track_masks_input(ns) is None
    assert RS._track_masks_input(argparse.Namespace()) is None      # a namespace from before the flags existed
    on = ["c", "s.jpg", "--video", "--compute_flow", "--auto_masks", "3", "--track_masks"]
    assert RS._track_masks_input(parser.parse_args(on)) == U.MASK_INERTIA == 0.05
    for b in (0.0, 0.3, 2.0):
        assert RS._track_masks_input(parser.parse_args(on + ["--mask_inertia", str(b)])) == b
    assert RS._auto_masks_input(parser.parse_args(on + ["--save_masks", "m"])) == (3, "m")
    assert U.MASK_INERTIA_RANGE == (0.0, 2.0)
    for bad in (-0.1, 2.5, math.nan, math.inf):
        with pytest.raises(ValueError):
            U.check_mask_inertia(bad)
    U.check_mask_inertia(None)
    for flag in ("--track_masks", "--mask_inertia"):
        assert flag in RS.__doc__


VIDEO = ["--video", "--compute_flow"]
REFUSALS = [(["--track_masks"], "needs --auto_masks"), (VIDEO + ["--track_masks"], "needs --auto_masks"),
            (["--auto_masks", "3", "--track_masks"], "needs --video"),
            (["--mask_inertia", "0.1"], "needs --track_masks"),
            (VIDEO + ["--auto_masks", "3", "--mask_inertia", "0.1"], "needs --track_masks"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--mask_inertia", "2.5"], "0..2"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--mask_inertia", "-0.5"], "0..2"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--mask_inertia", "nan"], "0..2"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--mask_inertia", "inf"], "0..2"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--style_mix", "other.jpg"], "--style_mix"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--content_mask", "c.png", "--style_mask", "s.png"], "--content_mask"),
            (VIDEO + ["--auto_masks", "9", "--track_masks"], "2..8"),
            (VIDEO + ["--auto_masks", "3", "--track_masks", "--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_track_masks_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be another error than the ValueError asked for"""
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    out = tmp_path / "out"
    with pytest.raises(ValueError, match=match):
        RS.run(RS.build_parser().parse_args([str(tmp_path / "no_frames"), str(tmp_path / "no_style.jpg"), "-o", str(out)] + extra))
    assert not out.exists()


def test_auto_masks_with_video_still_needs_track_masks(monkeypatch, tmp_path):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    video = [str(tmp_path / "no_frames"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out")] + VIDEO
    with pytest.raises(ValueError, match="--video") as err:
        RS.run(RS.build_parser().parse_args(video + ["--auto_masks", "3"]))
    assert "--track_masks" in str(err.value)
    # with the flag the refusals of --auto_masks are passed: the next complaint is the sequence's own (no such directory)
    with pytest.raises(ValueError, match="not a directory of frames"):
        RS.run(RS.build_parser().parse_args(video + ["--auto_masks", "3", "--track_masks"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(video + ["--auto_masks", "3", "--track_masks"]))
    assert not (tmp_path / "out").exists()
