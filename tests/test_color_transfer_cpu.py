"""Colour distribution transfer without a GPU: the float64 restatement's own identities (the sliced
Wasserstein orderings on the golden pair and on a two-colour content, masks, identical inputs), the properties of its
transfer table, the host's basis sequence against it, the refusals of the three C entries before any launch, and the
parser / refusals of --preserve_color transfer and --transfer_iters."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)
import _color_transfer_ref as T  # noqa: E402

GOLDEN = os.path.join(ROOT, "tests", "golden")
EINVAL, EALIGN = -1, -2
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)        # not 16-byte aligned
NULL = None


def _golden_pair(size=64):
    from PIL import Image

    def read(name):
        im = Image.open(os.path.join(GOLDEN, name)).convert("RGB")
        im.thumbnail((size, size))
        return np.asarray(im, dtype=np.float64) / 255.0
    return read("content_im.jpg"), read("style_im.jpg")


def _two_colour_pair():
    """a content of two colour masses, which no affine image of a uniform style has"""
    rng = np.random.default_rng(0)
    c = np.where(rng.random((48, 64, 1)) < 0.5, [0.8, 0.2, 0.1], [0.1, 0.3, 0.9]) + 0.03 * rng.standard_normal((48, 64, 3))
    return np.clip(c, 0, 1), rng.random((40, 56, 3))


# ------------------------------------------------------------------ 1. the restatement's own identities
@pytest.mark.parametrize("pair", [_golden_pair, _two_colour_pair])
def test_transfer_beats_the_affine_match_and_a_tenth_of_the_start(pair):
    content, style = pair()
    out = T.transfer64(style, content, iters=10, bins=1024)
    start, affine, moved = T.swd(style, content), T.swd(T.affine_match64(style, content), content), T.swd(out, content)
    print(f"{pair.__name__}: sliced Wasserstein distance to the content {start:.4f} before, {affine:.4f} after the affine "
          f"match, {moved:.4f} after the transfer; the result spans [{out.min():.3f}, {out.max():.3f}]")
    assert moved < affine
    assert moved < 0.1 * start


def test_pixels_outside_the_mask_are_unchanged():
    content, style = _two_colour_pair()
    rng = np.random.default_rng(3)
    sm, cm = (rng.random(style.shape[:2]) < 0.4).astype(np.float64), (rng.random(content.shape[:2]) < 0.6).astype(np.float64)
    out = T.transfer64(style, content, sm, cm, iters=4, bins=256)
    assert np.array_equal(out[sm == 0], style[sm == 0])
    assert not np.array_equal(out[sm != 0], style[sm != 0])
    # the counted pixels moved toward the counted content, not toward all of it
    assert T.swd(out, content, sm, cm) < 0.1 * T.swd(style, content, sm, cm)


def test_identical_source_and_target_give_the_identity():
    """Where the occupied bins of an axis are contiguous, equal histograms give the table T[j] = edge j on them and the
    map is the identity up to rounding.  (Across a run of EMPTY bins the table takes the run's left end, as the
    statement's "smallest target bin" says, and the pixels of the bin behind the run are stretched over it: 16 bins on a
    dense uniform image have no such run.)  The rounding is that of lo and scale to float32: the table's edge j is
    lo + j (hi - lo) / bins in double, the binning's is lo32 + j / scale32, at most 2^-24 (|lo| + (hi - lo)) apart; a
    pixel moves by at most that on each axis, sqrt(3) times that per channel, once per iteration."""
    x = np.random.default_rng(4).random((48, 64, 3))
    iters, budget = 4, 0.0
    for R in T.bases64(iters):
        h = T.hist64(x, R, 16)
        for k in range(3):
            filled = np.nonzero(h[k])[0]
            assert np.array_equal(filled, np.arange(filled[0], filled[-1] + 1))
        lo, hi = T.axis_range(R)
        budget += np.sqrt(3) * T.U24 * float((np.abs(lo) + (hi - lo)).max())
    out = T.transfer64(x, x, iters=iters, bins=16)
    print(f"identical inputs: largest move {np.abs(out - x).max():.3e}, budget {budget:.3e}")
    assert float(np.abs(out - x).max()) <= budget


# ------------------------------------------------------------------ 2. the restatement's table
def _histograms(kind, bins, rng):
    if kind == "random":
        return rng.integers(0, 50, (3, bins)), rng.integers(0, 50, (3, bins))
    if kind == "spiky":
        hs, hc = rng.integers(1, 50, (3, bins)), rng.integers(1, 50, (3, bins))
        hs[:, 1::2] = 0
        hc[:, ::2] = 0
        return hs, hc
    hs, hc = np.zeros((3, bins), dtype=np.int64), rng.integers(0, 50, (3, bins))
    hs[:, bins // 3] = 1000
    return (hs, hc) if kind == "single_src" else (hc, hs)


@pytest.mark.parametrize("kind", ["random", "spiky", "single_src", "single_dst"])
@pytest.mark.parametrize("bins", [2, 16, 256])
def test_table_is_monotone_between_the_targets_end_bins(kind, bins):
    rng = np.random.default_rng(bins)
    hs, hc = _histograms(kind, bins, rng)
    for R in T.bases64(3):
        table = T.table64(hs, hc, R, bins)
        lo, hi = T.axis_range(R)
        width = (hi - lo) / bins
        assert table.shape == (3, bins + 1)
        assert (np.diff(table, axis=1) >= 0).all()
        for k in range(3):
            filled = np.nonzero(hc[k])[0]
            assert abs(table[k, 0] - (lo[k] + filled[0] * width[k])) <= 1e-15 * 4
            assert abs(table[k, -1] - (lo[k] + (filled[-1] + 1) * width[k])) <= 1e-15 * 4


def test_table_of_an_empty_histogram_is_the_identity():
    rng = np.random.default_rng(9)
    full, zero = rng.integers(0, 9, (3, 16)), np.zeros((3, 16), dtype=np.int64)
    R = T.bases64(2)[1]
    ident = T.identity_table(R, 16)
    lo, hi = T.axis_range(R)
    assert np.array_equal(ident[:, 0], lo) and float(np.abs(ident[:, -1] - hi).max()) <= 1e-15
    for hs, hc in ((zero, full), (full, zero), (zero, zero)):
        assert np.array_equal(T.table64(hs, hc, R, 16), ident)
    mixed = full.copy()
    mixed[1] = 0                                    # one axis empty: that axis alone is the identity
    table = T.table64(rng.integers(0, 9, (3, 16)), mixed, R, 16)
    assert np.array_equal(table[1], ident[1]) and not np.array_equal(table[0], ident[0])


# ------------------------------------------------------------------ 3. the host's bases
def test_transfer_bases_are_the_restatements():
    from nn import strotss_utils as U
    assert (U.DEFAULT_TRANSFER_ITERS, U.TRANSFER_BINS) == (10, 1024)
    bases = U.transfer_bases(64)
    assert bases.dtype == np.float32 and bases.shape == (64, 3, 3)
    assert np.array_equal(bases, T.bases64(64))
    assert np.array_equal(bases[0], np.eye(3, dtype=np.float32))
    assert np.array_equal(U.transfer_bases(10), bases[:10])          # a prefix: more iterations go on where fewer stopped
    for R in bases.astype(np.float64):
        assert float(np.abs(R.T @ R - np.eye(3)).max()) <= 1e-6 < 1e-4
    np.random.seed(5)                                                # not a function of any global seed
    assert np.array_equal(U.transfer_bases(10), bases[:10])
    for bad in (0, 65, -1, 2.5, True, None):
        with pytest.raises(ValueError):
            U.transfer_bases(bad)


def test_axis_ranges_hold_twice_the_unit_cube():
    lo, hi = T.axis_range(np.eye(3, dtype=np.float32))
    assert np.array_equal(lo, [-0.5] * 3) and np.array_equal(hi, [1.5] * 3)
    lo, hi = T.axis_range(np.float32([[0, -1, 0], [1, 0, 0], [0, 0, -1]]))
    assert np.array_equal(lo, [-0.5, -1.5, -1.5]) and np.array_equal(hi, [1.5, 0.5, 0.5])
    corners = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=np.float64)
    for R in T.bases64(64):
        lo, hi = T.axis_range(R)
        u = corners @ R.astype(np.float64)
        width = u.max(0) - u.min(0)
        assert float(np.abs((lo + hi) / 2 - (u.max(0) + u.min(0)) / 2).max()) <= 1e-12
        assert float(np.abs((hi - lo) - 2 * width).max()) <= 1e-12


def test_transfer_colour_refuses_on_the_host():
    """refused before a kernel is asked for (there is none to ask for here)"""
    import torch
    from nn import strotss_utils as U
    img, other = torch.rand(1, 6, 8, 3), torch.rand(1, 5, 9, 3)
    with pytest.raises(ValueError):
        U.transfer_colour(torch.rand(6, 8), other)
    with pytest.raises(ValueError):
        U.transfer_colour(img, torch.rand(5, 9, 1))
    with pytest.raises(ValueError):
        U.transfer_colour(img, other, torch.ones(6, 9), None)
    with pytest.raises(ValueError):
        U.transfer_colour(img, other, None, torch.ones(6, 8))
    with pytest.raises(ValueError, match="1..64"):
        U.transfer_colour(img, other, iters=0)
    for bins in (1, 2, 3, 250, 1022, 4097, 4100, 16.0, True):      # slice t of the targets must start on 16 bytes
        with pytest.raises(ValueError, match="multiple of 4 in 4..4096"):
            U.transfer_colour(img, other, bins=bins)
    bad = img.clone()
    bad[0, 2, 3, 1] = float("nan")
    with pytest.raises(ValueError, match="not finite"):
        U.transfer_colour(bad, other)
    with pytest.raises(ValueError, match="not finite"):
        U.transfer_colour(other, bad * float("inf"))
    with pytest.raises(ValueError, match="style mask counts no pixel"):
        U.transfer_colour(img, other, torch.zeros(6, 8), None)
    with pytest.raises(ValueError, match="content mask counts no pixel"):
        U.transfer_colour(img, other, None, torch.zeros(5, 9))


# ------------------------------------------------------------------ 4. the C ABI refuses before it launches
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_abi_rows_are_additions(lib):
    from nn import _hip
    header = open(os.path.join(ROOT, "include", "strotss_hip.h")).read()
    for name in ("strotss_color_hist", "strotss_color_transfer_table", "strotss_color_transfer_apply",
                 "strotss_color_hist_group"):
        assert name in _hip.SIGNATURES and f"int {name}(" in header
        assert getattr(lib, name).argtypes == _hip.SIGNATURES[name][1]
    assert lib.strotss_abi_version() == 8 == _hip.ABI_VERSION


def test_hist_group_fits_the_lds_budget(lib):
    words, cap = 15360, 8
    for bins in (2, 16, 256, 640, 641, 1024, 1280, 2560, 2561, 4096):
        g = lib.strotss_color_hist_group(bins)
        assert g == max(1, min(cap, words // (3 * bins)))
        assert 4 * 3 * bins * g <= 60 * 1024
    assert lib.strotss_color_hist_group(1024) == 5
    assert [lib.strotss_color_hist_group(b) for b in (1, 0, -4, 4097)] == [0, 0, 0, 0]


def _basis(*values):
    return (C.c_float * 9)(*values)


IDENT = _basis(1, 0, 0, 0, 1, 0, 0, 0, 1)
BAD_BASES = [_basis(1, 0, 0, 0, float("nan"), 0, 0, 0, 1), _basis(1, 0, 0, 0, float("inf"), 0, 0, 0, 1),
             _basis(1, 0, 0, 0, 1.001, 0, 0, 0, 1),            # a column of length 1.001: R^T R - I = 2e-3
             _basis(1, 2e-4, 0, 0, 1, 0, 0, 0, 1),             # two columns 2e-4 from orthogonal
             _basis(0, 0, 0, 0, 0, 0, 0, 0, 0)]


def test_color_hist_refuses_bad_arguments(lib):
    big = 26755                                      # 3 * 26755^2 > INT_MAX
    hist = lib.strotss_color_hist
    assert hist(NULL, NULL, 8, 8, IDENT, 1, 16, P, NULL) == EINVAL
    assert hist(P, NULL, 8, 8, None, 1, 16, P, NULL) == EINVAL
    assert hist(P, NULL, 8, 8, IDENT, 1, 16, NULL, NULL) == EINVAL
    assert hist(P, P, 0, 8, IDENT, 1, 16, P, NULL) == EINVAL
    assert hist(P, P, 8, -1, IDENT, 1, 16, P, NULL) == EINVAL
    assert hist(P, P, big, big, IDENT, 1, 16, P, NULL) == EINVAL
    for bins in (1, 0, -16, 4097):
        assert hist(P, NULL, 8, 8, IDENT, 1, bins, P, NULL) == EINVAL
    two = (C.c_float * 18)(*(list(IDENT) * 2))
    for n in (0, -1, 65):
        assert hist(P, NULL, 8, 8, two, n, 16, P, NULL) == EINVAL
    for bad in BAD_BASES:
        assert hist(P, NULL, 8, 8, bad, 1, 16, P, NULL) == EINVAL
        second = (C.c_float * 18)(*(list(IDENT) + list(bad)))          # every basis of the set is checked
        assert hist(P, NULL, 8, 8, second, 2, 16, P, NULL) == EINVAL
    assert hist(ODD, NULL, 8, 8, IDENT, 1, 16, P, NULL) == EALIGN
    assert hist(P, ODD, 8, 8, IDENT, 1, 16, P, NULL) == EALIGN
    assert hist(P, NULL, 8, 8, IDENT, 1, 16, ODD, NULL) == EALIGN


def test_color_transfer_table_refuses_bad_arguments(lib):
    table = lib.strotss_color_transfer_table
    assert table(NULL, P, IDENT, 16, P, NULL) == EINVAL
    assert table(P, NULL, IDENT, 16, P, NULL) == EINVAL
    assert table(P, P, None, 16, P, NULL) == EINVAL
    assert table(P, P, IDENT, 16, NULL, NULL) == EINVAL
    for bins in (1, 0, -16, 4097):
        assert table(P, P, IDENT, bins, P, NULL) == EINVAL
    for bad in BAD_BASES:
        assert table(P, P, bad, 16, P, NULL) == EINVAL
    assert table(ODD, P, IDENT, 16, P, NULL) == EALIGN
    assert table(P, ODD, IDENT, 16, P, NULL) == EALIGN
    assert table(P, P, IDENT, 16, ODD, NULL) == EALIGN


def test_color_transfer_apply_refuses_bad_arguments(lib):
    big = 26755
    apply = lib.strotss_color_transfer_apply
    assert apply(NULL, NULL, 8, 8, IDENT, P, 16, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 8, 8, None, P, 16, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 8, 8, IDENT, NULL, 16, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 8, 8, IDENT, P, 16, NULL, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 0, 8, IDENT, P, 16, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 8, -3, IDENT, P, 16, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, big, big, IDENT, P, 16, P, None, NULL, NULL) == EINVAL
    for bins in (1, 0, -16, 4097):
        assert apply(P, NULL, 8, 8, IDENT, P, bins, P, None, NULL, NULL) == EINVAL
    assert apply(P, NULL, 8, 8, IDENT, P, 16, P, IDENT, NULL, NULL) == EINVAL          # exactly one of the pair
    assert apply(P, NULL, 8, 8, IDENT, P, 16, P, None, P, NULL) == EINVAL
    for bad in BAD_BASES:
        assert apply(P, NULL, 8, 8, bad, P, 16, P, None, NULL, NULL) == EINVAL
        assert apply(P, NULL, 8, 8, IDENT, P, 16, P, bad, P, NULL) == EINVAL
    assert apply(ODD, NULL, 8, 8, IDENT, P, 16, P, None, NULL, NULL) == EALIGN
    assert apply(P, ODD, 8, 8, IDENT, P, 16, P, None, NULL, NULL) == EALIGN
    assert apply(P, NULL, 8, 8, IDENT, ODD, 16, P, None, NULL, NULL) == EALIGN
    assert apply(P, NULL, 8, 8, IDENT, P, 16, ODD, None, NULL, NULL) == EALIGN
    assert apply(P, NULL, 8, 8, IDENT, P, 16, P, IDENT, ODD, NULL) == EALIGN


# ------------------------------------------------------------------ 5. the command line
def test_parser_takes_transfer_and_its_iterations():
    import run_strotss as RS
    parser = RS.build_parser()
    assert "transfer" in RS.PRESERVE_COLOR_MODES
    args = parser.parse_args(["c.jpg", "s.jpg", "--preserve_color", "transfer"])
    assert args.preserve_color == "transfer" and args.transfer_iters is None
    assert RS._preserve_color_input(args) == "transfer"
    args = parser.parse_args(["c.jpg", "s.jpg", "--preserve_color", "transfer", "--transfer_iters", "20"])
    assert args.transfer_iters == 20 and RS._preserve_color_input(args) == "transfer"
    assert parser.parse_args(["c.jpg", "s.jpg"]).transfer_iters is None
    assert "--transfer_iters" in RS.__doc__ and "transfer" in RS.__doc__.split("--preserve_color {")[1].split("}")[0]


@pytest.mark.parametrize("mode", [None, "match", "luminance"])
def test_transfer_iters_needs_the_mode(mode, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    argv = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg"),
            "--transfer_iters", "5"] + ([] if mode is None else ["--preserve_color", mode])
    with pytest.raises(ValueError, match="--transfer_iters needs --preserve_color transfer"):
        RS.run(RS.build_parser().parse_args(argv))
    video = [str(tmp_path / "no_frames"), argv[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"] + argv[4:]
    with pytest.raises(ValueError, match="--transfer_iters needs --preserve_color transfer"):
        RS.run(RS.build_parser().parse_args(video))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")


@pytest.mark.parametrize("iters", [0, -1, 65])
def test_transfer_iters_out_of_range_is_refused_before_anything_is_loaded(iters, tmp_path):
    import run_strotss as RS
    argv = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg"),
            "--preserve_color", "transfer", "--transfer_iters", str(iters)]
    with pytest.raises(ValueError, match="1..64"):
        RS.run(RS.build_parser().parse_args(argv))
    assert not os.path.exists(tmp_path / "out.jpg")


def test_transfer_is_refused_on_several_gpus_before_anything_is_loaded(monkeypatch, tmp_path):
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    mode = ["--preserve_color", "transfer", "--transfer_iters", "3"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    with pytest.raises(ValueError, match="--strips"):
        RS.run(RS.build_parser().parse_args(missing + mode + ["--strips"]))
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    with pytest.raises(ValueError, match="--strips"):
        RS.run(RS.build_parser().parse_args(video + mode + ["--strips"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(missing + mode))
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(video + mode))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")
