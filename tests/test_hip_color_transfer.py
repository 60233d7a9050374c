"""Colour distribution transfer on the MI355X: each of the three kernels against the float64
restatement (tests/_color_transfer_ref.py) on its own -- the histograms exactly where the arithmetic is exact and bracketed
where float32 cannot decide a bin, the tables from host-made histograms, the application from host-made tables --, then
transfer_colour end to end and --preserve_color transfer through the command line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_transfer_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
SMALL = [(1, 1), (1, 3), (42, 63), (48, 64), (257, 300)]
BIG = (768, 1024)                                   # more groups of 4 pixels than the grid has threads: the blocks stride
MASKS = [None, "random", "ones", "single"]
BINS = [2, 16, 1024, 4096]
BASES = T.bases64(64)
# every corner size under every mask; the large size, where the blocks stride, unmasked and under a random mask
IMAGES = [(hw, kind) for hw in SMALL for kind in MASKS] + [(BIG, None), (BIG, "random")]
PERMUTED = np.float32([[0, -1, 0], [0, 0, 1], [-1, 0, 0]])          # a signed permutation: exact arithmetic, like I


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _counts(a):
    return torch.as_tensor(np.ascontiguousarray(np.asarray(a, dtype=np.int64).astype(np.int32)), device=DEV)


def _image(h, w, seed, lo=-0.1, hi=1.1):
    return (lo + (hi - lo) * np.random.default_rng(seed).random((h, w, 3))).astype(np.float32)


def _mask(kind, h, w, seed=5):
    if kind is None:
        return None
    rng = np.random.default_rng(seed + h * w)
    if kind == "ones":
        return np.ones((h, w), dtype=np.float32)
    if kind == "single":
        m = np.zeros((h, w), dtype=np.float32)
        m[int(rng.integers(h)), int(rng.integers(w))] = 1.0
        return m
    m = (rng.random((h, w)) < 0.5).astype(np.float32)
    m[h // 2, w // 2] = 1.0                 # never empty
    return m


def _group(bins):
    from nn import _hip
    return int(_hip.lib().strotss_color_hist_group(bins))


def _hist(x, bases, bins, m):
    from nn import _ops
    out = _ops.color_hist(_dev(x), bases, bins, None if m is None else _dev(m))
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. the histograms
@pytest.mark.parametrize("hw,kind", IMAGES)
def test_color_hist_is_exact_on_dyadic_colours(hw, kind):
    """R = I or a signed permutation, colours k / 256 and a power-of-two bin count: u, ub - lo and the product with scale
    are exact in float32, so every count is numpy.bincount's"""
    h, w = hw
    x = (np.random.default_rng(h * w).integers(0, 257, (h, w, 3)) / 256.0).astype(np.float32)
    m = _mask(kind, h, w)
    bases = np.stack([np.eye(3, dtype=np.float32), PERMUTED])
    for bins in BINS:
        got = _hist(x, bases, bins, m).cpu().numpy()
        for n, R in enumerate(bases):
            assert np.array_equal(got[n], T.hist64(x, R, bins, m)), (bins, n)


def _check_bracket(x, m, bases, bins):
    got = _hist(x, bases, bins, m)
    again = _hist(x, bases, bins, m)
    assert got.dtype == torch.int32 and tuple(got.shape) == (len(bases), 3, bins)
    assert torch.equal(got, again)                                   # the same bits on every run
    got = got.cpu().numpy().astype(np.int64)
    n_counted = int(T.counted(m, x.shape[0] * x.shape[1]).sum())
    shares = []
    for n, R in enumerate(bases):
        lower, upper, share = T.hist_bounds(x, R, bins, m)
        assert (got[n].sum(1) == n_counted).all(), (bins, n)
        assert (lower <= got[n]).all() and (got[n] <= upper).all(), (bins, n)
        shares.append(share)
    # The bracket is not loose: of all the (pixel, axis) pairs of the call, uniform inputs flag 2 delta = bins 2^-19, and
    # at most 2 % may be flagged.  Below 50 pairs (1 x 1 and 1 x 3 images, single-pixel masks with few bases) one flagged
    # pair is already above 2 %: there at most one pair may be.
    pairs = 3 * n_counted * len(bases)
    flagged = int(round(float(np.mean(shares)) * pairs))
    assert flagged <= (0.02 * pairs if pairs >= 50 else 1), (flagged, pairs)
    return float(np.mean(shares))


@pytest.mark.parametrize("bins", BINS)
@pytest.mark.parametrize("hw", SMALL)
def test_color_hist_brackets_float64_on_either_side_of_the_group_size(hw, bins):
    h, w = hw
    g = _group(bins)
    worst = 0.0
    for n_bases, kind in ((g, None), (g + 1, "random")):
        worst = max(worst, _check_bracket(_image(h, w, h + w + bins), _mask(kind, h, w), BASES[3:3 + n_bases], bins))
    print(f"{h} x {w}, {bins} bins, {g} and {g + 1} bases: at most {100 * worst:.3f} % of the pixels flagged")


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("n_bases", [1, 64])
def test_color_hist_brackets_float64_at_one_and_64_bases(n_bases, kind):
    h, w = 42, 63
    for bins in BINS:
        _check_bracket(_image(h, w, 7 + bins), _mask(kind, h, w), BASES[:n_bases], bins)


def test_color_hist_brackets_float64_above_the_grid_cap():
    h, w = BIG
    g = _group(1024)
    worst = _check_bracket(_image(h, w, 11), _mask("random", h, w), BASES[:g + 1], 1024)
    print(f"{h} x {w}, 1024 bins, {g + 1} bases: {100 * worst:.3f} % of the pixels flagged")


# ------------------------------------------------------------------ 2. the table
def _hist_pair(kind, bins, rng):
    """(source, target) (3, bins) integer histograms, totals <= INT_MAX / 3"""
    if kind == "random":
        return rng.integers(0, 1000, (3, bins)), rng.integers(0, 1000, (3, bins))
    if kind == "spiky":                              # every other bin empty, the two combs interleaved
        hs, hc = rng.integers(1, 1000, (3, bins)), rng.integers(1, 1000, (3, bins))
        hs[:, 1::2] = 0
        hc[:, ::2] = 0
        return hs, hc
    if kind in ("single_src", "single_dst"):
        one, many = np.zeros((3, bins), dtype=np.int64), rng.integers(0, 1000, (3, bins))
        one[np.arange(3), rng.integers(0, bins, 3)] = 12345
        return (one, many) if kind == "single_src" else (many, one)
    if kind == "totals_100x":
        return rng.integers(0, 30, (3, bins)) + 1, 100 * (rng.integers(0, 30, (3, bins)) + 1)
    if kind == "near_int_max":                       # totals just below INT_MAX / 3: the 64-bit products near 2^59
        cap = (2 ** 31 - 1) // 3
        hs, hc = rng.integers(0, cap // bins, (3, bins)), rng.integers(0, cap // bins, (3, bins))
        hs[:, 0] += cap - hs.sum(1)
        hc[:, -1] += cap - hc.sum(1)
        return hs, hc
    if kind == "one_axis_empty":
        hs, hc = rng.integers(0, 1000, (3, bins)), rng.integers(0, 1000, (3, bins))
        hs[0], hc[2] = 0, 0
        return hs, hc
    raise ValueError(kind)


@pytest.mark.parametrize("kind", ["random", "spiky", "single_src", "single_dst", "totals_100x", "near_int_max",
                                  "one_axis_empty"])
@pytest.mark.parametrize("bins", BINS)
def test_color_transfer_table_matches_float64(bins, kind):
    """Everything before the one division is an integer; the float64 expression lo + (i + frac) (hi - lo) / bins is then
    rounded once to float32: half an ulp of a value of at most max(|lo|, |hi|), 2^-24 of it, and as much again for the
    float64 roundings on either side of a tie -- 2^-23 max(|lo|, |hi|)."""
    from nn import _ops
    rng = np.random.default_rng(bins + len(kind))
    hs, hc = _hist_pair(kind, bins, rng)
    assert hs.sum(1).max() <= (2 ** 31 - 1) // 3 and hc.sum(1).max() <= (2 ** 31 - 1) // 3
    for R in (BASES[0], BASES[3]):
        got = _ops.color_transfer_table(_counts(hs), _counts(hc), R, bins)
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.float64)
        ref = T.table64(hs, hc, R, bins)
        lo, hi = T.axis_range(R)
        bound = 2.0 ** -23 * np.maximum(np.abs(lo), np.abs(hi))[:, None]
        assert np.isfinite(got).all() and got.shape == (3, bins + 1)
        assert (np.abs(got - ref) <= bound).all(), float((np.abs(got - ref) / bound).max())
        assert (np.diff(got, axis=1) >= 0).all()


# ------------------------------------------------------------------ 3. the application
def _tables(kind, R, bins, rng):
    """a host-made (3, bins + 1) float32 table"""
    if kind == "identity":
        return T.identity_table(R, bins).astype(np.float32)
    if kind == "steep":                              # all of the source in one bin: the table crosses the target in it
        hs, hc = np.zeros((3, bins), dtype=np.int64), rng.integers(1, 100, (3, bins))
        hs[:, bins // 2] = 1000
    else:
        hs, hc = rng.integers(0, 100, (3, bins)), rng.integers(0, 100, (3, bins))
    return T.table64(hs, hc, R, bins).astype(np.float32)


@pytest.mark.parametrize("hw,kind", IMAGES)
def test_color_transfer_apply_matches_float64(hw, kind):
    from nn import _ops
    h, w = hw
    rng = np.random.default_rng(h * w + 2)
    x, m = _image(h, w, h + w + 1), _mask(kind, h, w)
    xd, md = _dev(x), None if m is None else _dev(m)
    cases = [(16, "random"), (1024, "random"), (1024, "steep"), (4096, "identity"), (2, "random")]
    for n, (bins, table_kind) in enumerate(cases if hw != BIG else cases[1:3]):
        R, following = BASES[n + 1], BASES[n + 2]
        table = _tables(table_kind, R, bins, rng)
        td = _dev(table)
        out = _ops.color_transfer_apply(xd, R, td, bins, md)
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        ref, d = T.apply64(x, R, table, bins, m)
        bound = T.apply_bound(x, R, table, bins, d)
        err = np.abs(got - ref)
        print(f"{h} x {w} mask {kind}, {bins} bins, {table_kind} table (slopes {np.round(T.slopes(table, R, bins), 1)}): "
              f"largest error / bound {float((err / bound).max()):.3f}")
        assert (err <= bound).all()
        if m is not None:                            # uncounted pixels: the input, bit for bit
            assert np.array_equal(got[m == 0].view(np.int32), x[m == 0].view(np.int32))
        if table_kind != "identity":
            assert not np.array_equal(got[T.counted(m, h * w).reshape(h, w)], x[T.counted(m, h * w).reshape(h, w)])
        # in place, and with the next histogram fused: the same image, and strotss_color_hist of it on the next basis
        inplace = xd.clone()
        hist = torch.full((3, bins), -1, dtype=torch.int32, device=DEV)              # the call clears it
        assert _ops.color_transfer_apply(inplace, R, td, bins, md, out=inplace, next_basis=following,
                                         next_hist=hist) is inplace
        torch.cuda.synchronize()
        assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))
        assert torch.equal(hist, _ops.color_hist(out, following, bins, md)[0])


# ------------------------------------------------------------------ 4. the whole transfer
def _orderings(name, start, affine, moved):
    print(f"{name}: sliced Wasserstein distance to the content {start:.4f} before, {affine:.4f} after the affine match, "
          f"{moved:.4f} after the transfer")
    assert moved < affine
    assert moved < 0.1 * start


def test_transfer_colour_on_the_golden_pair():
    from nn import strotss_utils as U
    from nn import utils
    content, style = utils.load_image(CONTENT, max_size=64), utils.load_image(STYLE, max_size=64)
    out = U.transfer_colour(style, content)
    again = U.transfer_colour(style, content)
    matched = U.match_colour(style, content)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(style.shape)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))              # the same bits on every run
    c, s = content[0].cpu().numpy(), style[0].cpu().numpy()
    _orderings("golden pair at 64 px", T.swd(s, c), T.swd(matched[0].cpu().numpy(), c), T.swd(out[0].cpu().numpy(), c))


@pytest.mark.parametrize("bins", [4, 16, 252, 4096])
def test_transfer_colour_at_other_bin_counts(bins):
    """iteration t reads the slice t of the content's (iters, 3, bins) histograms: with three iterations and bin counts
    that are no multiple of 16 or 64, the slices start at odd multiples of 16 bytes.  The first basis is I, the
    one-dimensional matching of each channel brings that channel's distribution to the content's up to the bin width, and
    the two later bases do not undo it: the distance to the content falls.  How far is not asserted."""
    from nn import strotss_utils as U
    rng = np.random.default_rng(31)
    content = (rng.random((42, 63, 3)) * np.float32([0.9, 0.5, 0.3])).astype(np.float32)
    style = (0.3 + 0.6 * rng.random((33, 50, 3))).astype(np.float32)
    sm = _mask("random", 33, 50)
    out = U.transfer_colour(_dev(style), _dev(content), _dev(sm), None, iters=3, bins=bins)
    again = U.transfer_colour(_dev(style), _dev(content), _dev(sm), None, iters=3, bins=bins)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    got = out.cpu().numpy()
    assert np.isfinite(got).all() and got.shape == style.shape
    assert np.array_equal(got[sm == 0].view(np.int32), style[sm == 0].view(np.int32))
    start, moved = T.swd(style, content, sm, None), T.swd(got, content, sm, None)
    print(f"{bins} bins, 3 iterations: sliced Wasserstein distance to the content {start:.4f} before, {moved:.4f} after")
    assert moved < start


def _halves(h, w, gap=0):
    """(left, right) (h, w, 1) float 0/1 masks as strotss_utils.load_mask returns them, `gap` columns in no region"""
    left, right = np.zeros((h, w, 1), dtype=np.float32), np.zeros((h, w, 1), dtype=np.float32)
    left[:, :w // 2 - gap] = 1.0
    right[:, w // 2 + gap:] = 1.0
    return [torch.from_numpy(left), torch.from_numpy(right)]


def test_transfer_region_by_region():
    import run_strotss as RS
    h, w, sh, sw = 48, 64, 40, 72
    rng = np.random.default_rng(21)
    content = _image(h, w, 22, 0.0, 1.0)
    content[:, :w // 2] *= np.float32([1.0, 0.4, 0.3])                # a red half and a blue half
    content[:, w // 2:] *= np.float32([0.3, 0.5, 1.0])
    style = (0.5 + 0.2 * rng.standard_normal((sh, sw, 3))).astype(np.float32)
    c_masks, s_masks = _halves(h, w), _halves(sh, sw, gap=4)
    args = RS._resolve(RS.build_parser().parse_args(["c.jpg", "s.jpg", "--preserve_color", "transfer"]))
    styles, cd = [_dev(style)[None]], _dev(content)[None]
    (out,) = RS._recolour_styles(args, styles, cd, c_masks, s_masks)
    (again,) = RS._recolour_styles(args, styles, cd, c_masks, s_masks)
    (matched,) = RS._match_styles(styles, cd, c_masks, s_masks)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, sh, sw, 3)
    assert torch.equal(out.view(torch.int32), again.view(torch.int32))
    got, aff = out[0].cpu().numpy(), matched[0].cpu().numpy()
    covered = np.zeros((sh, sw), dtype=bool)
    for r, (cm, sm) in enumerate(zip(c_masks, s_masks)):
        cm, sm = cm[..., 0].numpy(), sm[..., 0].numpy()
        covered |= sm != 0
        _orderings(f"region {r}", T.swd(style, content, sm, cm), T.swd(aff, content, sm, cm), T.swd(got, content, sm, cm))
    assert (~covered).any()
    assert np.array_equal(got[~covered].view(np.int32), style[~covered].view(np.int32))       # in no region: untouched


# ------------------------------------------------------------------ 5. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]
TRANSFER = ["--preserve_color", "transfer"]


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def _content_at_output_size(RS, path):
    args = RS.build_parser().parse_args([path, STYLE] + SETTINGS)
    return RS._frame_at_result_size(RS._resolve(args), path).cpu().numpy().astype(np.float64)


def test_cli_transfer_single_image(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs = {}
    for name, extra in (("plain", []), ("transfer", TRANSFER), ("short", TRANSFER + ["--transfer_iters", "2"])):
        outs[name] = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", outs[name]] + SETTINGS + extra))
    c = _content_at_output_size(RS, CONTENT)
    imgs = {k: _read(v) for k, v in outs.items()}
    assert all(im.shape == c.shape for im in imgs.values())
    D = {k: T.swd(im, c) for k, im in imgs.items()}
    print("single image, golden pair at 64 px: " + ", ".join(f"D({k}) = {D[k]:.4f}" for k in imgs))
    assert D["transfer"] < D["plain"]
    assert open(outs["short"], "rb").read() != open(outs["transfer"], "rb").read()
    # without the flags nothing changes: a namespace that has neither attribute writes the plain run's bytes
    ns = RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "bare.jpg")] + SETTINGS)
    assert ns.preserve_color is None and ns.transfer_iters is None
    delattr(ns, "preserve_color")
    delattr(ns, "transfer_iters")
    RS.run(ns)
    assert open(tmp_path / "bare.jpg", "rb").read() == open(outs["plain"], "rb").read()
    assert open(outs["transfer"], "rb").read() != open(outs["plain"], "rb").read()


def _texture(h, w, seed, tint):
    """a smooth random texture (h, w, 3) in [0, 1], its channels scaled by `tint`"""
    rng = np.random.default_rng(seed)
    coarse = rng.random((h // 6 + 2, w // 6 + 2, 3))
    ys, xs = np.linspace(0, coarse.shape[0] - 1.001, h), np.linspace(0, coarse.shape[1] - 1.001, w)
    y0, x0 = ys.astype(int), xs.astype(int)
    fy, fx = (ys - y0)[:, None, None], (xs - x0)[None, :, None]
    top = coarse[y0][:, x0] * (1 - fx) + coarse[y0][:, x0 + 1] * fx
    bot = coarse[y0 + 1][:, x0] * (1 - fx) + coarse[y0 + 1][:, x0 + 1] * fx
    smooth = top * (1 - fy) + bot * fy
    return np.clip((smooth * 0.8 + 0.1 * rng.random((h, w, 3))) * np.asarray(tint), 0.0, 1.0)


def test_cli_transfer_video(tmp_path, monkeypatch):
    """three crops of one reddish texture, moved by (3, 2) pixels per frame, against a bluish style"""
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, (h, w), (dx, dy) = tmp_path / "frames", (48, 64), (3, 2)
    os.makedirs(frames)
    big = _texture(h + 3 * dy + 8, w + 3 * dx + 8, 0, (1.0, 0.55, 0.35))
    paths = []
    for t in range(3):
        oy, ox = (3 - t) * dy, (3 - t) * dx
        paths.append(str(frames / f"frame_{t + 1:02d}.png"))
        Image.fromarray((big[oy:oy + h, ox:ox + w] * 255).round().astype(np.uint8)).save(paths[-1])
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    outs = {}
    for name, extra in (("plain", []), ("transfer", TRANSFER)):
        outs[name] = tmp_path / name
        RS.run(RS.build_parser().parse_args([str(frames), style, "--video", "--compute_flow", "-o", str(outs[name])]
                                            + SETTINGS + extra))
    for p in paths:
        stem = os.path.splitext(os.path.basename(p))[0]
        c = _content_at_output_size(RS, p)
        d_plain, d_transfer = (T.swd(_read(outs[k] / f"{stem}.jpg"), c) for k in ("plain", "transfer"))
        print(f"{stem}: D(plain) = {d_plain:.4f}, D(transfer) = {d_transfer:.4f}")
        assert d_transfer < d_plain, stem


def test_cli_transfer_with_auto_masks(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs = {}
    for name, extra in (("auto", []), ("transfer", TRANSFER)):
        outs[name] = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", outs[name], "--auto_masks", "2"] + SETTINGS + extra))
    c = _content_at_output_size(RS, CONTENT)
    imgs = {k: _read(v) for k, v in outs.items()}
    assert all(im.shape == c.shape for im in imgs.values())
    D = {k: T.swd(im, c) for k, im in imgs.items()}
    print("--auto_masks 2: " + ", ".join(f"D({k}) = {D[k]:.4f}" for k in imgs))
    assert D["transfer"] < D["auto"]
    assert open(outs["transfer"], "rb").read() != open(outs["auto"], "rb").read()
