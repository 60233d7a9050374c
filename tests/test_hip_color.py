"""Colour preservation on the MI355X: the three kernels element by element against the float64
restatement (tests/_color_ref.py) at the step shapes and the corner sizes, match_colour end to end on the golden pair,
--preserve_color through the command line (single image, --video --compute_flow, masks)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
SHAPES = [(48, 64), (42, 63), (257, 300), (768, 1024), (1, 1), (1, 3)]
MASKS = [None, "random", "ones", "single"]
U24 = 2.0 ** -24


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _image(h, w, seed, lo=0.0, hi=1.0):
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


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("hw", SHAPES)
def test_color_stats_matches_float64(hw, kind):
    from nn import _ops
    h, w = hw
    x, m = _image(h, w, h + w), _mask(kind, h, w)
    xd, md = _dev(x), None if m is None else _dev(m)
    got = _ops.color_stats(xd, md)
    again = _ops.color_stats(xd, md)
    torch.cuda.synchronize()
    assert got.dtype == torch.float64 and tuple(got.shape) == (10,)
    assert torch.equal(got.view(torch.int64), again.view(torch.int64))          # the same bits on every run
    got = got.cpu().numpy()
    ref = R.sums64(x, m, exact=True)
    # every term is >= 0: N * 2^-53 relative is the worst case of any summation order in float64 (N = h w)
    rel = np.abs(got - ref) / np.maximum(np.abs(ref), 1e-300)
    print(f"{h} x {w} mask {kind}: largest relative error {rel.max():.3e}, bound {h * w * 2.0 ** -53:.3e}")
    assert (np.abs(got - ref) <= h * w * 2.0 ** -53 * np.abs(ref)).all(), (got, ref)
    assert got[0] == (h * w if m is None else m.sum())


def test_color_stats_of_an_empty_mask_raises_on_the_host():
    from nn import _ops
    from nn import strotss_utils as U
    x = _dev(_image(42, 63, 1))
    zero = torch.zeros(42, 63, device=DEV)
    got = _ops.color_stats(x, zero).cpu().numpy()
    assert got[0] == 0.0 and not got.any()
    with pytest.raises(ValueError, match="W == 0"):
        U.colour_statistics(x, zero)
    # the workspace is left ready: the next call of that size is right
    mu, sigma = U.colour_statistics(x)
    mu_ref, sigma_ref = R.stats64(x.cpu().numpy(), exact=True)
    assert float(np.abs(mu - mu_ref).max()) <= 1e-12 and float(np.abs(sigma - sigma_ref).max()) <= 1e-12


@pytest.mark.parametrize("kind", MASKS)
@pytest.mark.parametrize("hw", SHAPES)
def test_color_affine_matches_float64(hw, kind):
    from nn import _ops
    h, w = hw
    rng = np.random.default_rng(h * w + 1)
    x, m = _image(h, w, h + w + 1, -0.2, 1.2), _mask(kind, h, w)
    A = (np.eye(3) + 0.6 * rng.standard_normal((3, 3))).astype(np.float32)
    b = rng.uniform(-0.5, 0.5, 3).astype(np.float32)
    xd, md = _dev(x), None if m is None else _dev(m)
    out = _ops.color_affine(xd, A, b, md)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = R.affine64(x, A, b, m)                     # float64 with the same float32-rounded A, b
    err = np.abs(got - ref)
    bound = 4 * U24 * R.affine_bound(x, A, b)        # four float32 roundings, fused or not
    print(f"{h} x {w} mask {kind}: largest error / bound {float((err / bound).max()):.3f}")
    assert (err <= bound).all()
    if m is not None:                                # masked-out pixels: the input, bit for bit
        assert np.array_equal(got[m == 0].view(np.int32), x[m == 0].view(np.int32))
        assert not np.array_equal(got[m != 0], x[m != 0])
    inplace = xd.clone()
    assert _ops.color_affine(inplace, A, b, md, out=inplace) is inplace
    torch.cuda.synchronize()
    assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))


@pytest.mark.parametrize("hw", SHAPES)
def test_luma_merge_matches_float64(hw):
    from nn import _ops
    h, w = hw
    r, c = _image(h, w, h + w + 2), _image(h, w, h + w + 3)
    rd, cd = _dev(r), _dev(c)
    out = _ops.luma_merge(rd, cd)
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ref = R.luma_merge64(r, c)
    scale = np.abs(c.astype(np.float64)) + (np.abs(R.luma64(r)) + np.abs(R.luma64(c)))[..., None]
    err = np.abs(got - ref)
    print(f"{h} x {w}: largest error / bound {float((err / (8 * U24 * scale)).max()):.3f}")
    assert (err <= 8 * U24 * scale).all()
    same = _ops.luma_merge(cd, cd).cpu().numpy()     # result == content: the content
    assert (np.abs(same - c) <= 8 * U24 * (np.abs(c.astype(np.float64)) + 2 * np.abs(R.luma64(c))[..., None])).all()
    inplace = rd.clone()
    _ops.luma_merge(inplace, cd, out=inplace)
    torch.cuda.synchronize()
    assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))


# ------------------------------------------------------------------ 2. the operator surface
def test_operator_surface_against_the_restatement():
    from nn import strotss_utils as U
    x, m = _image(42, 63, 11), _mask("random", 42, 63)
    mu, sigma = U.colour_statistics(_dev(x)[None], _dev(m))
    mu_ref, sigma_ref = R.stats64(x, m, exact=True)
    assert mu.dtype == np.float64 and sigma.shape == (3, 3)
    assert float(np.abs(mu - mu_ref).max()) <= 1e-12 and float(np.abs(sigma - sigma_ref).max()) <= 1e-12
    r, c = _image(42, 63, 12), _image(42, 63, 13)
    out = U.luminance_merge(_dev(r)[None], _dev(c))
    assert tuple(out.shape) == (1, 42, 63, 3)
    got = out[0].cpu().numpy().astype(np.float64)
    # the exact statement, on the float image: the result's luma, the content's chroma (to float32 rounding)
    assert float(np.abs(R.luma64(got) - R.luma64(r)).max()) <= 16 * U24
    assert R.chroma_distance(got, c) <= 16 * U24 < R.chroma_distance(r, c)
    with pytest.raises(ValueError):
        U.luminance_merge(_dev(r), _dev(c[:-1]))
    with pytest.raises(ValueError):
        U.colour_statistics(_dev(np.full((4, 4, 3), np.nan, dtype=np.float32)))


@pytest.mark.parametrize("max_size", [64, None])
def test_match_colour_on_the_golden_pair(max_size):
    """The budget is the float32 storage of s': 2^-23 absolute on the mean, 2^-21 on covariance entries."""
    from nn import strotss_utils as U
    from nn import utils
    content, style = utils.load_image(CONTENT, max_size=max_size), utils.load_image(STYLE, max_size=max_size)
    out = U.match_colour(style, content)
    torch.cuda.synchronize()
    assert tuple(out.shape) == tuple(style.shape)
    c64, s64 = content[0].cpu().numpy(), style[0].cpu().numpy()
    mu_c, sigma_c = R.stats64(c64, exact=True)
    mu_s, sigma_s = R.stats64(s64, exact=True)
    A, _ = R.transform64(mu_s, sigma_s, mu_c, sigma_c)
    mu, sigma = R.stats64(out[0].cpu().numpy(), exact=True)
    e_mu, e_cov = float(np.abs(mu - mu_c).max()), float(np.abs(sigma - R.expected_cov(sigma_c, A)).max())
    print(f"max_size {max_size}: style {tuple(style.shape)}, mean error {e_mu:.3e} (budget {2.0 ** -23:.3e}), covariance "
          f"error {e_cov:.3e} (budget {2.0 ** -21:.3e}); before matching {np.abs(mu_s - mu_c).max():.3e} / "
          f"{np.abs(sigma_s - sigma_c).max():.3e}")
    assert e_mu <= 2.0 ** -23
    assert e_cov <= 2.0 ** -21
    # the kernel's image is the restatement's, element by element
    ref, A64, b64 = R.match64(s64, c64)
    A32, b32 = A64.astype(np.float32), b64.astype(np.float32)
    err = np.abs(out[0].cpu().numpy() - R.affine64(s64, A32, b32))
    assert (err <= 6 * U24 * R.affine_bound(s64, A32, b32)).all()      # 4 + 2: an A or b one float32 ulp apart at most


def _halves(h, w, gap=0):
    """(left, right) (h, w, 1) float 0/1 masks as strotss_utils.load_mask returns them, `gap` columns in no region"""
    left, right = np.zeros((h, w, 1), dtype=np.float32), np.zeros((h, w, 1), dtype=np.float32)
    left[:, :w // 2 - gap] = 1.0
    right[:, w // 2 + gap:] = 1.0
    return [torch.from_numpy(left), torch.from_numpy(right)]


def test_match_region_by_region():
    import run_strotss as RS
    h, w, sh, sw = 48, 64, 40, 72
    rng = np.random.default_rng(21)
    content = _image(h, w, 22)
    content[:, :w // 2] *= np.float32([1.0, 0.4, 0.3])                # a red half and a blue half
    content[:, w // 2:] *= np.float32([0.3, 0.5, 1.0])
    style = (0.5 + 0.2 * rng.standard_normal((sh, sw, 3))).astype(np.float32)
    c_masks, s_masks = _halves(h, w), _halves(sh, sw, gap=4)
    (out,) = RS._match_styles([_dev(style)[None]], _dev(content)[None], c_masks, s_masks)
    torch.cuda.synchronize()
    assert tuple(out.shape) == (1, sh, sw, 3)
    got = out[0].cpu().numpy()
    covered = np.zeros((sh, sw), dtype=bool)
    for cm, sm in zip(c_masks, s_masks):
        cm, sm = cm[..., 0].numpy(), sm[..., 0].numpy()
        covered |= sm != 0
        mu_c, sigma_c = R.stats64(content, cm, exact=True)
        A, b = R.transform64(*R.stats64(style, sm, exact=True), mu_c, sigma_c)
        mu, sigma = R.stats64(got, sm, exact=True)
        # s' as stored = the exact A s + b plus e, |e_i| <= E_i = 5 * 2^-24 * max_p (|b_i| + sum_j |A_ij| |s_j(p)|): A and b
        # rounded once and the kernel's four roundings.  Then |mean error_i| <= E_i and, by Cauchy-Schwarz,
        # |cov error_ij| <= std_i E_j + std_j E_i + E_i E_j.
        E = 5 * U24 * R.affine_bound(style, A, b)[sm != 0].max(0)
        std = np.sqrt(np.diag(R.expected_cov(sigma_c, A)))
        assert (np.abs(mu - mu_c) <= E).all(), (mu - mu_c, E)
        assert (np.abs(sigma - R.expected_cov(sigma_c, A)) <= np.outer(std, E) + np.outer(E, std) + np.outer(E, E)).all()
    assert (~covered).any()
    assert np.array_equal(got[~covered].view(np.int32), style[~covered].view(np.int32))       # in no region: untouched
    assert not np.array_equal(got[covered], style[covered])


# ------------------------------------------------------------------ 3. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def _content_at_output_size(RS, path):
    args = RS.build_parser().parse_args([path, STYLE] + SETTINGS)
    return RS._frame_at_result_size(RS._resolve(args), path).cpu().numpy().astype(np.float64)


def test_cli_preserve_color_single_image(tmp_path, monkeypatch):
    """Orderings against the plain run of the same tree; the sizes of the gaps are recorded in DESIGN.md section 15, not
    asserted."""
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs = {}
    for name, extra in (("plain", []), ("match", ["--preserve_color", "match"]),
                        ("luminance", ["--preserve_color", "luminance"])):
        outs[name] = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", outs[name]] + SETTINGS + extra))
    c = _content_at_output_size(RS, CONTENT)
    imgs = {k: _read(v) for k, v in outs.items()}
    assert all(im.shape == c.shape for im in imgs.values())
    D = {k: R.colour_distance(im, c) for k, im in imgs.items()}
    Cd = {k: R.chroma_distance(im, c) for k, im in imgs.items()}
    print("single image, golden pair at 64 px: " + ", ".join(f"D({k}) = {D[k]:.4f}, C({k}) = {Cd[k]:.4f}" for k in imgs))
    assert D["match"] < D["plain"]
    assert Cd["luminance"] < Cd["plain"]
    # without the flag nothing changes: a namespace that has no such attribute and one that has None write the same bytes
    ns = RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "bare.jpg")] + SETTINGS)
    assert ns.preserve_color is None
    delattr(ns, "preserve_color")
    RS.run(ns)
    assert open(tmp_path / "bare.jpg", "rb").read() == open(outs["plain"], "rb").read()
    assert open(outs["match"], "rb").read() != open(outs["plain"], "rb").read()
    assert open(outs["luminance"], "rb").read() != open(outs["plain"], "rb").read()


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


def _moved_frames(dirpath, n_frames=3, h=48, w=64, shift=(3, 2)):
    """n_frames crops of one reddish texture, moved by `shift` pixels per frame -> the frames' paths"""
    from PIL import Image
    dx, dy = shift
    big = _texture(h + n_frames * dy + 8, w + n_frames * dx + 8, 0, (1.0, 0.55, 0.35))
    os.makedirs(dirpath, exist_ok=True)
    paths = []
    for t in range(n_frames):
        oy, ox = (n_frames - t) * dy, (n_frames - t) * dx
        paths.append(os.path.join(dirpath, f"frame_{t + 1:02d}.png"))
        Image.fromarray((big[oy:oy + h, ox:ox + w] * 255).round().astype(np.uint8)).save(paths[-1])
    return paths


def test_cli_preserve_color_video(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    outs = {}
    for name, extra in (("plain", []), ("match", ["--preserve_color", "match"]),
                        ("luminance", ["--preserve_color", "luminance"])):
        outs[name] = tmp_path / name
        RS.run(RS.build_parser().parse_args([frames, style, "--video", "--compute_flow", "-o", str(outs[name])]
                                            + SETTINGS + extra))
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    for name in outs:
        assert sorted(os.listdir(outs[name])) == sorted(s + ".jpg" for s in stems)
    for p, s in zip(paths, stems):
        c = _content_at_output_size(RS, p)
        plain, match, lum = (_read(outs[k] / f"{s}.jpg") for k in ("plain", "match", "luminance"))
        d_plain, d_match = R.colour_distance(plain, c), R.colour_distance(match, c)
        c_plain, c_lum = R.chroma_distance(plain, c), R.chroma_distance(lum, c)
        print(f"{s}: D(plain) = {d_plain:.4f}, D(match) = {d_match:.4f}, C(plain) = {c_plain:.4f}, C(luminance) = {c_lum:.4f}")
        assert d_match < d_plain, s
        assert c_lum < c_plain, s
