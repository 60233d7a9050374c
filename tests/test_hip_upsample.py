"""Guided upsampling on the MI355X: strotss_guided_upsample element by element against the float64
restatement (tests/_upsample_ref.py) within E_round + E_stat, both modes, at exact, odd, anisotropic and degenerate size pairs,
at the apply kernel's tile edges and with more tiles than its grid; bit equality with strotss_guided_smooth at equal sizes,
repeatability, a side stream, the refusals of the entry on real buffers, and --output_size through the command line (single
image, with --preserve_color luminance, --video --compute_flow)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as CR  # noqa: E402
import _upsample_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
TILE = 1024                          # UPS_TILE: the apply kernel's tile is 1024 consecutive pixels of the flat image
MAX_GRID = 1 << 12                   # UPS_MAX_GRID
# (h, w) -> (H, W): exact factor 4 | just under 2, odd width | anisotropic, non-integer | equal | one pixel | one row |
# H W one below, on and above the tile (a tile is a run of the flat image: its "height and width" are H W)
SHAPES = [((12, 16), (48, 64)), ((21, 32), (42, 63)), ((42, 63), (257, 300)), ((5, 7), (5, 7)), ((1, 1), (3, 5)),
          ((1, 3), (1, 300)), ((11, 31), (33, 31)), ((8, 8), (32, 32)), ((5, 41), (25, 41)), ((2, 2), (1024, 2))]
RADII = [1, 4, 64]
EPSILONS = [1e-2, 1e-4]
U24 = 2.0 ** -24
EINVAL, EALIGN = -1, -2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------ 1. the kernels
def test_tile_shapes_sit_on_the_tile_edges():
    sizes = sorted(H * W for _, (H, W) in SHAPES)
    assert {TILE - 1, TILE, TILE + 1, 2 * TILE} <= set(sizes)


@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("lo,hi", SHAPES)
def test_guided_upsample_matches_float64(lo, hi, r):
    """|out - ref| <= E_round + E_stat per element (tests/_upsample_ref.py: error_budgets; derivation in DESIGN.md section
    27), and the statistics condition max E_stat <= max E_round, both modes, both eps"""
    from nn import _ops
    p, I_lo, I_hi = R.test_images(*lo, *hi, 1000 * r + lo[0] + hi[1])
    if lo == hi:
        I_hi = I_lo
    pd, lod, hid = _dev(p), _dev(I_lo), _dev(I_hi)
    for eps in EPSILONS:
        ref = R.coefficients(p, I_lo, r, eps)
        for mode in R.MODES:
            out = _ops.guided_upsample(pd, lod, hid, r, eps, mode)
            again = _ops.guided_upsample(pd, lod, hid, r, eps, mode)
            torch.cuda.synchronize()
            assert tuple(out.shape) == hi + (3,)
            assert torch.equal(out.view(torch.int32), again.view(torch.int32))   # the same bits on every run
            got = out.cpu().numpy().astype(np.float64)
            want = R.upsample(p, I_lo, I_hi, r, eps, mode, ref=ref)
            e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, eps, mode, ref)
            err = np.abs(got - want)
            print(f"{lo} -> {hi}, r {r}, eps {eps}, {mode}: largest error {err.max():.3e} = "
                  f"{float((err / (e_round + e_stat)).max()):.3f} of its bound; max E_round {e_round.max():.3e}, "
                  f"max E_stat {e_stat.max():.3e}")
            assert np.isfinite(got).all()
            assert (err <= e_round + e_stat).all()
            assert e_stat.max() <= e_round.max()


@pytest.mark.parametrize("mode", R.MODES)
def test_more_tiles_than_the_largest_grid(mode):
    """16 x 16 -> 2099 x 2101: 4307 tiles against a grid of at most 2^12 workgroups, so that the first workgroups walk to a
    second tile.  The restatement is taken on the first rows, the rows around the 4096th tile's start and the last rows;
    the whole output is finite and the same on a second call."""
    from nn import _ops
    (h, w), (H, W), r, eps = (16, 16), (2099, 2101), 4, 1e-2
    assert -(-H * W // TILE) > MAX_GRID
    p, I_lo = R.S.test_images(h, w, 11)
    I_hi = np.random.default_rng(12).random((H, W, 3)).astype(np.float32)
    pd, lod, hid = _dev(p), _dev(I_lo), _dev(I_hi)
    out = _ops.guided_upsample(pd, lod, hid, r, eps, mode)
    again = _ops.guided_upsample(pd, lod, hid, r, eps, mode)
    torch.cuda.synchronize()
    assert torch.equal(out.view(torch.int32), again.view(torch.int32)) and bool(torch.isfinite(out).all())
    first_walked = MAX_GRID * TILE // W                                   # the row in which tile 4096 starts
    rows = np.r_[0:6, first_walked - 3:first_walked + 4, H - 6:H]
    assert 0 <= rows.min() and rows.max() < H and first_walked + 4 < H - 6
    got = out[torch.as_tensor(rows, device=DEV)].cpu().numpy().astype(np.float64)
    ref = R.coefficients(p, I_lo, r, eps)
    want = R.upsample(p, I_lo, I_hi, r, eps, mode, ref=ref, rows=rows)
    e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, eps, mode, ref, rows=rows)
    err = np.abs(got - want)
    print(f"{h} x {w} -> {H} x {W}, r {r}, eps {eps}, {mode}: largest error {float((err / (e_round + e_stat)).max()):.3f} "
          f"of its bound on {len(rows)} rows; max E_round {e_round.max():.3e}, max E_stat {e_stat.max():.3e}")
    assert (err <= e_round + e_stat).all()
    assert e_stat.max() <= e_round.max()


@pytest.mark.parametrize("lo,hi", [((12, 16), (48, 64)), ((42, 63), (257, 300)), ((5, 41), (25, 41))])
def test_the_kernels_up_is_resize_bilinear_bit_for_bit(lo, hi):
    """With a guide_hi of zeros every fma of the pixel returns its addend, so `guided` returns up(bbar) itself: at equal
    sizes (every weight 0) that is the plane bbar, at (H, W) it must be strotss_resize_bilinear of that plane, bit for bit
    (the taps, the order of the two lerps and the arithmetic of a lerp are the resize kernel's)."""
    from nn import _ops
    p, I_lo = R.S.test_images(*lo, 21)
    pd, lod = _dev(p), _dev(I_lo)
    for r, eps in ((1, 1e-4), (4, 1e-2)):
        bbar = _ops.guided_upsample(pd, lod, torch.zeros(*lo, 3, device=DEV), r, eps, "guided")
        got = _ops.guided_upsample(pd, lod, torch.zeros(*hi, 3, device=DEV), r, eps, "guided")
        want = _ops.resize_bilinear(bbar, *hi)
        torch.cuda.synchronize()
        assert bool((bbar != 0).any())
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))


@pytest.mark.parametrize("hw", [(5, 7), (42, 63), (257, 300), (1, 1)])
def test_guided_at_equal_sizes_is_guided_smooth_bit_for_bit(hw):
    """every interpolation weight is 0: the existing kernel is the yardstick.  residual returns p up to the rounding of
    q + (p - q): |out - p| <= u (|p - q| + |p|) and a little (the two roundings, in float32)"""
    from nn import _ops
    p, I = R.S.test_images(*hw, 5)
    pd, Id = _dev(p), _dev(I)
    for r, eps in ((1, 1e-4), (4, 1e-2), (64, 1e-4)):
        want = _ops.guided_smooth(pd, Id, r, eps)
        got = _ops.guided_upsample(pd, Id, Id.clone(), r, eps, "guided")
        back = _ops.guided_upsample(pd, Id, Id.clone(), r, eps, "residual")
        torch.cuda.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
        p64, q64 = p.astype(np.float64), want.cpu().numpy().astype(np.float64)
        assert (np.abs(back.cpu().numpy().astype(np.float64) - p64) <= U24 * (np.abs(p64 - q64) + np.abs(p64)) * (1 + 1e-6)).all()


def test_a_side_stream_gives_the_same_bits():
    from nn import _ops
    p, I_lo, I_hi = R.test_images(42, 63, 257, 300, 6)
    pd, lod, hid = _dev(p), _dev(I_lo), _dev(I_hi)
    for mode in R.MODES:
        want = _ops.guided_upsample(pd, lod, hid, 4, 1e-2, mode)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            got = _ops.guided_upsample(pd, lod, hid, 4, 1e-2, mode)
        side.synchronize()
        assert torch.equal(got.view(torch.int32), want.view(torch.int32))
    assert torch.equal(hid.cpu(), torch.from_numpy(I_hi)) and torch.equal(pd.cpu(), torch.from_numpy(p))    # inputs only read


def test_entry_refuses_bad_arguments_before_any_launch():
    """on real device buffers: every refusal returns its code and leaves `out` and the workspace untouched"""
    from nn import _hip
    from nn._ops import ptr
    lib = _hip.lib()
    h, w, H, W = 8, 8, 16, 24

    def roomy(t):
        """t with 16 spare bytes behind it: the misaligned pointers below (4 bytes on) then span their own allocation only,
        wherever the allocator puts the others -- a span reaching into a neighbour is refused as an overlap, not as misaligned"""
        flat = torch.empty(t.numel() + 4, dtype=t.dtype, device=DEV)
        flat[:t.numel()] = t.flatten()
        return flat[:t.numel()].view(t.shape)
    img, lo, hi = roomy(torch.rand(h, w, 3, device=DEV)), roomy(torch.rand(h, w, 3, device=DEV)), roomy(torch.rand(H, W, 3, device=DEV))
    out = roomy(torch.full((H, W, 3), 7.0, device=DEV))
    nbytes = int(lib.strotss_guided_upsample_workspace_bytes(h, w, 4))
    assert nbytes == 280 * h * w
    work = torch.full((nbytes + 16,), 5, dtype=torch.uint8, device=DEV)
    big = 26755
    odd = lambda t: C.c_void_p(t.data_ptr() + 4)
    call = lambda i=ptr(img), g=ptr(lo), hh=h, ww=w, G=ptr(hi), HH=H, WW=W, r=4, eps=1e-2, m=1, o=ptr(out), ws=ptr(work), \
        nb=nbytes: lib.strotss_guided_upsample(i, g, hh, ww, G, HH, WW, r, eps, m, o, ws, nb, None)
    for kwargs in (dict(i=None), dict(g=None), dict(G=None), dict(o=None), dict(ws=None), dict(hh=0), dict(ww=-1), dict(HH=0),
                   dict(WW=-2), dict(HH=7), dict(WW=7), dict(HH=big, WW=big), dict(r=0), dict(r=65), dict(r=-2),
                   dict(eps=float("nan")), dict(eps=float("inf")), dict(eps=0.0), dict(eps=0.99e-4), dict(eps=1.0001),
                   dict(eps=-1e-2), dict(m=2), dict(m=-1), dict(nb=nbytes - 1), dict(nb=0), dict(o=ptr(hi)), dict(o=ptr(lo)),
                   dict(o=ptr(img)), dict(o=C.c_void_p(hi.data_ptr() + 16))):
        assert call(**kwargs) == EINVAL, kwargs
    for kwargs in (dict(i=odd(img)), dict(g=odd(lo)), dict(G=odd(hi)), dict(o=odd(out)), dict(ws=odd(work))):
        assert call(**kwargs) == EALIGN, kwargs
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((work == 5).all())
    assert call() == 0 and call(m=0) == 0 and call(eps=1e-4) == 0 and call(eps=1.0) == 0 and call(r=64) == 0 and call(r=1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).any())


def test_operator_surface():
    from nn import strotss_utils as U
    p, I_lo, I_hi = R.test_images(42, 63, 100, 130, 9)
    for mode in U.UPSAMPLE_MODES:
        out = U.guided_upsample(_dev(p)[None], _dev(I_lo), _dev(I_hi)[None], mode=mode)      # radius None: 1 at 42 x 63
        assert tuple(out.shape) == (1, 100, 130, 3)
        r, eps = U.default_smooth_radius(42, 63), U.default_upsample_eps(mode)
        e_round, e_stat = R.error_budgets(p, I_lo, I_hi, r, eps, mode)
        assert (np.abs(out[0].cpu().numpy() - R.upsample(p, I_lo, I_hi, r, eps, mode)) <= e_round + e_stat).all()
    assert tuple(U.guided_upsample(_dev(p), _dev(I_lo), _dev(I_hi)).shape) == (100, 130, 3)
    with pytest.raises(ValueError):
        U.guided_upsample(_dev(p), _dev(I_lo), _dev(I_hi[:30]))
    with pytest.raises(ValueError):
        U.guided_upsample(_dev(p), _dev(I_lo), _dev(I_hi), mode="bicubic")


# ------------------------------------------------------------------ 2. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def _block_mean_to(img, h, w):
    """an (H, W, 3) image averaged over the H / h x W / w cells of an (h, w) grid (area downsample, any ratio)"""
    H, W = img.shape[:2]
    ys, xs = (np.arange(H) * h) // H, (np.arange(W) * w) // W
    acc, cnt = np.zeros((h, w, 3)), np.zeros((h, w, 1))
    np.add.at(acc, (ys[:, None], xs[None, :]), img)
    np.add.at(cnt, (ys[:, None], xs[None, :]), 1.0)
    return acc / cnt


def test_cli_output_size_full_single_image(tmp_path, monkeypatch):
    """the JPEG has the content file's size; downsampled to the result's size it lies nearer (mean absolute difference) to the
    run without the flag than a constant image does -- an ordering, not a threshold.  Without the flag: the same bytes from a
    namespace without the attributes and from one with output_size=None."""
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs = {}
    for name, extra in (("plain", []), ("full", ["--output_size", "full"]),
                        ("guided", ["--output_size", "full", "--upsample_mode", "guided"])):
        outs[name] = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", outs[name]] + SETTINGS + extra))
    content = _read(CONTENT)
    imgs = {k: _read(v) for k, v in outs.items()}
    assert imgs["full"].shape == content.shape == imgs["guided"].shape and imgs["plain"].shape != content.shape
    h, w = imgs["plain"].shape[:2]
    for name in ("full", "guided"):
        near = float(np.abs(_block_mean_to(imgs[name], h, w) - imgs["plain"]).mean())
        const = float(np.abs(imgs["plain"].mean((0, 1)) - imgs["plain"]).mean())
        print(f"{name}: {content.shape[:2]} written; downsampled to {h} x {w}: mean |.- plain| {near:.5f}, the plain "
              f"result's own mean colour {const:.5f}")
        assert near < const
    ns = RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "bare.jpg")] + SETTINGS)
    assert ns.output_size is None
    for name in ("output_size", "upsample_mode", "upsample_radius", "upsample_eps"):
        delattr(ns, name)
    RS.run(ns)
    assert open(tmp_path / "bare.jpg", "rb").read() == open(outs["plain"], "rb").read()


def test_cli_output_size_with_luminance(tmp_path, monkeypatch):
    """--output_size full --preserve_color luminance: the float image handed to postprocess has the full-size content's
    chroma within the merge's bound of section 15 (16 * 2^-24) and the luma of the upsampled result"""
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    seen = {}
    upsample, post = RS.strotss.guided_upsample, RS.strotss.postprocess

    def up_spy(*a, **k):
        seen["upsampled"] = upsample(*a, **k)
        return seen["upsampled"]

    def post_spy(final):
        seen["written"] = final.detach().clone()
        return post(final)

    monkeypatch.setattr(RS.strotss, "guided_upsample", up_spy)
    monkeypatch.setattr(RS.strotss, "postprocess", post_spy)
    RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "both.jpg"), "--output_size", "full",
                                         "--preserve_color", "luminance"] + SETTINGS))
    c = RS.utils.load_image(CONTENT)[0].cpu().numpy().astype(np.float64)
    f = lambda t: t.reshape(c.shape).cpu().numpy().astype(np.float64)
    upsampled, written = f(seen["upsampled"]), f(seen["written"])
    assert _read(str(tmp_path / "both.jpg")).shape == c.shape
    assert float(np.abs(CR.luma64(written) - CR.luma64(upsampled)).max()) <= 16 * U24
    assert CR.chroma_distance(written, c) <= 16 * U24 < CR.chroma_distance(upsampled, c)


def test_cli_output_size_video(tmp_path, monkeypatch):
    """three 96 x 128 frames, results at 48 x 64: full-size frames are written, and the flows (computed on the content at
    the results' size) are byte for byte those of the run without the flag"""
    import run_strotss as RS
    from PIL import Image
    from test_hip_color import _moved_frames, _texture
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames, h=96, w=128)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    outs, flows = {}, {}
    for name, extra in (("plain", []), ("full", ["--output_size", "full"])):
        outs[name], flows[name] = tmp_path / name, tmp_path / (name + "_flow")
        RS.run(RS.build_parser().parse_args([frames, style, "--video", "--compute_flow", "--save_flow", str(flows[name]),
                                             "-o", str(outs[name])] + SETTINGS + extra))
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    for s in stems:
        assert _read(str(outs["plain"] / f"{s}.jpg")).shape == (48, 64, 3)
        assert _read(str(outs["full"] / f"{s}.jpg")).shape == (96, 128, 3)
    names = sorted(os.listdir(flows["plain"]))
    assert len(names) == 4 and names == sorted(os.listdir(flows["full"]))
    for n in names:
        assert open(flows["plain"] / n, "rb").read() == open(flows["full"] / n, "rb").read(), n


def test_cli_refuses_a_target_smaller_than_the_result_before_the_first_step(tmp_path, monkeypatch):
    import run_strotss as RS
    stepped = []
    monkeypatch.setattr(RS, "_stylise", lambda *a, **k: stepped.append(1))
    with pytest.raises(ValueError, match="smaller than the result"):
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "o.jpg"), "--max_size", "128", "--level",
                                             "2", "--max_iter", "30", "--output_size", "64"]))
    assert not stepped and not os.path.exists(tmp_path / "o.jpg")
