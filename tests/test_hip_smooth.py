"""Photo smoothing on the MI355X: strotss_guided_smooth element by element against the float64
restatement (tests/_smooth_ref.py) within E_round + E_stat at the step shapes and the corner sizes, bit-for-bit repeatability,
in place, a side stream, the refusals of the entry on real buffers, and --photo_smooth through the command line (single
image, --video --compute_flow, with --preserve_color luminance)."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _color_ref as CR  # noqa: E402
import _smooth_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
SHAPES = [(48, 64), (42, 63), (257, 300), (768, 1024), (1, 1), (1, 3), (5, 200)]
RADII = [1, 4, 16, 64]
EPSILONS = [1e-2, 1e-4]
U24 = 2.0 ** -24
EINVAL, EALIGN = -1, -2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------ 1. the kernels
@pytest.mark.parametrize("r", RADII)
@pytest.mark.parametrize("hw", SHAPES)
def test_guided_smooth_matches_float64(hw, r):
    """|q - q_ref| <= E_round + E_stat per element (tests/_smooth_ref.py: error_budgets; derivations in DESIGN.md section
    16), and the statistics condition max E_stat <= max E_round, at both eps."""
    from nn import _ops
    h, w = hw
    p, I = R.test_images(h, w, 1000 * r + h + w)
    pd, Id = _dev(p), _dev(I)
    for eps in EPSILONS:
        out = _ops.guided_smooth(pd, Id, r, eps)
        again = _ops.guided_smooth(pd, Id, r, eps)
        torch.cuda.synchronize()
        assert torch.equal(out.view(torch.int32), again.view(torch.int32))       # the same bits on every run
        got = out.cpu().numpy().astype(np.float64)
        ref = R.guided_separable(p, I, r, eps, full=True)
        e_round, e_stat = R.error_budgets(p, I, r, eps, ref)
        err = np.abs(got - ref["q"])
        print(f"{h} x {w}, r {r}, eps {eps}: largest error {err.max():.3e} = {float((err / (e_round + e_stat)).max()):.3f} of "
              f"its bound; max E_round {e_round.max():.3e}, max E_stat {e_stat.max():.3e}")
        assert np.isfinite(got).all()
        assert (err <= e_round + e_stat).all()
        assert e_stat.max() <= e_round.max()


def test_more_tiles_than_the_largest_grid():
    """a one-pixel-wide image of 2^16 + 37 rows: 2^14 + 10 tiles in the column passes and 2^16 + 37 in the row passes, against
    grids of at most 2^14 workgroups, so that workgroups walk several tiles and the last tiles come from a second walk"""
    from nn import _ops
    h, w, r, eps = 2 ** 16 + 37, 1, 4, 1e-2
    p, I = R.test_images(h, w, 11)
    got = _ops.guided_smooth(_dev(p), _dev(I), r, eps).cpu().numpy().astype(np.float64)
    ref = R.guided_separable(p, I, r, eps, full=True)
    e_round, e_stat = R.error_budgets(p, I, r, eps, ref)
    err = np.abs(got - ref["q"])
    print(f"{h} x {w}, r {r}, eps {eps}: largest error {float((err / (e_round + e_stat)).max()):.3f} of its bound")
    assert np.isfinite(got).all()
    assert (err <= e_round + e_stat).all()


@pytest.mark.parametrize("hw", [(42, 63), (257, 300), (1, 3)])
def test_in_place_is_out_of_place_bit_for_bit(hw):
    from nn import _ops
    h, w = hw
    p, I = R.test_images(h, w, 5)
    pd, Id = _dev(p), _dev(I)
    for r, eps in ((1, 1e-4), (16, 1e-2), (64, 1e-4)):
        out = _ops.guided_smooth(pd, Id, r, eps)
        inplace = pd.clone()
        assert _ops.guided_smooth(inplace, Id, r, eps, out=inplace) is inplace
        torch.cuda.synchronize()
        assert torch.equal(inplace.view(torch.int32), out.view(torch.int32))
        assert torch.equal(Id.cpu(), torch.from_numpy(I))                        # the guide is only read


def test_a_side_stream_gives_the_same_bits():
    from nn import _ops
    p, I = R.test_images(257, 300, 6)
    pd, Id = _dev(p), _dev(I)
    want = _ops.guided_smooth(pd, Id, 16, 1e-2)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        got = _ops.guided_smooth(pd, Id, 16, 1e-2)
    side.synchronize()
    assert torch.equal(got.view(torch.int32), want.view(torch.int32))


def test_constant_guide_and_self_guidance():
    """the identities of the CPU tests, on the kernels: a constant guide gives the twice box-averaged image (a == 0, so only
    the storage of b and the rounding of its mean are inexact, fma(0, I, b) is b: two roundings of boxmean |b|), and 1 x 1
    returns the image"""
    from nn import _ops
    rng = np.random.default_rng(8)
    p = rng.random((42, 63, 3)).astype(np.float32)
    I = np.full((42, 63, 3), 0.5, dtype=np.float32)
    got = _ops.guided_smooth(_dev(p), _dev(I), 4, 1e-2).cpu().numpy()
    want = R.box_mean_twice(p, 4)
    assert (np.abs(got - want) <= R.gamma32(2) * np.abs(want) + 1e-12).all()
    one = rng.random((1, 1, 3)).astype(np.float32)
    assert np.array_equal(_ops.guided_smooth(_dev(one), _dev(one), 64, 1e-4).cpu().numpy(), one)


def test_entry_refuses_bad_arguments_before_any_launch():
    """on real device buffers: every refusal returns its code and leaves `out` untouched"""
    from nn import _hip
    from nn._ops import ptr
    lib = _hip.lib()
    h, w = 8, 8
    img, guide = torch.rand(h, w, 3, device=DEV), torch.rand(h, w, 3, device=DEV)
    out = torch.full((h, w, 3), 7.0, device=DEV)
    nbytes = int(lib.strotss_guided_smooth_workspace_bytes(h, w, 4))
    assert nbytes == 216 * h * w
    work = torch.empty(nbytes + 16, dtype=torch.uint8, device=DEV)
    big = 26755
    odd = lambda t: C.c_void_p(t.data_ptr() + 4)
    call = lambda i=ptr(img), g=ptr(guide), hh=h, ww=w, r=4, eps=1e-2, o=ptr(out), ws=ptr(work), nb=nbytes: \
        lib.strotss_guided_smooth(i, g, hh, ww, r, eps, o, ws, nb, None)
    for kwargs in (dict(i=None), dict(g=None), dict(o=None), dict(ws=None), dict(hh=0), dict(ww=-1),
                   dict(hh=big, ww=big, nb=2 ** 62), dict(r=0), dict(r=65), dict(r=-2), dict(eps=float("nan")),
                   dict(eps=float("inf")), dict(eps=0.0), dict(eps=0.99e-4), dict(eps=1.0001), dict(eps=-1e-2),
                   dict(nb=nbytes - 1), dict(nb=0), dict(o=ptr(guide))):
        assert call(**kwargs) == EINVAL, kwargs
    for kwargs in (dict(i=odd(img)), dict(g=odd(guide)), dict(o=odd(out)), dict(ws=odd(work))):
        assert call(**kwargs) == EALIGN, kwargs
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
    assert call() == 0 and call(eps=1e-4) == 0 and call(eps=1.0) == 0 and call(r=64) == 0 and call(r=1) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())


def test_operator_surface():
    from nn import strotss_utils as U
    p, I = R.test_images(42, 63, 9)
    out = U.guided_smooth(_dev(p)[None], _dev(I))                                # radius None: the rule, 1 at 42 x 63
    assert tuple(out.shape) == (1, 42, 63, 3)
    ref = R.guided_separable(p, I, U.default_smooth_radius(42, 63), 1e-2, full=True)
    e_round, e_stat = R.error_budgets(p, I, 1, 1e-2, ref)
    assert (np.abs(out[0].cpu().numpy() - ref["q"]) <= e_round + e_stat).all()
    with pytest.raises(ValueError):
        U.guided_smooth(_dev(p), _dev(I[:-1]))
    with pytest.raises(ValueError):
        U.guided_smooth(_dev(p), _dev(I), radius=65)
    with pytest.raises(ValueError):
        U.guided_smooth(_dev(p), _dev(I), eps=float("nan"))


# ------------------------------------------------------------------ 2. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def _content_at_output_size(RS, path):
    args = RS.build_parser().parse_args([path, STYLE] + SETTINGS)
    return RS._frame_at_result_size(RS._resolve(args), path).cpu().numpy().astype(np.float64)


def test_cli_photo_smooth_single_image(tmp_path, monkeypatch):
    """R(img) = mean |img - guided_ref(img; content)| on the written uint8 / 255: the ordering R(smooth) < R(plain) only; the
    sizes of the gaps are recorded in DESIGN.md section 16, not asserted."""
    import run_strotss as RS
    from nn import strotss_utils as U
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs = {}
    for name, extra in (("plain", []), ("smooth", ["--photo_smooth"])):
        outs[name] = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", outs[name]] + SETTINGS + extra))
    c = _content_at_output_size(RS, CONTENT)
    r, eps = U.default_smooth_radius(c.shape[0], c.shape[1]), U.DEFAULT_SMOOTH_EPS
    imgs = {k: _read(v) for k, v in outs.items()}
    assert all(im.shape == c.shape for im in imgs.values())
    res = {k: R.residual(im, c, r, eps) for k, im in imgs.items()}
    print(f"single image, golden pair at 64 px, r {r}, eps {eps}: R(plain) = {res['plain']:.5f}, "
          f"R(smooth) = {res['smooth']:.5f}")
    assert res["smooth"] < res["plain"]
    # without the flag nothing changes: a namespace without the attributes and one with photo_smooth=False, same bytes
    ns = RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "bare.jpg")] + SETTINGS)
    assert ns.photo_smooth is False
    for name in ("photo_smooth", "smooth_radius", "smooth_eps"):
        delattr(ns, name)
    RS.run(ns)
    assert open(tmp_path / "bare.jpg", "rb").read() == open(outs["plain"], "rb").read()
    assert open(outs["smooth"], "rb").read() != open(outs["plain"], "rb").read()


def test_cli_photo_smooth_with_luminance(tmp_path, monkeypatch):
    """--photo_smooth --preserve_color luminance: the float image handed to postprocess has the luma of the SMOOTHED result
    and the chroma of the content, within the merge's bound of section 15 (16 * 2^-24)."""
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    seen = {}
    smooth, post = RS.strotss.guided_smooth, RS.strotss.postprocess

    def smooth_spy(result, content, *a, **k):
        seen["unfiltered"] = result.detach().clone()
        seen["smoothed"] = smooth(result, content, *a, **k)
        return seen["smoothed"]

    def post_spy(final):
        seen["written"] = final.detach().clone()
        return post(final)

    monkeypatch.setattr(RS.strotss, "guided_smooth", smooth_spy)
    monkeypatch.setattr(RS.strotss, "postprocess", post_spy)
    RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", str(tmp_path / "both.jpg"), "--photo_smooth", "--smooth_radius",
                                         "3", "--smooth_eps", "1e-3", "--preserve_color", "luminance"] + SETTINGS))
    c = _content_at_output_size(RS, CONTENT)
    f = lambda t: t.reshape(c.shape).cpu().numpy().astype(np.float64)
    smoothed, written, unfiltered = f(seen["smoothed"]), f(seen["written"]), f(seen["unfiltered"])
    assert float(np.abs(CR.luma64(written) - CR.luma64(smoothed)).max()) <= 16 * U24
    assert CR.chroma_distance(written, c) <= 16 * U24 < CR.chroma_distance(smoothed, c)
    # and the smoothed image is the filter of the optimiser's result at the flags' radius and eps
    e_round, e_stat = R.error_budgets(unfiltered, c, 3, 1e-3)
    assert (np.abs(smoothed - R.guided_separable(unfiltered, c, 3, 1e-3)) <= e_round + e_stat).all()
    assert float(np.abs(CR.luma64(smoothed) - CR.luma64(unfiltered)).max()) > 1e-3


def test_cli_photo_smooth_video(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three synthetic frames of the colour test
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    r, eps = 2, 1e-3
    outs = {}
    for name, extra in (("plain", []), ("smooth", ["--photo_smooth", "--smooth_radius", str(r), "--smooth_eps", str(eps)])):
        outs[name] = tmp_path / name
        RS.run(RS.build_parser().parse_args([frames, style, "--video", "--compute_flow", "-o", str(outs[name])]
                                            + SETTINGS + extra))
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    for name in outs:
        assert sorted(os.listdir(outs[name])) == sorted(s + ".jpg" for s in stems)
    for p, s in zip(paths, stems):
        c = _content_at_output_size(RS, p)
        plain, smooth = (_read(outs[k] / f"{s}.jpg") for k in ("plain", "smooth"))
        r_plain, r_smooth = R.residual(plain, c, r, eps), R.residual(smooth, c, r, eps)
        print(f"{s}, r {r}, eps {eps}: R(plain) = {r_plain:.5f}, R(smooth) = {r_smooth:.5f}")
        assert r_smooth < r_plain, s
