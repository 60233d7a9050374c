"""Scribble masks on the MI355X: strotss_scribble_labels in its plain and blocked forms bit for bit
against each other and element by element against the float64 restatement (tests/_scribble_ref.py) on the seeded cases of
tests/_scribble_cases.py (tests/test_scribble_cpu.py asserts their yardstick Y and their margins), strotss_kmeans_scores
against strotss_kmeans_assign and float64, two degenerate inputs, scribble_masks on the golden pair and the scribble flags
through the command line."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as CR  # noqa: E402
import _scribble_cases as S  # noqa: E402
import _scribble_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
CASES = [(h, w, k) for (h, w) in S.SHAPES for k in S.KS]
BOUND_FACTOR = 4.0                                           # |x_hip - x_f64ref| <= 4 Y: the factor of the flow tests


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _call(img, stroke, scores, iters, per=0, **kw):
    from nn import _ops
    label, count, x = _ops.scribble_labels(img, stroke, scores, kw.get("tau", R.TAU), kw.get("lam", R.LAMBDA),
                                           kw.get("sigma", R.SIGMA), iters, per, planes=True)
    return label, count, x


def _same_bits(a, b):
    return all(torch.equal(u.view(torch.int32), v.view(torch.int32)) for u, v in zip(a, b))


# ------------------------------------------------------------------ 1. the two forms, and float64
@pytest.mark.parametrize("case", CASES, ids=lambda c: "%dx%d-k%d" % c)
def test_blocked_equals_plain_and_both_match_float64(case):
    h, w, k = case
    img, stroke, scores = (_dev(a, t) for a, t in zip(S.make(h, w, k), (torch.float32, torch.int32, torch.float32)))
    ref = S.run(h, w, k)
    for n in S.sweeps_of((h, w)):
        plain = _call(img, stroke, scores, n, 1)
        for per in (0, 2, 4, 8):
            assert _same_bits(plain, _call(img, stroke, scores, n, per)), f"{n} sweeps, {per} per launch"
        label, count, x = (t.cpu().numpy() for t in plain)
        Y = S.yardstick(h, w, k, n)
        err = np.abs(x.astype(np.float64) - ref[n]["x"])
        at = np.unravel_index(int(err.argmax()), err.shape)
        print(f"{h} x {w}, k {k}, {n} sweeps: worst |x - ref| {err.max():.2e} = {err.max() / Y:.2f} Y at plane {at[0]}, "
              f"pixel ({at[1]}, {at[2]})")
        assert (err <= BOUND_FACTOR * Y).all()
        assert x.min() >= 0 and x.max() <= 1
        wide = ref[n]["margin"] >= S.MARGIN_FACTOR * Y
        assert label.dtype == np.int32 and np.array_equal(label[wide], ref[n]["label"][wide])
        assert np.array_equal(count, np.bincount(label.reshape(-1), minlength=k))
        fixed = ref["fixed"]
        assert np.array_equal(x[:, fixed], (np.arange(k)[:, None] == S.make(h, w, k)[1][fixed][None]).astype(np.float32))


def test_two_streams_give_the_same_bits():
    h, w, k = 97, 130, 7
    img, stroke, scores = (_dev(a, t) for a, t in zip(S.make(h, w, k), (torch.float32, torch.int32, torch.float32)))
    for per in (1, 8):
        first = _call(img, stroke, scores, 24, per)
        first = tuple(t.clone() for t in first)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            aside = _call(img, stroke, scores, 24, per)
        side.synchronize()
        assert _same_bits(first, aside)


def test_a_very_tall_image_has_more_tile_rows_than_one_grid_axis_holds():
    """65537 rows of 32-row tiles: the blocked form numbers its tiles in grid.x, whose limit is 2^31 - 1, not in grid.y
    (65535); the forms agree bit for bit there too, and the strokes reach two pixels along the column in two sweeps"""
    h, w, k = 65536 * 32 + 1, 1, 2
    img = torch.full((h, w, 3), 0.5, device=DEV)                       # every weight is 1
    scores = _dev(np.full((4, 1, k), 0.25, dtype=np.float32))
    stroke = np.full((h, w), -1, dtype=np.int32)
    stroke[0, 0], stroke[h - 1, 0], stroke[h // 2, 0] = 0, 1, 1
    stroke = _dev(stroke, torch.int32)
    plain = _call(img, stroke, scores, 2, 1)
    for per in (0, 2):
        assert _same_bits(plain, _call(img, stroke, scores, 2, per))
    label, count, x = plain
    assert int(count.sum()) == h and label[0, 0] == 0 and label[h - 1, 0] == 1 and label[h // 2, 0] == 1
    moved = (x[0, :, 0] != 0.5).nonzero().reshape(-1).cpu().numpy()
    assert set(moved.tolist()) == set(range(0, 3)) | set(range(h - 3, h)) | set(range(h // 2 - 2, h // 2 + 3))


# ------------------------------------------------------------------ 2. degenerate inputs
@pytest.mark.parametrize("k", S.KS)
def test_constant_image_with_uniform_scores_stays_at_one_kth(k):
    """every weight is 1; after one sweep x is exactly 1 / k on the rows that no stroke neighbours"""
    h, w = 40, 70
    img = torch.full((h, w, 3), 0.5, device=DEV)
    scores = torch.full((5, 9, k), 0.25, device=DEV)
    stroke = np.full((h, w), -1, dtype=np.int32)
    stroke[20, 10:30] = 0
    stroke[20, 40:60] = k - 1
    label, count, x = _call(img, _dev(stroke, torch.int32), scores, 1, 1)
    blocked = _call(img, _dev(stroke, torch.int32), scores, 1, 8)       # one sweep: runs in the plain form
    assert _same_bits((label, count, x), blocked)
    x = x.cpu().numpy()
    away = np.ones(h, dtype=bool)
    away[19:22] = False
    assert (x[:, away] == np.float32(1.0 / k)).all()
    assert (x[0, 19, 10:30] > np.float32(1.0 / k)).all() and (x[k - 1, 21, 40:60] > np.float32(1.0 / k)).all()
    _, _, x8 = _call(img, _dev(stroke, torch.int32), scores, 8, 8)
    x8 = x8.cpu().numpy()
    far = np.ones(h, dtype=bool)
    far[20 - 9:20 + 10] = False                                        # 8 sweeps carry a stroke 8 rows
    assert (x8[:, far] == np.float32(1.0 / k)).all()


@pytest.mark.parametrize("iters,per", [(1, 1), (5, 2), (16, 8)])
def test_strokes_on_every_pixel_are_the_labels(iters, per):
    h, w, k = 45, 65, 3
    img, _, scores = S.make(h, w, k)
    stroke = np.random.default_rng(3).integers(0, k, size=(h, w)).astype(np.int32)
    label, count, x = _call(_dev(img), _dev(stroke, torch.int32), _dev(scores), iters, per)
    assert np.array_equal(label.cpu().numpy(), stroke)
    assert np.array_equal(count.cpu().numpy(), np.bincount(stroke.reshape(-1), minlength=k))
    assert np.array_equal(x.cpu().numpy(), (np.arange(k)[:, None, None] == stroke[None]).astype(np.float32))


# ------------------------------------------------------------------ 3. the scores
@pytest.mark.parametrize("shape", [(1, 3, 1), (33, 35, 2), (1000, 35, 16), (4096, 2179, 7)])
def test_kmeans_scores_are_the_scores_of_the_assignment(shape):
    from nn import _ops
    n, d, k = shape
    x, _ = CR.planted_rows(n, d, k, 1.0, 2000 + n % 997 + d + k)
    inv = CR.inv_norm(x, n)
    centres, _ = CR.farthest_first(x, inv, n, d, k)
    c32 = np.zeros((k, x.shape[1]), dtype=np.float32)
    c32[:, :d] = centres
    if n >= 3:
        x[1] = 0.0
        inv[1] = CR.inv_norm(x, n)[1]
        inv[2] = 0.0
    xd, invd, cd = _dev(x), _dev(inv), _dev(c32)
    s = _ops.kmeans_scores(xd, invd, n, d, cd, k)
    again = _ops.kmeans_scores(xd, invd, n, d, cd, k)
    label, best, second = _ops.kmeans_assign(xd, invd, n, d, cd, k)
    assert tuple(s.shape) == (n, k) and torch.equal(s.view(torch.int32), again.view(torch.int32))
    top = torch.sort(s, dim=1, descending=True).values
    assert torch.equal(top[:, 0].contiguous().view(torch.int32), best.view(torch.int32))
    if k > 1:
        assert torch.equal(top[:, 1].contiguous().view(torch.int32), second.view(torch.int32))
    assert torch.equal(s.gather(1, label.long()[:, None])[:, 0].view(torch.int32), best.view(torch.int32))
    ref = CR.scores(x, inv, n, d, c32)
    err = np.abs(s.cpu().numpy().astype(np.float64) - ref).max()
    print(f"scores n {n} d {d} k {k}: largest |s - ref| {err:.2e}, allowed {CR.assign_bound(d):.2e}")
    assert err <= CR.assign_bound(d)
    if n >= 3:
        assert not s[2].any()                                          # inverse norm 0: k zeros


# ------------------------------------------------------------------ 4. scribble_masks on the golden pair
def _bars(h, w):
    """two-colour strokes: a 3-pixel bar in opposite corners -- region 0 top left, region 1 bottom right"""
    strokes = np.full((h, w), -1, dtype=np.int32)
    strokes[2:5, 2:w // 3] = 0
    strokes[h - 5:h - 2, w - w // 3:w - 2] = 1
    return strokes


@pytest.fixture(scope="module")
def golden_pair():
    from nn import utils
    from nn.model import VGG
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    return vgg.params, utils.load_image(CONTENT, max_size=64), utils.load_image(STYLE, max_size=64)


def test_scribble_masks_on_the_golden_pair(golden_pair):
    from nn import strotss_utils as U
    params, content, style = golden_pair
    strokes = [_bars(int(im.shape[1]), int(im.shape[2])) for im in (content, style)]
    masks = U.scribble_masks(params, content, style, strokes[0], strokes[1], 2)
    again = U.scribble_masks(params, content, style, strokes[0], strokes[1], 2)
    found = U.scribble_regions(params, content, style, strokes[0], strokes[1], 2, planes=True)
    print(f"golden pair at 64 px, two strokes per image: pixels per region (content, style) {found['counts'].tolist()}")
    for i, image in enumerate((content, style)):
        H, W = int(image.shape[1]), int(image.shape[2])
        m = masks[i]
        assert len(m) == 2 and all(tuple(t.shape) == (H, W, 1) and t.dtype == torch.float32 for t in m)
        assert bool(((torch.stack(m) == 0) | (torch.stack(m) == 1)).all()) and bool((torch.stack(m).sum(dim=0) == 1).all())
        assert all(torch.equal(a, b) for a, b in zip(m, again[i]))
        on = strokes[i] >= 0
        for r in range(2):
            assert (m[r].cpu().numpy()[..., 0][strokes[i] == r] == 1).all()
        assert np.array_equal(found["strokes"][i].cpu().numpy(), strokes[i])
        label = found["labels"][i].cpu().numpy()
        assert all(np.array_equal(m[r].cpu().numpy()[..., 0] == 1, label == r) for r in range(2))
        assert np.array_equal(found["counts"][i], np.bincount(label.reshape(-1), minlength=2))
        # the restatement fed with the device's scores: the same labels outside the margin band, x within the bound
        ref = R.diffuse(image[0].cpu().numpy(), strokes[i], found["grid_scores"][i].cpu().numpy())
        ref32 = R.diffuse(image[0].cpu().numpy(), strokes[i], found["grid_scores"][i].cpu().numpy(), dtype=np.float32)
        Y = float(np.abs(ref32[R.ITERS]["x"].astype(np.float64) - ref[R.ITERS]["x"]).max())
        err = float(np.abs(found["x"][i].cpu().numpy().astype(np.float64) - ref[R.ITERS]["x"]).max())
        wide = ref[R.ITERS]["margin"] >= S.MARGIN_FACTOR * Y
        print(f"image {i}: Y {Y:.2e}, worst |x - ref| {err:.2e}, {int((~wide).sum())} pixels inside the margin band, "
              f"{int(on.sum())} stroke pixels")
        assert 0 < Y < S.Y_CAP and err <= BOUND_FACTOR * Y
        assert np.array_equal(label[wide], ref[R.ITERS]["label"][wide])
    # the seeds are the restatement's, and the centres one update over them
    n_c = found["n_c"]
    seeds = np.concatenate([s.reshape(-1) for s in found["seeds"]])
    assert seeds.size == n_c + found["n_s"] and set(np.unique(seeds)) == {-1, 0, 1}
    rows, inv = found["rows"].cpu().numpy(), found["inv_norm"].cpu().numpy()
    centres, _ = CR.update(rows, inv, seeds, seeds.size, found["d"], 2, np.zeros((2, found["d"])))
    assert np.abs(found["centres"].cpu().numpy()[:, :found["d"]] - centres).max() <= 2.0 ** -23


def test_scribble_regions_names_a_stroke_that_is_too_thin(golden_pair):
    from nn import strotss_utils as U
    params, content, style = golden_pair
    strokes = [_bars(int(im.shape[1]), int(im.shape[2])) for im in (content, style)]
    with pytest.raises(ValueError, match="too thin"):
        U.scribble_regions(params, content, style, strokes[0], strokes[1], 3)           # region 2 has no stroke at all
    strokes[1][:] = 0                                                                   # region 1 takes none of the style
    strokes[1][0, 0] = 1
    with pytest.raises(ValueError, match=r"colour \(255, 0, 0\)"):
        U.scribble_masks(params, content, style, strokes[0], strokes[1], 2, colours=[(0, 0, 255), (255, 0, 0)])


# ------------------------------------------------------------------ 5. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_scribbles(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    palette = np.array(R.CORNER_COLOURS, dtype=np.uint8)
    files = []
    for name, path in (("c.png", CONTENT), ("s.png", STYLE)):
        with Image.open(path) as im:
            wide, high = im.size
        factor = max(high / 64, wide / 64)                             # the size the image is loaded at (nn.utils.resize)
        strokes = _bars(int(high / factor), int(wide / factor))
        strokes = strokes.repeat(2, axis=0).repeat(2, axis=1)          # twice that size: brought back by nearest neighbour
        Image.fromarray(palette[np.where(strokes < 0, 0, strokes * 3 + 1)], "RGB").save(tmp_path / name)      # blue, red
        files.append(str(tmp_path / name))
    seen = {}
    grow = RS.strotss.scribble_masks

    def spy(*a, **k):
        seen["masks"] = grow(*a, **k)
        return seen["masks"]

    monkeypatch.setattr(RS.strotss, "scribble_masks", spy)
    out = {name: str(tmp_path / f"{name}.jpg") for name in ("plain", "scribbles", "given", "bare")}
    parse = lambda name, extra: RS.build_parser().parse_args([CONTENT, STYLE, "-o", out[name]] + SETTINGS + extra)
    RS.run(parse("plain", []))
    RS.run(parse("scribbles", ["--content_scribbles", files[0], "--style_scribbles", files[1], "--save_masks",
                               str(tmp_path / "masks")]))
    c_masks, s_masks = seen["masks"]
    assert len(c_masks) == len(s_masks) == 2 and _bytes(out["scribbles"]) != _bytes(out["plain"])
    # the same run with the masks handed in where painted masks come from: the same bytes
    monkeypatch.setattr(RS, "_load_masks", lambda args: (c_masks, s_masks))
    RS.run(parse("given", []))
    monkeypatch.undo()
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    assert _bytes(out["given"]) == _bytes(out["scribbles"])
    # --save_masks: two PNGs of the images' sizes in the corner colours, the same partition
    for name, masks in (("content_mask.png", c_masks), ("style_mask.png", s_masks)):
        img = np.asarray(Image.open(tmp_path / "masks" / name).convert("RGB"))
        assert img.shape == tuple(masks[0].shape[:2]) + (3,) and np.isin(img, (0, 255)).all()
        region = (img[..., 0] // 255) * 4 + (img[..., 1] // 255) * 2 + img[..., 2] // 255
        for r, m in enumerate(masks):
            assert np.array_equal(region == r, m.cpu().numpy()[..., 0] == 1)
    # without the flags nothing changes: a namespace without the attributes writes the plain run's bytes
    ns = parse("bare", [])
    for name in ("content_scribbles", "style_scribbles", "scribble_sigma", "scribble_iters"):
        assert getattr(ns, name) is None
        delattr(ns, name)
    RS.run(ns)
    assert _bytes(out["bare"]) == _bytes(out["plain"])
