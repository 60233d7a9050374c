"""Region clustering on the MI355X: strotss_kmeans_assign and strotss_kmeans_update row by row against
the float64 restatement (tests/_cluster_ref.py) at the shapes where the kernels can go wrong, spherical_kmeans label for label
on the planted cases (tests/test_cluster_cpu.py shows that no margin of theirs is within the float32 bound E, so equality is
exact), auto_masks on the golden pair, and --auto_masks / --save_masks through the command line."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
U23, U24 = 2.0 ** -23, 2.0 ** -24
# (n, d, k): the smallest case; a row tail and a column tail; small d, largest k; the product's width; the largest case the
# feature makes; more rows than the largest grid holds tiles for (4098 tiles of 32 rows on 2048 workgroups)
SHAPES = [(1, 3, 1), (33, 35, 2), (1000, 35, 16), (4096, 2179, 5), (8192, 2179, 16), (2 ** 17 + 37, 35, 3)]
_cases = {}


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _padded(centres, ld):
    """(k, d) float64 centres -> (k, ld) float32, zero-padded"""
    out = np.zeros((centres.shape[0], ld), dtype=np.float32)
    out[:, :centres.shape[1]] = centres
    return out


def _case(n, d, k):
    """planted rows with a zero row and a row of inverse norm 0 (n >= 3), float32 centres one update after farthest-first,
    and the float64 assignment against exactly those float32 centres; computed once"""
    if (n, d, k) not in _cases:
        x, _ = R.planted_rows(n, d, k, 1.0, 1000 + n % 997 + d + k)
        inv = R.inv_norm(x, n)
        centres, _ = R.farthest_first(x, inv, n, d, k)
        label, _, _, _ = R.assign(x, inv, n, d, centres)
        centres, _ = R.update(x, inv, label, n, d, k, centres)
        c32 = _padded(centres, x.shape[1])
        if n >= 3:
            x[1] = 0.0
            inv[1] = R.inv_norm(x, n)[1]                            # 1e6: what strotss_row_inv_norm gives a zero row
            inv[2] = 0.0
        _cases[(n, d, k)] = (x, inv, c32) + R.assign(x, inv, n, d, c32)
    return _cases[(n, d, k)]


def _check_assignment(got, ref, d, what):
    label, best, second = (t.cpu().numpy() for t in got)
    ref_label, ref_best, ref_second, s = ref
    E = R.assign_bound(d)
    n, k = s.shape
    assert label.dtype == np.int32 and ((0 <= label) & (label < k)).all()
    ok = R.admissible(label, s, E)
    wide = (ref_best - ref_second) > E
    tol = E / 2 + U23
    err_b = np.abs(best - ref_best)
    print(f"{what}: {100 * float((~wide).mean()):.2f} % of the rows within E = {E:.2e}; largest |best - ref| "
          f"{err_b.max():.2e} (allowed {tol:.2e}); {int((label != ref_label).sum())} labels differ from the reference's")
    assert ok.all()
    assert np.array_equal(label[wide], ref_label[wide])
    assert (err_b <= tol).all()
    if k == 1:
        assert np.isneginf(second).all()
    else:
        assert (np.abs(second - ref_second) <= tol).all()


# ------------------------------------------------------------------ 1. the assignment
@pytest.mark.parametrize("shape", SHAPES)
def test_assign_matches_float64(shape):
    from nn import _ops
    n, d, k = shape
    x, inv, c32, *ref = _case(n, d, k)
    xd, invd, cd = _dev(x), _dev(inv), _dev(c32)
    got = _ops.kmeans_assign(xd, invd, n, d, cd, k)
    again = _ops.kmeans_assign(xd, invd, n, d, cd, k)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        aside = _ops.kmeans_assign(xd, invd, n, d, cd, k)
    side.synchronize()
    for a, b, c in zip(got, again, aside):                           # the same bits on a second call and on a side stream
        assert torch.equal(a.view(torch.int32), b.view(torch.int32)) and torch.equal(a.view(torch.int32), c.view(torch.int32))
    _check_assignment(got, ref, d, f"assign n {n} d {d} k {k}")
    if n >= 3:
        label, best, second = (t.cpu().numpy() for t in got)
        for row in (1, 2):                                           # the zero row and the row of inverse norm 0
            assert label[row] == 0 and best[row] == 0 and second[row] == (0 if k > 1 or row == 2 else -np.inf)


@pytest.mark.parametrize("case", R.UNSTRUCTURED)
def test_assign_on_unstructured_rows(case):
    """rows with margins down to 1e-9 (at most 5 % within E: tests/test_cluster_cpu.py), at the reference's final centres"""
    from nn import _ops
    n, d, k = case[:3]
    x, _ = R.planted_rows(*case)
    inv = R.inv_norm(x, n)
    c32 = _padded(R.planted_result(case)["centres"], x.shape[1])
    got = _ops.kmeans_assign(_dev(x), _dev(inv), n, d, _dev(c32), k)
    _check_assignment(got, R.assign(x, inv, n, d, c32), d, f"unstructured n {n} d {d} k {k}")


def test_assign_breaks_ties_toward_the_lowest_centre():
    from nn import _ops
    x = np.zeros((32, 32), dtype=np.float32)
    x[:5, :3] = [0.25, 0.5, 0.125]
    c = np.zeros((4, 32), dtype=np.float32)
    c[:, :3] = [[0, 0, 1], [0, 1, 0], [0, 1, 0], [0, 0, 1]]       # exact products: centres 1 and 2 tie at the top
    inv = np.ones(32, dtype=np.float32)
    label, best, second = _ops.kmeans_assign(_dev(x), _dev(inv), 5, 3, _dev(c), 4)
    assert label.tolist() == [1] * 5 and best.tolist() == [0.5] * 5 and second.tolist() == [0.5] * 5


def test_argmax_and_argmin_take_the_lowest_index_on_the_device():
    """the tie rule of the farthest-first initialisation (nn.strotss_utils.farthest_first relies on it)"""
    for n in (5, 4096, 2 ** 17 + 37):
        v = torch.zeros(n, device=DEV)
        v[n // 3] = v[n - 1] = 2.0
        v[n // 2] = v[n - 2] = -2.0
        assert int(torch.argmax(v)) == n // 3 and int(torch.argmin(v)) == min(n // 2, n - 2)
        assert int(torch.argmax(torch.ones(n, device=DEV))) == 0 and int(torch.argmin(torch.ones(n, device=DEV))) == 0


# ------------------------------------------------------------------ 2. the centre update
@pytest.mark.parametrize("shape", SHAPES)
def test_update_matches_float64(shape):
    from nn import _ops
    n, d, k = shape
    x, inv, _, ref_label, *_ = _case(n, d, k)
    ld = x.shape[1]
    label = ref_label.copy()
    if k >= 2:
        label[label == k - 1] = 0                                    # cluster k - 1 left empty on purpose
    if n >= 8:
        label[5], label[6] = k + 3, -1                               # outside 0..k-1: skipped, never an index
    rng = np.random.default_rng(n + d + k)
    start = np.zeros((k, ld), dtype=np.float32)
    start[:, :d] = rng.random((k, d))
    start[:, d:] = 7.0                                               # the padding of a written centre becomes zero
    want, want_count = R.update(x, inv, label, n, d, k, start[:, :d])
    xd, invd, labd = _dev(x), _dev(inv), _dev(label, torch.int32)
    runs = []
    for _ in range(2):
        cd = _dev(start)
        count = _ops.kmeans_update(xd, invd, labd, n, d, k, cd)
        runs.append((cd, count))
    torch.cuda.synchronize()
    assert torch.equal(runs[0][0].view(torch.int32), runs[1][0].view(torch.int32)) and torch.equal(runs[0][1], runs[1][1])
    got, count = runs[0][0].cpu().numpy(), runs[0][1].cpu().numpy()
    assert count.dtype == np.int32 and np.array_equal(count, want_count)
    err = np.abs(got[:, :d].astype(np.float64) - want)
    print(f"update n {n} d {d} k {k}: counts {count.tolist()}, largest error {err.max():.2e} = "
          f"{float((err / (U24 * np.abs(want) + 1e-10)).max()):.3f} of its bound")
    assert (err <= U24 * np.abs(want) + 1e-10).all()
    for j in range(k):
        if want_count[j] == 0:
            assert np.array_equal(got[j].view(np.int32), start[j].view(np.int32))       # bit for bit, padding included
        else:
            assert not got[j, d:].any()
    if k >= 2:
        assert want_count[k - 1] == 0


# ------------------------------------------------------------------ 3. the loop
@pytest.mark.parametrize("case", R.PLANTED)
def test_spherical_kmeans_finds_the_planted_labels(case):
    from nn import strotss_utils as U
    n, d, k = case[:3]
    x, planted = R.planted_rows(*case)
    ref = R.planted_result(case)
    label, centres, count, objective = U.spherical_kmeans(_dev(x), n, d, k)
    label, objective = label.cpu().numpy(), objective.cpu().numpy().astype(np.float64)
    E = R.assign_bound(d)
    print(f"planted n {n} d {d} k {k}: objective {objective[0]:.6f} -> {objective[-1]:.6f} (reference {ref['objective'][-1]:.6f})")
    assert np.array_equal(label, ref["label"])
    assert R.same_partition(label, planted, k)
    assert np.array_equal(count.cpu().numpy(), ref["count"]) and count.dtype == torch.int32
    assert len(objective) == U.AUTO_MASK_ITERS == R.ITERS and (np.diff(objective) >= -E).all()
    assert (np.abs(objective - np.array(ref["objective"])) <= E).all()
    norms = np.linalg.norm(centres.cpu().numpy().astype(np.float64), axis=1)
    assert (np.abs(norms - 1.0) <= 1e-6).all() and tuple(centres.shape) == (k, x.shape[1])


@pytest.mark.parametrize("case", R.UNSTRUCTURED)
def test_spherical_kmeans_ends_at_a_fixed_point_of_its_assignment(case):
    """on unstructured rows the labels returned are admissible against the centres returned"""
    from nn import strotss_utils as U
    n, d, k = case[:3]
    x, _ = R.planted_rows(*case)
    xd = _dev(x)
    label, centres, count, objective = U.spherical_kmeans(xd, n, d, k)
    again = U.spherical_kmeans(xd, n, d, k)
    assert torch.equal(label, again[0]) and torch.equal(centres.view(torch.int32), again[1].view(torch.int32))
    s = R.scores(x, R.inv_norm(x, n), n, d, centres.cpu().numpy())
    E = R.assign_bound(d)
    assert R.admissible(label.cpu().numpy(), s, E).all()
    assert int(count.sum()) == n and np.array_equal(count.cpu().numpy(), np.bincount(label.cpu().numpy(), minlength=k))
    assert (np.diff(objective.cpu().numpy().astype(np.float64)) >= -E).all()


# ------------------------------------------------------------------ 4. auto_masks
@pytest.fixture(scope="module")
def golden_pair():
    from nn import utils
    from nn.model import VGG
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    return vgg.params, utils.load_image(CONTENT, max_size=64), utils.load_image(STYLE, max_size=64)


def test_auto_masks_on_the_golden_pair(golden_pair):
    from nn import strotss_utils as U
    params, content, style = golden_pair
    c_masks, s_masks = U.auto_masks(params, content, style, 3)
    again = U.auto_masks(params, content, style, 3)
    found = U.auto_mask_regions(params, content, style, 3)
    kept = found["kept"]
    print(f"golden pair at 64 px, K = 3: {kept} regions, counts (content, style) {found['counts'].tolist()}")
    assert kept >= 2 and len(c_masks) == len(s_masks) == kept
    for image, masks, twice, grid in ((content, c_masks, again[0], found["content_grid"]),
                                      (style, s_masks, again[1], found["style_grid"])):
        H, W = int(image.shape[1]), int(image.shape[2])
        assert all(tuple(m.shape) == (H, W, 1) and m.dtype == torch.float32 for m in masks)
        assert bool(((torch.stack(masks) == 0) | (torch.stack(masks) == 1)).all())
        assert bool((torch.stack(masks).sum(dim=0) == 1).all())                      # a partition
        assert all(torch.equal(a, b) for a, b in zip(masks, twice))
        share = np.bincount(grid.cpu().numpy().reshape(-1), minlength=kept) / grid.numel()
        assert (share >= U.AUTO_MASK_MIN_SHARE).all()
        want = R.masks_from_labels(R.upsample_labels(grid.cpu().numpy(), H, W), kept)
        assert all(np.array_equal(m.cpu().numpy(), w) for m, w in zip(masks, want))
    n = found["n_c"] + found["n_s"]
    rows, inv = found["rows"].cpu().numpy(), found["inv_norm"].cpu().numpy()
    s = R.scores(rows, inv, n, found["d"], found["centres"].cpu().numpy())
    grid_labels = torch.cat([found["content_grid"].reshape(-1), found["style_grid"].reshape(-1)]).cpu().numpy()
    assert R.admissible(grid_labels, s, R.assign_bound(found["d"])).all()
    ys, xs = R.grid_points(int(content.shape[1]), int(content.shape[2]))
    assert tuple(found["content_grid"].shape) == (len(ys), len(xs)) and found["n_c"] == len(ys) * len(xs)


def test_auto_masks_falls_back_on_constant_images(golden_pair, caplog):
    from nn import strotss_utils as U
    params = golden_pair[0]
    content = torch.full((1, 40, 56, 3), 0.25, device=DEV)
    style = torch.full((1, 48, 36, 3), 0.75, device=DEV)
    with caplog.at_level(logging.WARNING):
        masks = U.auto_masks(params, content, style, 3)
    assert masks == ([None], [None])
    assert any("running unmasked" in r.getMessage() for r in caplog.records)


# ------------------------------------------------------------------ 5. the command line
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "30"]


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_auto_masks(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    seen = {}
    auto = RS.strotss.auto_masks

    def spy(*a, **k):
        seen["masks"] = auto(*a, **k)
        return seen["masks"]

    monkeypatch.setattr(RS.strotss, "auto_masks", spy)
    out = {name: str(tmp_path / f"{name}.jpg") for name in ("plain", "auto", "given", "bare")}
    parse = lambda name, extra: RS.build_parser().parse_args([CONTENT, STYLE, "-o", out[name]] + SETTINGS + extra)
    RS.run(parse("plain", []))
    RS.run(parse("auto", ["--auto_masks", "3", "--save_masks", str(tmp_path / "masks")]))
    c_masks, s_masks = seen["masks"]
    assert os.path.exists(out["auto"])
    if c_masks[0] is not None:
        assert len(c_masks) >= 2 and _bytes(out["auto"]) != _bytes(out["plain"])
    # the same run with the masks handed in where painted masks come from: the same bytes
    monkeypatch.setattr(RS, "_load_masks", lambda args: (c_masks, s_masks))
    RS.run(parse("given", []))
    monkeypatch.undo()
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    assert _bytes(out["given"]) == _bytes(out["auto"])
    # --save_masks: two PNGs of the images' sizes in the eight corner colours, the same partition
    for name, masks in (("content_mask.png", c_masks), ("style_mask.png", s_masks)):
        img = np.asarray(Image.open(tmp_path / "masks" / name).convert("RGB"))
        assert img.shape == tuple(masks[0].shape[:2]) + (3,) and np.isin(img, (0, 255)).all()
        region = (img[..., 0] // 255) * 4 + (img[..., 1] // 255) * 2 + img[..., 2] // 255
        for r, m in enumerate(masks):
            assert np.array_equal(region == r, m.cpu().numpy()[..., 0] == 1)
        assert region.max() == len(masks) - 1
    # without the flag nothing changes: a namespace without the attributes writes the plain run's bytes
    ns = parse("bare", [])
    assert ns.auto_masks is None and ns.save_masks is None
    delattr(ns, "auto_masks")
    delattr(ns, "save_masks")
    RS.run(ns)
    assert _bytes(out["bare"]) == _bytes(out["plain"])


def test_cli_auto_masks_with_colour_and_weight_map(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    ramp = np.tile(np.linspace(0, 255, 96).astype(np.uint8), (64, 1))
    Image.fromarray(ramp, "L").save(tmp_path / "weight.png")
    runs = {"auto": [], "match": ["--preserve_color", "match"], "weight": ["--content_weight_map", str(tmp_path / "weight.png")]}
    data = {}
    for name, extra in runs.items():
        path = str(tmp_path / f"{name}.jpg")
        RS.run(RS.build_parser().parse_args([CONTENT, STYLE, "-o", path, "--auto_masks", "3"] + SETTINGS + extra))
        data[name] = _bytes(path)
    assert data["match"] != data["auto"] and data["weight"] != data["auto"]
