"""Mask refinement on the MI355X: strotss_refine_labels pixel by pixel against the float64 restatement
(tests/_refine_ref.py) at the shapes where the kernels can go wrong -- tests/test_refine_cpu.py shows that no margin of the
planted cases is within the bound E, so their labels compare exactly -- ties, foreign labels, auto_masks(refine=) on the
golden pair, the fallback when refinement empties a region, and --refine_masks through the command line."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _refine_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _check(got, ref, k, sigma_r, what, exact):
    """labels equal the reference's where the margin is wide and are admissible everywhere, best and second within eps best
    (half of E: the bound of ONE vote), the counts are the bincount of the kernel's own labels, the cell colours are the
    float32 roundings of the float64 means"""
    label, count, best, second, mean = (None if t is None else t.cpu().numpy() for t in got)
    assert label.dtype == np.int32 and count.dtype == np.int32 and best.dtype == np.float64
    assert ((0 <= label) & (label < k)).all()
    E = R.bound(ref["best"], sigma_r)
    wide = (ref["best"] - ref["second"]) > E
    ok = R.admissible(label, ref["vote"], ref["present"], ref["best"], sigma_r)
    err_b = np.abs(best - ref["best"])
    both = np.isfinite(ref["second"])
    err_s = np.abs(second[both] - ref["second"][both])
    err_m = np.abs(mean.astype(np.float64) - ref["means"])
    print(f"{what}: {100 * float((~wide).mean()):.3f} % of the pixels within E = {2 * R.vote_eps(sigma_r):.2e} best; largest "
          f"|best - ref| / best {float((err_b / ref['best']).max()):.2e} (allowed {R.vote_eps(sigma_r):.2e}); "
          f"{int((label != ref['label']).sum())} labels differ from the reference's; largest mean error "
          f"{float((err_m / np.maximum(ref['means'], 1e-30)).max()):.2e} of the mean")
    assert ok.all()
    assert np.array_equal(label[wide], ref["label"][wide])
    if exact:
        assert wide.all()
    assert (err_b <= E / 2).all()
    assert (err_s <= E[both] / 2).all() and np.array_equal(np.isneginf(second), ~both)
    assert np.array_equal(count, np.bincount(label.reshape(-1), minlength=k)) and count.sum() == label.size
    assert (err_m <= (R.U24 + 2.0 ** -33) * np.abs(ref["means"])).all()


# ------------------------------------------------------------------ 1. the kernels against the restatement
@pytest.mark.parametrize("case", R.CASES + [R.UNSTRUCTURED], ids=R.case_id)
def test_refine_matches_float64(case):
    from nn import _ops
    (H, W, gh, gw, k), radius, sigma_r = case
    img, grid, ref = R.case_result(case)
    imgd, gridd = _dev(img), _dev(grid, torch.int32)
    got = _ops.refine_labels(imgd, gridd, k, radius, R.SIGMA_S, sigma_r, votes=True, means=True)
    again = _ops.refine_labels(imgd, gridd, k, radius, R.SIGMA_S, sigma_r, votes=True)
    bare = _ops.refine_labels(imgd, gridd, k, radius, R.SIGMA_S, sigma_r)         # best and second NULL
    torch.cuda.synchronize()
    assert tuple(got[0].shape) == (H, W) and tuple(got[1].shape) == (k,) and tuple(got[4].shape) == (gh, gw, 3)
    assert torch.equal(got[0], again[0]) and torch.equal(got[1], again[1])       # the same bits on a second call
    assert torch.equal(got[2].view(torch.int64), again[2].view(torch.int64))
    assert torch.equal(got[3].view(torch.int64), again[3].view(torch.int64))
    assert bare[2] is None and bare[3] is None and torch.equal(got[0], bare[0]) and torch.equal(got[1], bare[1])
    _check(got, ref, k, sigma_r, R.case_id(case), exact=case != R.UNSTRUCTURED)


def test_ties_go_to_the_lower_label():
    """a constant image: the colour factor is exactly 1; the middle pixel of three over two cells sits exactly between them"""
    from nn import _ops
    img = np.full((1, 3, 3), 0.25, dtype=np.float32)
    for grid, want in (([[1, 0]], [[1, 0, 0]]), ([[0, 1]], [[0, 0, 1]])):
        label, count, best, second, _ = _ops.refine_labels(_dev(img), _dev(grid, torch.int32), 2, 2, 1.0, 0.1, votes=True)
        assert label.tolist() == want and count.tolist() == [2, 1]
        assert float(best[0, 1]) == float(second[0, 1]) > 0
    # a column of five pixels over four cells, labels 3 2 1 0: the middle pixel (u = 1.5) is between cells 1 and 2
    img = np.full((5, 1, 3), 0.5, dtype=np.float32)
    label, _, best, second, _ = _ops.refine_labels(_dev(img), _dev([[3], [2], [2], [3]], torch.int32), 4, 1, 1.0, 0.1, votes=True)
    ref = R.refine(img, np.array([[3], [2], [2], [3]], dtype=np.int32), 4, radius=1)
    assert label[:, 0].tolist() == ref["label"][:, 0].tolist() and int(label[2, 0]) == 2


def test_foreign_labels_cast_no_vote():
    """cells whose label lies outside 0..k-1 are skipped by comparison; absent labels cannot win; nothing faults"""
    from nn import _ops
    rng = np.random.default_rng(5)
    img = rng.random((33, 47, 3)).astype(np.float32)
    grid = rng.integers(0, 3, size=(5, 7)).astype(np.int32)
    grid[0, 0], grid[2, 3], grid[4, 6], grid[1, 5] = 3, 16, -1, 2 ** 30
    ref = R.refine(img, grid, 3)
    got = _ops.refine_labels(_dev(img), _dev(grid, torch.int32), 3, R.RADIUS, R.SIGMA_S, R.SIGMA_R, votes=True, means=True)
    _check(got, ref, 3, R.SIGMA_R, "foreign labels", exact=False)
    clean = np.where((grid >= 0) & (grid < 3), grid, 0)
    assert not np.array_equal(R.refine(img, clean, 3)["vote"], ref["vote"])      # the skipped cells would have counted
    # no label of 0..k-1 anywhere: label 0, best = second = -inf
    label, count, best, second, _ = _ops.refine_labels(_dev(img), _dev(np.full((5, 7), 9), torch.int32), 3, 2, 1.0, 0.1, votes=True)
    assert not bool(label.any()) and count.tolist() == [33 * 47, 0, 0]
    assert bool(torch.isneginf(best).all()) and bool(torch.isneginf(second).all())


def test_wrapper_refuses_a_grid_larger_than_the_image():
    from nn import _ops, strotss_utils as U
    img = torch.zeros((4, 6, 3), device=DEV)
    with pytest.raises(ValueError, match="grid"):
        _ops.refine_labels(img, torch.zeros((5, 6), dtype=torch.int32, device=DEV), 2, 2, 1.0, 0.1)
    with pytest.raises(ValueError, match="grid"):
        U.refine_labels(img, torch.zeros((4, 7), dtype=torch.int32, device=DEV), 2)


# ------------------------------------------------------------------ 2. auto_masks(refine=)
@pytest.fixture(scope="module")
def golden_pair():
    from nn import utils
    from nn.model import VGG
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    return vgg.params, utils.load_image(CONTENT, max_size=256), utils.load_image(STYLE, max_size=256)


def test_auto_masks_refined_on_the_golden_pair(golden_pair):
    from nn import strotss_utils as U
    params, content, style = golden_pair
    plain = U.auto_masks(params, content, style, 3)
    fine = U.auto_masks(params, content, style, 3, refine=0.1)
    again = U.auto_masks(params, content, style, 3, refine=0.1)
    found = U.auto_mask_regions(params, content, style, 3)
    kept = found["kept"]
    assert kept >= 2 and len(fine[0]) == len(fine[1]) == len(plain[0]) == kept
    changed = 0
    for image, masks, twice, coarse, grid in ((content, fine[0], again[0], plain[0], found["content_grid"]),
                                              (style, fine[1], again[1], plain[1], found["style_grid"])):
        H, W = int(image.shape[1]), int(image.shape[2])
        assert all(tuple(m.shape) == (H, W, 1) and m.dtype == torch.float32 for m in masks)
        stack = torch.stack(masks)
        assert bool(((stack == 0) | (stack == 1)).all()) and bool((stack.sum(dim=0) == 1).all())       # a partition
        assert all(torch.equal(a, b) for a, b in zip(masks, twice))
        label = stack[..., 0].argmax(dim=0).cpu().numpy().astype(np.int32)
        ref = R.refine(image[0].cpu().numpy(), grid.cpu().numpy(), kept)
        wide = (ref["best"] - ref["second"]) > R.bound(ref["best"], 0.1)
        print(f"golden pair {H} x {W}, grid {tuple(grid.shape)}: {int((~wide).sum())} pixels within E, counts "
              f"{np.bincount(label.reshape(-1), minlength=kept).tolist()}")
        assert np.array_equal(label[wide], ref["label"][wide])        # the masks of the reference on the kernel's own grid
        assert R.admissible(label, ref["vote"], ref["present"], ref["best"], 0.1).all()
        assert (np.bincount(label.reshape(-1), minlength=kept) >= U.AUTO_MASK_MIN_SHARE * H * W).all()
        changed += sum(int((a != b).sum()) for a, b in zip(masks, coarse))
    print(f"refinement moved {changed // 2} pixels to another region")
    assert changed > 0


def test_refinement_that_empties_a_region_falls_back(caplog):
    from nn import strotss_utils as U
    img = torch.full((1, 40, 40, 3), 0.5, device=DEV)
    grid = torch.zeros((10, 10), dtype=torch.int32, device=DEV)
    grid[4, 6] = 1                                                    # a lone cell in a constant image: voted away
    label, count = U.refine_labels(img, grid, 2)
    assert not bool(label.any()) and count.tolist() == [1600, 0] and count.dtype == torch.int32
    with caplog.at_level(logging.WARNING):
        masks = U.masks_from_grids(img, img, grid, grid, 2, refine=0.1)
    assert any("keeping the unrefined masks" in r.getMessage() for r in caplog.records)
    plain = U.masks_from_grids(img, img, grid, grid, 2)
    nearest = R.upsample_labels(grid.cpu().numpy(), 40, 40)
    for side, same in zip(masks, plain):
        assert all(torch.equal(a, b) for a, b in zip(side, same))
        assert np.array_equal(side[1].cpu().numpy()[..., 0], (nearest == 1).astype(np.float32)) and int(side[1].sum()) == 16
    # two halves survive the refinement: no warning, the refined masks
    caplog.clear()
    grid[:, 5:] = 1
    with caplog.at_level(logging.WARNING):
        masks = U.masks_from_grids(img, img, grid, grid, 2, refine=0.1)
    assert not caplog.records and int(masks[0][1].sum()) == 800


# ------------------------------------------------------------------ 3. the command line
SETTINGS = ["--max_size", "64", "--max_iter", "5"]


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def test_cli_refine_masks(tmp_path, monkeypatch):
    import run_strotss as RS
    from nn import strotss_utils as U
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    seen = []
    auto = RS.strotss.auto_masks

    def spy(*a, **k):
        seen.append((k, auto(*a, **k)))
        return seen[-1][1]

    monkeypatch.setattr(RS.strotss, "auto_masks", spy)
    out = {name: str(tmp_path / f"{name}.jpg") for name in ("fine", "coarse")}
    parse = lambda name, extra: RS.build_parser().parse_args([CONTENT, STYLE, "-o", out[name]] + extra + SETTINGS)
    RS.run(parse("fine", ["--auto_masks", "4", "--refine_masks", "--save_masks", str(tmp_path / "fine")]))
    RS.run(parse("coarse", ["--auto_masks", "4", "--save_masks", str(tmp_path / "coarse")]))
    (kw_fine, used_fine), (kw_coarse, used_coarse) = seen
    assert kw_fine == {"refine": 0.1} and kw_coarse == {}             # without the flag the call is the parent commit's
    assert os.path.exists(out["fine"]) and os.path.exists(out["coarse"])
    assert used_fine[0][0] is not None and used_coarse[0][0] is not None
    for name, used in (("fine", used_fine), ("coarse", used_coarse)):  # --save_masks writes what the run uses
        back = U.load_mask(str(tmp_path / name / "content_mask.png"), str(tmp_path / name / "style_mask.png"), None,
                           sample_threth=1)
        for side, wrote in zip(used, back):
            assert len(side) == len(wrote) and all(torch.equal(a.cpu(), b.cpu()) for a, b in zip(side, wrote))
    # without the flag: the masks are upsample_labels of the grids, as before
    monkeypatch.undo()
    from nn import utils
    from nn.model import VGG
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    content, style = utils.load_image(CONTENT, max_size=64), utils.load_image(STYLE, max_size=64)
    found = U.auto_mask_regions(vgg.params, content, style, 4)
    for image, grid, side in ((content, found["content_grid"], used_coarse[0]), (style, found["style_grid"], used_coarse[1])):
        labels = U.upsample_labels(grid, int(image.shape[1]), int(image.shape[2]))
        assert len(side) == found["kept"] and all(torch.equal(m, (labels == j).float()[..., None]) for j, m in enumerate(side))
    moved = sum(int((a != b).sum()) for a, b in zip(used_fine[0], used_coarse[0]))
    print(f"--refine_masks at 64 px: {moved // 2} content pixels in another region; the outputs "
          f"{'differ' if _bytes(out['fine']) != _bytes(out['coarse']) else 'are equal'}")
