"""Region tracking on the MI355X: strotss_label_warp cell for cell against the integer restatement,
strotss_kmeans_assign_prior row by row against float64 and bit for bit against strotss_kmeans_assign where no bias applies
(tests/_track_ref.py; tests/test_track_cpu.py shows how few rows lie within the float32 bound), the refusals of both entries
with their outputs untouched, and --auto_masks K --video --track_masks through the command line."""
import logging
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _cluster_ref as R  # noqa: E402
import _temporal_long_ref as TL  # noqa: E402
import _temporal_ref as T  # noqa: E402
import _track_ref as TR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CONTENT, STYLE = os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg")
U23 = 2.0 ** -23


def _dev(a, dtype=torch.float32):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype, device=DEV)


def _bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


# ------------------------------------------------------------------ A. the prior along the flow
@pytest.mark.parametrize("shape", TR.WARP_SHAPES)
def test_label_warp_equals_the_restatement(shape):
    from nn import _ops
    h, w, gh, gw = shape
    side = torch.cuda.Stream()
    for name, grid, flow, cert in TR.warp_cases(h, w, gh, gw):
        want = TR.label_warp(grid, TR.WARP_K, flow, cert)
        g, f, c = _dev(grid, torch.int32), _dev(flow), None if cert is None else _dev(cert)
        got = _ops.label_warp(g, TR.WARP_K, f, c)
        again = _ops.label_warp(g, TR.WARP_K, f, c)
        torch.cuda.synchronize()
        with torch.cuda.stream(side):
            aside = _ops.label_warp(g, TR.WARP_K, f, c)
        side.synchronize()
        assert got.dtype == torch.int32 and tuple(got.shape) == (gh, gw)
        assert np.array_equal(got.cpu().numpy(), want), name
        assert torch.equal(got, again) and torch.equal(got, aside), name


# ------------------------------------------------------------------ B. the biased assignment
@pytest.mark.parametrize("shape", TR.ASSIGN_SHAPES)
@pytest.mark.parametrize("beta", TR.BETAS)
def test_assign_prior_matches_float64(shape, beta):
    from nn import _ops
    n, d, k = shape
    x, inv, c32, prior = TR.assign_case(n, d, k)
    ref_label, ref_best, ref_second, s, score = TR.assign_prior(x, inv, n, d, c32, prior, beta)
    xd, invd, cd, pd = _dev(x), _dev(inv), _dev(c32), _dev(prior, torch.int32)
    got = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, pd, beta)
    again = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, pd, beta)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        aside = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, pd, beta)
    side.synchronize()
    for a, b, c in zip(got, again, aside):                           # the same bits on a second call and on a side stream
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))
    label, best, second = (t.cpu().numpy() for t in got)
    E = R.assign_bound(d)
    tol = E / 2 + U23
    exact = TR.exact_rows(x, inv, n, d)
    wide = (TR.biased_margin(score) > E) | exact
    same = label == ref_label
    err_b = np.abs(best - ref_best)[same]
    print(f"assign_prior n {n} d {d} k {k} beta {beta}: {100 * float((~wide).mean()):.2f} % of the rows within E = {E:.2e}; "
          f"{int((~same).sum())} labels differ from the reference's; largest |best - ref| {err_b.max():.2e} (allowed {tol:.2e})")
    assert label.dtype == np.int32 and ((0 <= label) & (label < k)).all()
    assert R.admissible(label, score, E).all()                       # within E of the largest biased score
    assert np.array_equal(label[wide], ref_label[wide])
    assert (err_b <= tol).all()
    if k == 1:
        assert np.isneginf(second[inv[:n] != 0]).all()
    else:
        assert (np.abs(second - ref_second)[same] <= tol).all()
    if n >= 3:                                                       # the zero row and the row of inverse norm 0
        want = prior[1] if beta > 0 else 0
        assert label[1] == want and label[2] == want and best[1] == 0 and best[2] == 0 and second[2] == 0
    if beta == 2.0:
        valid = (prior[:n] >= 0) & (prior[:n] < k)
        assert np.array_equal(label[valid], prior[:n][valid])        # exactly: a label with a prior never changes


@pytest.mark.parametrize("shape", TR.ASSIGN_SHAPES)
def test_assign_prior_without_a_bias_is_kmeans_assign_bit_for_bit(shape):
    from nn import _ops
    n, d, k = shape
    x, inv, c32, prior = TR.assign_case(n, d, k)
    xd, invd, cd = _dev(x), _dev(inv), _dev(c32)
    plain = _ops.kmeans_assign(xd, invd, n, d, cd, k)
    zero = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, _dev(prior, torch.int32), 0.0)
    none = _ops.kmeans_assign_prior(xd, invd, n, d, cd, k, _dev(np.full_like(prior, -1), torch.int32), 0.05)
    for got in (zero, none):
        for a, b in zip(got, plain):
            assert torch.equal(_bits(a), _bits(b))


def test_assign_prior_breaks_ties_toward_the_lowest_centre_and_reports_raw_scores():
    from nn import _ops
    x = np.zeros((32, 32), dtype=np.float32)
    x[:5, :3] = [0.25, 0.5, 0.125]
    c = np.zeros((4, 32), dtype=np.float32)
    c[:, :3] = [[0, 0, 1], [0, 1, 0], [0, 1, 0], [1, 0, 0]]       # exact products: 0.125, 0.5, 0.5, 0.25
    inv = np.ones(32, dtype=np.float32)
    prior = np.full(32, -1, dtype=np.int32)
    prior[:5] = [-1, 2, 3, 0, 7]
    call = lambda beta: [t.tolist() for t in _ops.kmeans_assign_prior(_dev(x), _dev(inv), 5, 3, _dev(c), 4,
                                                                      _dev(prior, torch.int32), beta)]
    label, best, second = call(0.125)                                # 3 reaches 0.375, 0 reaches 0.25: neither wins
    assert label == [1, 2, 1, 1, 1] and best == [0.5] * 5 and second == [0.5] * 5
    label, best, second = call(0.25)                                 # 3 ties with 1 at 0.5: the lowest j
    assert label == [1, 2, 1, 1, 1]
    label, best, second = call(0.5)                                  # 3 wins at 0.75, 0 at 0.625: best raw, second the others' top
    assert label == [1, 2, 3, 0, 1] and best == [0.5, 0.5, 0.25, 0.125, 0.5] and second == [0.5] * 5


# ------------------------------------------------------------------ the refusals leave the outputs untouched
def test_entries_refuse_bad_arguments_with_outputs_untouched():
    from nn import _hip
    lib = _hip.lib()
    st = _hip.stream_ptr()
    grid = _dev(np.zeros((5, 7)), torch.int32)
    flow, cert = _dev(np.zeros((21, 32, 2))), _dev(np.ones((21, 32)))
    prior = torch.full((35,), 77, dtype=torch.int32, device=DEV)
    p = lambda t: t.data_ptr()
    warp = lambda g=p(grid), gh=5, gw=7, k=3, f=p(flow), c=p(cert), h=21, w=32, out=p(prior): \
        lib.strotss_label_warp(g, gh, gw, k, f, c, h, w, out, st)
    for bad in (dict(g=None), dict(f=None), dict(gh=0), dict(gw=0), dict(h=0), dict(w=-1), dict(gh=22), dict(gw=33),
                dict(k=0), dict(k=17)):
        assert warp(**bad) == -1, bad
    for bad in (dict(g=p(grid) + 4), dict(f=p(flow) + 4), dict(c=p(cert) + 4), dict(out=p(prior) + 4)):
        assert warp(**bad) == -2, bad
    assert warp(out=None) == -1
    x, inv, c = _dev(np.ones((32, 64))), _dev(np.ones(32)), _dev(np.ones((3, 64)))
    pr = _dev(np.zeros(32), torch.int32)
    label = torch.full((32,), 77, dtype=torch.int32, device=DEV)
    best, second = torch.full((32,), 7.0, device=DEV), torch.full((32,), 7.0, device=DEV)
    assign = lambda x_=p(x), n=8, d=35, ld=64, k=3, pr_=p(pr), beta=0.05, lab=p(label): \
        lib.strotss_kmeans_assign_prior(x_, p(inv), n, d, ld, p(c), k, pr_, beta, lab, p(best), p(second), st)
    for bad in (dict(x_=None), dict(pr_=None), dict(n=0), dict(d=0), dict(d=65), dict(k=0), dict(k=17), dict(beta=-0.5),
                dict(beta=2.5), dict(beta=float("nan")), dict(beta=float("inf")), dict(n=2 ** 26)):
        assert assign(**bad) == -1, bad
    for bad in (dict(ld=48), dict(x_=p(x) + 4), dict(pr_=p(pr) + 4), dict(lab=p(label) + 4)):
        assert assign(**bad) == -2, bad
    torch.cuda.synchronize()
    assert bool((prior == 77).all()) and bool((label == 77).all()) and bool((best == 7).all()) and bool((second == 7).all())
    assert warp() == 0 and assign() == 0                             # and the good calls run
    torch.cuda.synchronize()
    assert bool((prior == 0).all()) and bool((label[:8] != 77).all()) and bool((label[8:] == 77).all())


# ------------------------------------------------------------------ the host path
def test_track_regions_with_results_smaller_than_the_grid():
    """a 171 x 256 frame has a 43 x 64 clustering grid, its 64-px result is 42 x 64: flow and certainty are brought to the
    clustering image's size before the warp.  A zero flow then hands every cell its own earlier label, and beta = 2 keeps it."""
    from nn import strotss_utils as U
    from nn import utils
    from nn.model import VGG
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    frame = _dev(T.texture(171, 256, 3))[None].contiguous()
    got = U.frame_rows(vgg.params, frame)
    assert got["grid"] == (43, 64) and got["size"] == (171, 256)
    rows = got["rows"][[0, got["n"] - 1]] * got["inv_norm"][[0, got["n"] - 1], None]
    grid = torch.from_numpy(np.random.default_rng(0).integers(0, 2, size=(43, 64)).astype(np.int32)).to(DEV)
    state = dict(kept=2, centres=rows.contiguous(), grid=grid, present=[0, 1], mask_grid=grid)
    flow, cert = torch.zeros((42, 64, 2), device=DEV), torch.ones((42, 64), device=DEV)
    out = U.track_regions(state, vgg.params, frame, flow, cert, beta=2.0)
    assert torch.equal(out["prior"], grid) and torch.equal(out["grid"], grid) and out["present"] == [0, 1]
    none = U.track_regions(state, vgg.params, frame, None, None, beta=2.0)
    assert bool((none["prior"] == -1).all())
    plain = U._ops.kmeans_assign(got["rows"], got["inv_norm"], got["n"], got["d"], state["centres"], 2)[0]
    assert torch.equal(none["grid"].reshape(-1), plain)              # no prior: the plain assignment to the fixed centres
    half = torch.zeros((42, 64), device=DEV)
    assert bool((U.track_regions(state, vgg.params, frame, flow, half, beta=2.0)["prior"] == -1).all())


# ------------------------------------------------------------------ end to end
SETTINGS = ["--max_size", "64", "--level", "1", "--max_iter", "5"]
COLOURS = {tuple(c) for c in R.CORNER_COLOURS}


def _bytes(path):
    with open(path, "rb") as f:
        return f.read()


def _colours(path):
    from PIL import Image
    img = np.asarray(Image.open(path).convert("RGB"))
    return img.shape[:2], {tuple(int(v) for v in c) for c in np.unique(img.reshape(-1, 3), axis=0)}


def test_cli_static_scene_keeps_its_masks(tmp_path, monkeypatch):
    """three copies of one frame and zero flows: the same features, every prior the cell's own label -- the content masks of
    frames 2 and 3 are frame 1's byte for byte, the style mask is written once"""
    import shutil
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, flows, masks, out = (tmp_path / n for n in ("frames", "flows", "masks", "out"))
    frames.mkdir()
    flows.mkdir()
    stems = ["frame_01", "frame_02", "frame_03"]
    for s in stems:
        shutil.copy(CONTENT, frames / f"{s}.jpg")
    with Image.open(CONTENT) as im:
        w, h = im.size
    for t in (2, 3):
        T.write_flo(flows / f"backward_{t}_{t - 1}.flo", np.zeros((h, w, 2), np.float32))
        T.write_flo(flows / f"forward_{t - 1}_{t}.flo", np.zeros((h, w, 2), np.float32))
    RS.run(RS.build_parser().parse_args([str(frames), STYLE, "-o", str(out), "--video", "--flow_dir", str(flows), "--auto_masks",
                                         "3", "--track_masks", "--save_masks", str(masks)] + SETTINGS))
    assert all((out / f"{s}.jpg").exists() for s in stems)
    assert sorted(os.listdir(masks)) == sorted(["style_mask.png"] + [f"content_mask_{s}.png" for s in stems])
    first = _bytes(masks / f"content_mask_{stems[0]}.png")
    assert _bytes(masks / f"content_mask_{stems[1]}.png") == first and _bytes(masks / f"content_mask_{stems[2]}.png") == first
    shape, used = _colours(masks / f"content_mask_{stems[0]}.png")
    assert len(used) >= 2 and used <= COLOURS                        # the golden pair has regions (test_hip_cluster.py)


@pytest.mark.parametrize("source", ["compute_flow", "flow_dir"])
def test_cli_moving_scene(source, tmp_path, monkeypatch, caplog):
    """the occluder sequence with K = 2, flows computed or read, --refine_masks on the computed ones: the run completes, one
    content mask per frame in the kept colours.  The synthetic VGG may or may not tell the two textures apart: an unmasked
    sequence with the warning is a pass as well."""
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, flows, masks, out = (str(tmp_path / n) for n in ("frames", "flows", "masks", "out"))
    paths, _ = TL.occluder_sequence(frames, flows, n_frames=3, offsets=(1,))
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    extra = ["--compute_flow", "--refine_masks"] if source == "compute_flow" else ["--flow_dir", flows]
    with caplog.at_level(logging.WARNING):
        RS.run(RS.build_parser().parse_args([frames, style, "-o", out, "--video", "--auto_masks", "2", "--track_masks",
                                             "--save_masks", masks] + extra + SETTINGS))
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    assert all(os.path.exists(os.path.join(out, f"{s}.jpg")) for s in stems)
    if any("running the sequence unmasked" in r.getMessage() for r in caplog.records):
        print(f"{source}: frame 1 gave fewer than two regions; the sequence ran unmasked")
        assert not os.path.exists(masks)
        return
    shape, used = _colours(os.path.join(masks, "style_mask.png"))
    kept = len(used)
    allowed = set(sorted(COLOURS)[:kept])
    assert kept == 2 and used == allowed
    unmasked = [r.getMessage() for r in caplog.records if "running this frame unmasked" in r.getMessage()]
    print(f"{source}: {kept} regions; {len(unmasked)} frames ran unmasked")
    assert sorted(os.listdir(masks)) == sorted(["style_mask.png"] + [f"content_mask_{s}.png" for s in stems])
    for s in stems:
        shape, used = _colours(os.path.join(masks, f"content_mask_{s}.png"))
        assert shape == (48, 64) and used <= allowed
