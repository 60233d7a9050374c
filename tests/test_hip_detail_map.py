"""--sample_map auto on the GPU: strotss_detail_map element by element against the float64 statement
of tests/_detail_map_ref.py on random and step-edge images at every shape of DR.SHAPES, exactness on a constant image,
repeatability, and the command line (the identity with the plain run on a constant content, a real content, --host_draw,
--save_sample_map, --video).

Tolerance.  Per case E32 = max |float32 twin - float64 reference| is measured on the host; the device may be off by
4 E32 + 1e-7.  The factor 4 covers another float32 operation order and contraction (the window sums are float64 on both
sides); 1e-7 is one unit in the last place of a level near 1.  Nothing of the bound comes from the kernel's output."""
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _detail_map_ref as DR                      # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def _device_map(img, r, gain, floor):
    from nn import _ops
    return _ops.detail_map(torch.from_numpy(np.ascontiguousarray(img)).cuda(), r, gain, floor)


@pytest.mark.parametrize("params", DR.PARAMS, ids=lambda p: f"g{p[0]}_f{p[1]}")
@pytest.mark.parametrize("shape", DR.SHAPES, ids=lambda s: "x".join(map(str, s[:2])) + f"_r{s[2]}")
@pytest.mark.parametrize("kind", DR.KINDS)
def test_device_map_against_float64(kind, shape, params):
    img, ref, twin, e32 = DR.case(kind, shape, params)
    got = _device_map(img, shape[2], *params)
    assert got.dtype == torch.float32 and tuple(got.shape) == shape[:2]
    got = got.cpu().numpy().astype(np.float64)
    err = float(np.abs(got - ref).max())
    bound = 4.0 * e32 + 1e-7
    print(f"detail_map {kind} {shape} gain={params[0]} floor={params[1]}: E32={e32:.3e} device_err={err:.3e} "
          f"bound={bound:.3e} twin_mismatches={int((got != twin).sum())}")
    assert np.isfinite(got).all() and got.min() >= np.float32(params[1]) and got.max() <= 1.0
    assert err <= bound
    if params[1] == 1.0:
        assert np.array_equal(got, np.ones_like(got))
    if params == (0.25, 0.0) and kind == "random" and shape[0] * shape[1] > 1:
        assert (ref == 1.0).any() and (got == 1.0).any()     # the clamp acts


@pytest.mark.parametrize("shape", [(1, 1, 1), (5, 7, 8), (33, 65, 4), DR.BIG], ids=str)
def test_a_constant_image_gives_all_ones_exactly(shape):
    h, w, r = shape
    img = np.empty((h, w, 3), dtype=np.float32)
    img[...] = np.float32([0.3, 0.7, 0.55])
    for gain, floor in DR.PARAMS + [(2.0, 0.1)]:
        got = _device_map(img, r, gain, floor).cpu().numpy()
        assert np.array_equal(got, np.ones((h, w), dtype=np.float32))


def test_two_calls_give_the_same_bits_and_leave_the_workspace_ready():
    h, w, r = DR.BIG
    img = torch.from_numpy(DR.image("random", h, w)).cuda()
    other = torch.from_numpy(DR.image("edge", h, w)).cuda()
    from nn import _ops
    a = _ops.detail_map(img, r)
    _ops.detail_map(other, r)                                # the same workspace, another image in between
    b = _ops.detail_map(img, r)
    assert torch.equal(a, b)
    assert torch.equal(_ops.detail_map(img), _ops.detail_map(img, max(1, max(h, w) // 64), 2.0, 0.25))


def test_auto_sample_map_is_a_host_map_like_a_painted_one():
    from nn import strotss_utils as SU
    img = DR.image("random", 33, 65)
    m = SU.auto_sample_map(torch.from_numpy(img)[None].cuda(), 4, None, None)
    assert m.device.type == "cpu" and m.dtype == torch.float32 and tuple(m.shape) == (33, 65)
    ref, e32 = DR.case("random", (33, 65, 4), (2.0, 0.25))[1], DR.case("random", (33, 65, 4), (2.0, 0.25))[3]
    assert np.abs(m.numpy().astype(np.float64) - ref).max() <= 4.0 * e32 + 1e-7
    levels = SU.sample_levels_at_scale(m, 33, 65)
    assert levels.dtype == np.uint16 and levels.min() >= int(0.25 * 65535)
    with pytest.raises(ValueError, match="radius"):
        SU.auto_sample_map(torch.from_numpy(img).cuda(), 65)


# ------------------------------------------------------------------ command line
def _run(tmp_path, tag, content, extra, trace=None):
    import run_strotss as RS
    out = str(tmp_path / f"{tag}.jpg")
    RS.run(RS.build_parser().parse_args([content, os.path.join(GOLD, "style_im.jpg"), "--max_size", "64", "--level", "1",
                                         "--max_iter", "4", "-o", out] + extra), trace=trace)
    return open(out, "rb").read()


def test_run_on_a_constant_content_writes_the_plain_runs_bytes(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")      # sorted tap scatter: two runs of one configuration are bitwise alike
    flat = str(tmp_path / "flat.png")
    Image.fromarray(np.full((48, 64, 3), (90, 140, 200), dtype=np.uint8)).save(flat)
    plain = _run(tmp_path, "plain", flat, [])
    auto = _run(tmp_path, "auto", flat, ["--sample_map", "auto", "--save_sample_map", str(tmp_path / "maps")])
    assert auto == plain                                     # the map is all ones, the levels all 65535: section 28's identity
    with Image.open(tmp_path / "maps" / "sample_map.png") as im:
        assert im.mode == "L" and im.size == (64, 48) and np.array_equal(np.asarray(im), np.full((48, 64), 255, dtype=np.uint8))


def test_run_on_a_real_content(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    from nn import strotss_utils as SU
    from nn import utils as U
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    content = os.path.join(GOLD, "content_im.jpg")
    traces = {k: [] for k in ("auto", "host")}
    plain = _run(tmp_path, "plain", content, [])
    auto = _run(tmp_path, "auto", content, ["--sample_map", "auto", "--save_sample_map", str(tmp_path / "maps")], traces["auto"])
    host = _run(tmp_path, "host", content, ["--sample_map", "auto", "--host_draw"], traces["host"])
    assert auto != plain
    assert host == auto                                      # the host loop draws the same weighted sequence (section 28)
    assert traces["host"][0]["steps"] == traces["auto"][0]["steps"]
    assert all(np.isfinite(st[k]) for st in traces["auto"][0]["steps"] for k in ("loss", "loss_c", "loss_s"))
    loaded = U.load_image(content, max_size=64)
    h, w = int(loaded.shape[1]), int(loaded.shape[2])
    with Image.open(tmp_path / "maps" / "sample_map.png") as im:
        assert im.mode == "L" and im.size == (w, h)          # the content's loaded size
        saved = np.asarray(im)
    want = SU.auto_sample_map(loaded, None, None, None).numpy()
    assert np.array_equal(saved, np.rint(want.astype(np.float64) * 255.0).astype(np.uint8))
    assert saved.min() >= 63 and len(np.unique(saved)) > 1   # floor 0.25; a photograph's map is not constant


def test_run_with_other_parameters_and_a_saved_map_read_back(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    content = os.path.join(GOLD, "content_im.jpg")
    maps = str(tmp_path / "maps")
    auto = _run(tmp_path, "auto", content, ["--sample_map", "auto"])
    other = _run(tmp_path, "other", content, ["--sample_map", "auto", "--sample_radius", "1", "--sample_gain", "0.5",
                                              "--sample_floor", "0", "--save_sample_map", maps])
    assert other != auto                                     # the parameters reach the map, hence the draws
    back = _run(tmp_path, "back", content, ["--sample_map", os.path.join(maps, "sample_map.png")])
    assert back[:2] == b"\xff\xd8"                           # the 8-bit map is a painted map like any other


def test_run_video_writes_one_map_per_frame(tmp_path):
    import run_strotss as RS
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three shifted crops of one texture
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    RS.run(RS.build_parser().parse_args(
        [frames, style, "--video", "--compute_flow", "-o", str(tmp_path / "out"), "--max_size", "64", "--level", "1",
         "--max_iter", "4", "--sample_map", "auto", "--sample_radius", "2", "--save_sample_map", str(tmp_path / "maps")]))
    stems = [os.path.splitext(os.path.basename(q))[0] for q in paths]
    assert len(stems) == 3 and sorted(os.listdir(tmp_path / "out")) == sorted(t + ".jpg" for t in stems)
    assert sorted(os.listdir(tmp_path / "maps")) == sorted(f"sample_map_{t}.png" for t in stems)
    maps = []
    for t in stems:
        with Image.open(tmp_path / "maps" / f"sample_map_{t}.png") as im:
            assert im.mode == "L" and im.size == (64, 48)
            maps.append(np.asarray(im).copy())
    assert not np.array_equal(maps[0], maps[1]) and not np.array_equal(maps[1], maps[2])     # a map per frame, of that frame
