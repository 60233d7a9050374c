"""--sample_map auto without a GPU: properties of the float64 statement and its float32 twin
(tests/_detail_map_ref.py), the status codes of refused strotss_detail_map calls (nothing launches), the command line and
its refusals before anything is loaded."""
import argparse
import ctypes as C
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _detail_map_ref as DR                      # noqa: E402

EINVAL, EALIGN, ERANGE = -1, -2, -3
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)
NULL = None


# ------------------------------------------------------------------ 1. the statement
@pytest.mark.parametrize("fn", [DR.detail_map_ref, DR.detail_map_f32])
def test_a_constant_image_gives_all_ones(fn):
    img = np.full((11, 13, 3), 0.37, dtype=np.float32)
    for floor in (0.0, 0.25, 1.0):
        assert np.array_equal(fn(img, 3, 2.0, floor), np.ones((11, 13)))
    assert np.array_equal(fn(np.zeros((1, 1, 3), dtype=np.float32), 1), np.ones((1, 1)))


@pytest.mark.parametrize("fn", [DR.detail_map_ref, DR.detail_map_f32])
@pytest.mark.parametrize("gain,floor", DR.PARAMS + [(1.0, 0.1), (8.0, 0.9)])
def test_the_output_lies_between_the_floor_and_one(fn, gain, floor):
    for kind in DR.KINDS:
        out = fn(DR.image(kind, 33, 65), 4, gain, floor)
        assert out.shape == (33, 65) and np.isfinite(out).all()
        assert out.min() >= np.float32(floor) and out.max() <= 1.0
    if floor == 1.0:
        assert np.array_equal(out, np.ones_like(out))


def test_the_small_gain_case_clamps_and_the_default_one_does_not_everywhere():
    img = DR.image("random", 33, 65)
    clamped = DR.detail_map_ref(img, 4, 0.25, 0.0)
    assert (clamped == 1.0).any()
    edge = DR.detail_map_ref(DR.image("edge", 33, 65), 4, 2.0, 0.25)
    assert (edge == 1.0).any() and (edge == 0.25).any()      # on the edge; far from it


@pytest.mark.parametrize("fn", [DR.detail_map_ref, DR.detail_map_f32])
def test_the_flat_half_sits_on_the_floor_away_from_the_border(fn):
    h, w, r, floor = 24, 40, 3, 0.25
    img = np.random.default_rng(3).random((h, w, 3), dtype=np.float32)
    img[:, :w // 2] = np.float32([0.4, 0.5, 0.6])
    out = fn(img, r, 2.0, floor)
    assert np.array_equal(out[:, :w // 2 - (r + 1)], np.full((h, w // 2 - (r + 1)), floor))
    assert (out[:, w // 2 - r - 1] > floor).all()            # the first column whose window reaches a gradient
    assert (out[:, w // 2:] > floor).all()


def test_a_window_larger_than_the_image_gives_the_global_mean():
    img = DR.image("random", 5, 7)
    e = DR.energy(img, np.float64)
    for r in (7, 8, 64):
        s = DR.local_detail(img, r)
        assert np.allclose(s, np.sqrt(e.mean()), rtol=1e-14, atol=0)
        out = DR.detail_map_ref(img, r, 2.0, 0.25)           # s == m everywhere: 0.25 + 0.75 / 2
        assert np.allclose(out, 0.625, rtol=1e-14, atol=0)
    assert np.ptp(DR.local_detail(img, 2)) > 0


def test_the_gradient_is_the_halved_central_difference_with_clamped_indices():
    y = np.zeros((3, 4, 3))
    y[1, 2] = 1.0                                            # luma 1 at (1, 2): the weights sum to 1
    e = DR.energy(y, np.float64)
    want = np.zeros((3, 4))
    want[1, 1] = want[1, 3] = want[0, 2] = want[2, 2] = 0.25
    assert np.allclose(e, want, atol=1e-15)
    assert np.array_equal(DR.energy(np.random.default_rng(0).random((1, 1, 3)), np.float64), np.zeros((1, 1)))
    row = DR.energy(np.random.default_rng(0).random((1, 9, 3)), np.float64)
    col = DR.energy(np.random.default_rng(0).random((1, 9, 3)).transpose(1, 0, 2), np.float64)
    assert np.array_equal(row.T, col) and (row > 0).all()    # a 1-pixel axis adds nothing


def test_the_twin_is_close_to_the_statement():
    for kind in DR.KINDS:
        for shape in DR.SHAPES[:-1]:
            for params in DR.PARAMS:
                assert DR.case(kind, shape, params)[3] < 1e-5


def test_window_counts():
    n = DR.window_counts(5, 7, 2)
    assert n[0, 0] == 9 and n[2, 3] == 25 and n[4, 6] == 9 and n[2, 0] == 15
    assert (DR.window_counts(5, 7, 8) == 35).all()


# ------------------------------------------------------------------ 2. the C entry's refusals
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_detail_map_refusals(lib):
    call = lib.strotss_detail_map
    nan, inf = float("nan"), float("inf")
    assert call(NULL, 8, 8, 2, 2.0, 0.25, P, P, NULL) == EINVAL
    assert call(P, 8, 8, 2, 2.0, 0.25, NULL, P, NULL) == EINVAL
    assert call(P, 8, 8, 2, 2.0, 0.25, P, NULL, NULL) == EINVAL
    for h, w in ((0, 8), (8, 0), (-1, 8), (8, -3), (26755, 26755)):      # 3 * 26755^2 > INT_MAX
        assert call(P, h, w, 2, 2.0, 0.25, P, P, NULL) == EINVAL
    for radius in (0, -1, 65, 1 << 20):
        assert call(P, 8, 8, radius, 2.0, 0.25, P, P, NULL) == ERANGE
    for gain in (0.0, -1.0, nan, inf, -inf):
        assert call(P, 8, 8, 2, gain, 0.25, P, P, NULL) == ERANGE
    for floor in (-0.01, 1.01, nan, inf, -inf):
        assert call(P, 8, 8, 2, 2.0, floor, P, P, NULL) == ERANGE
    assert call(ODD, 8, 8, 2, 2.0, 0.25, P, P, NULL) == EALIGN
    assert call(P, 8, 8, 2, 2.0, 0.25, ODD, P, NULL) == EALIGN
    assert call(P, 8, 8, 2, 2.0, 0.25, P, ODD, NULL) == EALIGN
    # the order of the three classes: sizes and null pointers first, then the parameters, then the alignment
    assert call(NULL, 8, 8, 0, 2.0, 0.25, ODD, P, NULL) == EINVAL
    assert call(ODD, 8, 8, 0, 2.0, 0.25, P, P, NULL) == ERANGE


def test_detail_map_workspace_bytes(lib):
    size = lib.strotss_detail_map_workspace_bytes
    for h, w in ((0, 8), (8, 0), (-1, 8), (26755, 26755)):
        assert size(h, w) == 0
    for h, w in ((1, 1), (5, 7), (33, 65), (150, 293), (1024, 1024)):
        n = size(h, w)
        assert n % 8 == 0 and 8 * h * w + 32 <= n <= 8 * h * w + 32 + 8 * 512
    assert size(33, 65) == 32 + 8 * 34 + 8 * 33 * 65                    # one partial per 256 pixels of a row (33, an even count)
    assert size(1024, 1024) == 32 + 8 * 512 + 8 * 1024 * 1024           # ... of at most 512 workgroups


# ------------------------------------------------------------------ 3. the command line
def _args(*extra, content="c.jpg"):
    import run_strotss as RS
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


def test_parser_knows_auto_and_its_four_flags():
    import run_strotss as RS
    ns = _args()
    assert ns.sample_map is None and ns.sample_radius is None and ns.sample_gain is None and ns.sample_floor is None
    assert ns.save_sample_map is None
    ns = _args("--sample_map", "auto", "--sample_radius", "5", "--sample_gain", "1.5", "--sample_floor", "0.1",
               "--save_sample_map", "maps")
    assert (ns.sample_map, ns.sample_radius, ns.sample_gain, ns.sample_floor, ns.save_sample_map) == ("auto", 5, 1.5, 0.1, "maps")
    with pytest.raises(SystemExit):
        _args("--sample_map", "auto", "--sample_radius", "2.5")
    assert RS._auto_sample_input(ns) == (5, 1.5, 0.1, "maps")
    assert RS._auto_sample_input(_args("--sample_map", "auto")) == (None, None, None, None)
    assert RS._auto_sample_input(_args()) is None
    assert RS._auto_sample_input(argparse.Namespace()) is None           # a namespace from before the flags existed


def test_docstring_and_help_mention_the_flags():
    import run_strotss as RS
    text = RS.build_parser().format_help()
    for flag in ("--sample_radius", "--sample_gain", "--sample_floor", "--save_sample_map"):
        assert flag in RS.__doc__ and flag in text
    assert "--sample_map PATH" in RS.__doc__ and "--sample_map PATH" in text
    assert "--sample_map auto" in RS.__doc__ and "auto" in text
    assert "section 29" in RS.__doc__ and "not tuned" in text
    kw = dict((names[0], kw) for names, kw in RS._FLAGS)
    assert kw["--sample_map"]["metavar"] == "PATH"


def test_the_flags_stand_directly_behind_sample_map_and_the_tail_is_unchanged():
    import run_strotss as RS
    first = [names[0] for names, _ in RS._FLAGS]
    at = first.index("--sample_map")
    assert first[at + 1:at + 5] == ["--sample_radius", "--sample_gain", "--sample_floor", "--save_sample_map"]
    assert first[-3:] == ["--detail_weight", "--detail_pool", "--tv_weight"] and at + 5 == len(first) - 3


def test_sample_map_input_returns_auto_without_a_file_check(monkeypatch, tmp_path):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    monkeypatch.chdir(tmp_path)                              # no file called "auto" here
    assert not os.path.exists("auto")
    assert RS._sample_map_input(_args("--sample_map", "auto")) == "auto"
    assert RS._sample_map_input(_args("--sample_map", "auto", "--style_mix", "a.jpg", "--content_weight_map", "w.png",
                                      "--host_draw", "--auto_masks", "3")) == "auto"
    with pytest.raises(ValueError, match="--strips"):
        RS._sample_map_input(_args("--sample_map", "auto", "--strips"))
    with pytest.raises(ValueError, match="no such file"):
        RS._sample_map_input(_args("--sample_map", "Auto"))   # the literal word only
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS._sample_map_input(_args("--sample_map", "auto"))
    with pytest.raises(ValueError, match="one GPU"):
        RS._auto_sample_input(_args("--sample_map", "auto", "--sample_radius", "0"))     # --sample_map's refusals first


AUTO = ["--sample_map", "auto"]
REFUSALS = [(["--sample_radius", "4"], "needs --sample_map auto"), (["--sample_gain", "2"], "needs --sample_map auto"),
            (["--sample_floor", "0.5"], "needs --sample_map auto"), (["--save_sample_map", "maps"], "needs --sample_map auto"),
            (AUTO + ["--sample_radius", "0"], "radius"), (AUTO + ["--sample_radius", "65"], "radius"),
            (AUTO + ["--sample_radius", "-3"], "radius"),
            (AUTO + ["--sample_gain", "0"], "gain"), (AUTO + ["--sample_gain", "-1"], "gain"),
            (AUTO + ["--sample_gain", "nan"], "gain"), (AUTO + ["--sample_gain", "inf"], "gain"),
            (AUTO + ["--sample_floor", "-0.1"], "floor"), (AUTO + ["--sample_floor", "1.5"], "floor"),
            (AUTO + ["--sample_floor", "nan"], "floor"), (AUTO + ["--strips"], "--strips")]


@pytest.mark.parametrize("extra,match", REFUSALS)
def test_auto_sample_map_is_refused_before_anything_is_loaded(extra, match, monkeypatch, tmp_path):
    """the paths do not exist: loading anything would be a FileNotFoundError, not the ValueError asked for"""
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    video = [str(tmp_path / "no_frames"), missing[1], "-o", str(tmp_path / "out"), "--video", "--compute_flow"]
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    for base in (missing, video):
        with pytest.raises(ValueError, match=match):
            RS.run(RS.build_parser().parse_args(base + extra))
    assert not os.path.exists(tmp_path / "out.jpg") and not os.path.exists(tmp_path / "out")
    assert not os.path.exists(tmp_path / "maps")


def test_the_four_flags_are_refused_with_a_painted_map(monkeypatch, tmp_path):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    painted = str(tmp_path / "painted.png")
    Image.fromarray(np.full((8, 8), 255, dtype=np.uint8)).save(painted)
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    for extra in (["--sample_radius", "4"], ["--sample_gain", "2"], ["--sample_floor", "0.5"], ["--save_sample_map", "m"]):
        with pytest.raises(ValueError, match="needs --sample_map auto"):
            RS.run(RS.build_parser().parse_args(missing + ["--sample_map", painted] + extra))


def test_auto_is_refused_on_several_ranks(monkeypatch, tmp_path):
    import run_strotss as RS
    missing = [str(tmp_path / "no_content.jpg"), str(tmp_path / "no_style.jpg"), "-o", str(tmp_path / "out.jpg")]
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(RS.build_parser().parse_args(missing + AUTO))


# ------------------------------------------------------------------ 4. the host helpers
def test_parameter_checks_and_the_default_radius():
    from nn import strotss_utils as SU
    assert [SU.default_sample_radius(*hw) for hw in ((1, 1), (63, 64), (127, 128), (512, 384), (100, 5000))] == [1, 1, 2, 8, 64]
    assert SU.DEFAULT_SAMPLE_GAIN == 2.0 and SU.DEFAULT_SAMPLE_FLOOR == 0.25
    SU.check_sample_parameters(None, None, None)
    SU.check_sample_parameters(1, 1e-3, 0.0)
    SU.check_sample_parameters(64, 100.0, 1.0)
    for bad in ((0, None, None), (65, None, None), (2.5, None, None), (None, 0.0, None), (None, float("inf"), None),
                (None, None, -1e-3), (None, None, 1.001), (None, None, float("nan"))):
        with pytest.raises(ValueError):
            SU.check_sample_parameters(*bad)


def test_a_saved_map_loads_back_as_a_painted_one(tmp_path):
    from nn import strotss_utils as SU
    m = DR.detail_map_f32(DR.image("random", 9, 14), 2)
    path = str(tmp_path / "deep" / "sample_map.png")
    SU.save_sample_map(path, m)
    back = SU.load_sample_map(path).numpy()
    assert back.shape == (9, 14) and back.dtype == np.float32
    assert np.array_equal(back, (np.rint(m.astype(np.float64) * 255.0) / 255.0).astype(np.float32))
    assert np.abs(back - m).max() <= 0.5 / 255 + 1e-7
