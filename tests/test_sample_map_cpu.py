"""--sample_map without a GPU: the host twin of the weighted index draw (its two identities with the
unweighted draw, its use of the stream, the accepted count on the threshold, proportionality of inclusion to the level), the
command line and its refusals, the level helper's refusals, and the status codes of refused C calls (nothing launches)."""
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

import _sample_map_cases as SC                    # noqa: E402
from nn import rand as RAND                       # noqa: E402
from nn import strotss_utils as SU                # noqa: E402

EINVAL, ERANGE = -1, -3
IDENTITY_CASES = [n for n in SC.CASE_NAMES if n.startswith("flat")]


@pytest.mark.parametrize("name", IDENTITY_CASES)
def test_flat_maps_give_the_unweighted_draw(name):
    """all 65535: every candidate in class 0; all 0: every candidate in class 1 -- the order is (key, j) either way"""
    case = SC.BY_NAME[name]
    got = SC.host_reference(name)[0]
    want = SC.host_region(case, 0, weighted=False)
    assert got.dtype == want.dtype == np.float32 and got.shape == want.shape
    assert np.array_equal(got, want)


def test_weighted_and_unweighted_calls_consume_the_stream_alike():
    a, b = RAND.PhiloxStream(7, 11), RAND.PhiloxStream(7, 11)
    levels = SC.BY_NAME["random_300x200_n100"]["regions"][0][0]
    for _ in range(3):
        SU.make_indices_weighted_np(300, 200, 1024, a, levels)
        SU.make_indices_np(300, 200, True, 1024, b)
        assert a.t == b.t and a._k == b._k == 0
    assert a.t == 14
    # the acceptance words are their own Philox blocks (c1 = 3), not the shuffle keys' (c1 = 0)
    s = RAND.PhiloxStream(7, 11)
    assert np.array_equal(s.accept_words(9), np.stack(RAND.philox4x32_10(np.arange(3), 3, 11, 0, *s.key), axis=1).reshape(-1)[:9])
    assert not np.array_equal(s.accept_words(64), s.keys(64))


@pytest.mark.parametrize("a", SC.THRESHOLD_A)
def test_accepted_count_on_the_threshold(a):
    case = SC.BY_NAME[f"two_level_A{a}"]
    levels = case["regions"][0][0]
    assert int((levels == 65535).sum()) == a and int((levels == 0).sum()) == 4096 - a
    got = SC.host_reference(case["name"])[0]
    assert got.shape == (1024, 2)
    x, y = got[:, 0].astype(int), got[:, 1].astype(int)
    head = min(a, 1024)
    assert (levels[x[:head], y[:head]] == 65535).all()                   # the accepted first ...
    assert (levels[x[head:], y[head:]] == 0).all()                       # ... the rest filled from the rejected
    assert len(set(zip(x.tolist(), y.tolist()))) == 1024                 # no coordinate repeats
    if a <= 1024:                                                        # every accepted cell is in
        assert len(set(zip(x[:head].tolist(), y[:head].tolist()))) == a


def test_fewer_candidates_than_samples_returns_all_accepted_first():
    case = SC.BY_NAME["random_20x30"]
    got = SC.host_reference(case["name"])[0]
    assert got.shape == (600, 2)
    assert len(set(map(tuple, got.astype(int).tolist()))) == 600
    levels = case["regions"][0][0]
    stream = RAND.PhiloxStream(case["seed"], case["t0"])
    q = levels.T.reshape(-1).astype(np.uint64)            # candidate order: meshgrid 'xy', rows fastest
    accepted = (q == 65535) | ((stream.accept_words(600) >> np.uint64(16)) < q)
    na = int(accepted.sum())
    pos = got[:, 0].astype(int) + 20 * got[:, 1].astype(int)
    assert accepted[pos[:na]].all() and not accepted[pos[na:]].any()
    keys = stream.keys(600)
    assert np.all(np.diff(keys[pos[:na]].astype(np.int64)) >= 0) and np.all(np.diff(keys[pos[na:]].astype(np.int64)) >= 0)


def test_masked_draw_stays_inside_its_mask():
    for name in ("random_64x64_mask_few", "random_64x64_mask_many", "three_regions"):
        case = SC.BY_NAME[name]
        for r, (levels, mask) in enumerate(case["regions"]):
            got = SC.host_reference(name)[r].astype(int)
            assert got.shape[0] == min(case["n"], int(mask.sum()))
            assert mask[got[:, 0], got[:, 1]].all()


def test_inclusion_is_proportional_to_the_level():
    """Left half level 65535, right half 16384 (acceptance exactly 1/4): given the accepted set every accepted candidate is
    equally likely, so the per-candidate inclusion frequency left over right is 4 up to O(1 / accepted).  200 draws put
    about 41 000 samples on the right half (standard deviation about 0.5 %): the margin of 3 % is six of them."""
    levels = SC.halves_map()
    stream = RAND.PhiloxStream(123, 0)
    draws = [SU.make_indices_weighted_np(64, 64, 1024, stream, levels) for _ in range(200)]
    assert stream.t == 200
    ratio = SC.inclusion_ratio(draws)
    print(f"inclusion frequency, level 65535 over level 16384: {ratio:.4f} (expected 4)")
    assert abs(ratio / 4.0 - 1.0) < 0.03


# ------------------------------------------------------------------ levels of a scale
def test_sample_levels_at_scale_refuses_nan_and_all_zero_maps():
    with pytest.raises(ValueError):
        SU.sample_levels_at_scale(np.array([[0.5, np.nan], [0.5, 0.5]], dtype=np.float32), 4, 4)
    with pytest.raises(ValueError):
        SU.sample_levels_at_scale(np.array([[0.5, np.inf], [0.5, 0.5]], dtype=np.float32), 4, 4)
    with pytest.raises(ValueError):
        SU.sample_levels_at_scale(np.zeros((8, 8), dtype=np.float32), 4, 4)
    with pytest.raises(ValueError):
        SU.sample_levels_at_scale(np.ones((8,), dtype=np.float32), 4, 4)
    with pytest.raises(ValueError):                                      # the host twin takes uint16 levels of the scale's size
        SU.make_indices_weighted_np(8, 8, 16, RAND.PhiloxStream(0), np.ones((8, 8), dtype=np.float32))
    with pytest.raises(ValueError):
        SU.make_indices_weighted_np(8, 8, 16, RAND.PhiloxStream(0), np.ones((8, 4), dtype=np.uint16))


def test_load_sample_map(tmp_path):
    import torch
    from PIL import Image
    grey = np.zeros((6, 9), dtype=np.uint8)
    grey[:, :3] = 255
    grey[:, 3:6] = 128
    Image.fromarray(grey).save(tmp_path / "m.png")
    m = SU.load_sample_map(str(tmp_path / "m.png"))
    assert tuple(m.shape) == (6, 9) and m.dtype == torch.float32
    assert torch.equal(m, torch.from_numpy(grey.astype(np.float32) / np.float32(255)))


# ------------------------------------------------------------------ command line
def _args(*extra):
    import run_strotss as RS
    return RS.build_parser().parse_args(["/nonexistent/c.jpg", "/nonexistent/s.jpg", *extra])


def test_flag_is_listed_parsed_and_documented():
    import run_strotss as RS
    names = [n for names, _ in RS._FLAGS for n in names]
    assert "--sample_map" in names
    assert [names[0] for names, _ in RS._FLAGS[-3:]] == ["--detail_weight", "--detail_pool", "--tv_weight"]
    assert "--sample_map PATH" in RS.__doc__
    assert "--sample_map" in RS.build_parser().format_help()
    assert _args().sample_map is None and _args("--sample_map", "m.png").sample_map == "m.png"
    a = _args("--sample_map", "m.png", "--content_weight_map", "w.png", "--auto_masks", "3", "--style_transport", "sliced",
              "--video")
    assert a.sample_map == "m.png" and a.content_weight_map == "w.png" and a.video


def test_sample_map_input_refuses_before_anything_is_loaded(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    path = str(tmp_path / "m.png")
    Image.fromarray(np.full((4, 4), 255, dtype=np.uint8)).save(path)
    assert RS._sample_map_input(_args()) is None
    assert RS._sample_map_input(_args("--sample_map", path)) == path
    assert RS._sample_map_input(_args("--sample_map", path, "--style_mix", "a.jpg", "--content_mask", "c", "--style_mask", "s",
                                      "--content_weight_map", "w.png")) == path
    with pytest.raises(ValueError, match="strips"):
        RS._sample_map_input(_args("--sample_map", path, "--strips"))
    with pytest.raises(ValueError, match="no such file"):
        RS._sample_map_input(_args("--sample_map", str(tmp_path / "missing.png")))
    # run() refuses before it reads the (nonexistent) content and style images, with and without --video
    with pytest.raises(ValueError, match="strips"):
        RS.run(_args("--sample_map", path, "--strips"))
    with pytest.raises(ValueError, match="no such file"):
        RS.run(_args("--sample_map", str(tmp_path / "missing.png")))
    with pytest.raises(ValueError, match="no such file"):
        RS.run(_args("--sample_map", str(tmp_path / "missing.png"), "--video"))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(ValueError, match="one GPU"):
        RS._sample_map_input(_args("--sample_map", path))
    with pytest.raises(ValueError, match="one GPU"):
        RS.run(_args("--sample_map", path))
    assert RS._sample_map_input(_args()) is None         # no map: a multi-process run is not this flag's business


# ------------------------------------------------------------------ refused C calls
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_weighted_entry_refuses_before_launching(lib):
    from nn import _hip
    assert hasattr(lib, "strotss_index_draw_weighted")
    P = 0x10000                                          # "some buffer": non-null, never touched

    def draw(h=64, w=64, sx=1, sy=1, n=1024, regions=1, counter=P, idx=P):
        d = _hip.DrawT()
        d.h, d.w, d.step_x, d.step_y, d.sample_size, d.n_regions, d.counter_stride = h, w, sx, sy, n, regions, regions
        d.counter = counter
        for r in range(min(max(regions, 0), _hip.MAX_DRAW_REGIONS)):
            d.idx[r] = idx
        return d
    lv = _hip.DrawLevelsT()
    lv.level[0] = P

    def call(d, levels=lv):
        return lib.strotss_index_draw_weighted(C.byref(d) if d is not None else None,
                                               C.byref(levels) if levels is not None else None, None)
    assert call(draw(), levels=None) == EINVAL
    assert call(None) == EINVAL
    bad = [(draw(counter=None), EINVAL), (draw(h=0), EINVAL), (draw(w=-1), EINVAL), (draw(sx=0), EINVAL), (draw(sy=0), EINVAL),
           (draw(regions=0), EINVAL), (draw(regions=17), EINVAL), (draw(n=0), EINVAL), (draw(n=1025), EINVAL),
           (draw(idx=None), EINVAL), (draw(h=182, w=181), ERANGE), (draw(h=1024, w=1024), ERANGE)]
    for d, code in bad:
        assert call(d) == code
        assert lib.strotss_index_draw(C.byref(d), None) == code          # the unweighted entry refuses alike
