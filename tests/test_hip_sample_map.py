"""--sample_map on the GPU: strotss_index_draw_weighted against its host twin element for element on
every case of _sample_map_cases.py and both selection paths, its two identities with strotss_index_draw bit for bit,
repeatability, refusals that touch nothing, proportionality of inclusion to the level, the StepEngine with levels (eager and
as the first node of the captured graph), and the command line."""
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

import _sample_map_cases as SC                    # noqa: E402
from nn import rand as RAND                       # noqa: E402
from nn import strotss_utils as SU                # noqa: E402

pytestmark = pytest.mark.gpu
GOLD = os.path.join(ROOT, "tests", "golden")


def _dev(a, dtype=None):
    return None if a is None else torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).cuda()


def _device_draw(case, general: bool, weighted: bool = True):
    """one call on the case -> (coordinates per region as written, n_out, counters after the call)"""
    from nn import _ops
    R = len(case["regions"])
    counters = torch.tensor([(case["t0"] + r) & 0xFFFFFFFF for r in range(R)], dtype=torch.int64).to(torch.int32).cuda()
    n_out = torch.full((R,), -1, dtype=torch.int32, device="cuda")
    out = [torch.full((case["n"], 2), -7.0, device="cuda") for _ in range(R)]
    masks = [_dev(m, np.uint8) for _, m in case["regions"]]
    if weighted:
        levels = [_dev(q) for q, _ in case["regions"]]
        _ops.index_draw_weighted(case["h"], case["w"], case["n"], case["seed"], counters, out, levels, masks, n_out,
                                 stride=case["stride"], general_path=general)
    else:
        _ops.index_draw(case["h"], case["w"], case["n"], case["seed"], counters, out, masks, n_out, stride=case["stride"],
                        general_path=general)
    torch.cuda.synchronize()
    return [o.cpu().numpy() for o in out], n_out.tolist(), [c & 0xFFFFFFFF for c in counters.tolist()]


@pytest.mark.parametrize("general", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("name", SC.CASE_NAMES)
def test_device_draw_equals_the_host_twin(name, general):
    """idx, n_out and the counters after the call; coordinates are small integers in float32: exact, no tolerance"""
    case = SC.BY_NAME[name]
    got, n_out, counters = _device_draw(case, general)
    want = SC.host_reference(name)
    assert counters == [(case["t0"] + r + case["stride"]) & 0xFFFFFFFF for r in range(len(want))]
    for r, ref in enumerate(want):
        assert n_out[r] == ref.shape[0], (name, r, n_out[r], ref.shape)
        assert got[r].dtype == np.float32 and np.array_equal(got[r][:n_out[r]], ref), (name, r)
        assert not got[r][n_out[r]:].any()                               # rows beyond the count: zeros


@pytest.mark.parametrize("general", [False, True], ids=["fast", "general"])
@pytest.mark.parametrize("name", [n for n in SC.CASE_NAMES if n.startswith("flat")])
def test_flat_maps_give_the_unweighted_entrys_bits(name, general):
    case = SC.BY_NAME[name]
    a, b = _device_draw(case, general), _device_draw(case, general, weighted=False)
    assert a[1] == b[1] and a[2] == b[2]
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))


def test_two_calls_from_the_same_counters_give_the_same_bits():
    for name in ("random_181x181", "three_regions", "two_level_A1023"):
        a, b = _device_draw(SC.BY_NAME[name], False), _device_draw(SC.BY_NAME[name], False)
        assert a[1] == b[1] and a[2] == b[2] and all(x.tobytes() == y.tobytes() for x, y in zip(a[0], b[0]))


def test_a_refused_call_leaves_idx_and_counters_untouched():
    import ctypes as C
    from nn import _hip, _ops
    counters = torch.tensor([5], dtype=torch.int32, device="cuda")
    out = [torch.full((1024, 2), -7.0, device="cuda")]
    levels = [_dev(SC.halves_map())]
    lv = _hip.DrawLevelsT()
    lv.level[0] = levels[0].data_ptr()
    d = _ops._draw_t(64, 64, 1024, 0, counters, out, None, None, None, False)
    assert _hip.lib().strotss_index_draw_weighted(C.byref(d), None, _ops.stream_ptr()) == -1       # lv == NULL
    d.sample_size = 1025
    assert _hip.lib().strotss_index_draw_weighted(C.byref(d), C.byref(lv), _ops.stream_ptr()) == -1
    d.sample_size, d.h, d.w = 1024, 1024, 1024           # at step 1: more than 32768 candidates
    assert _hip.lib().strotss_index_draw_weighted(C.byref(d), C.byref(lv), _ops.stream_ptr()) == -3
    torch.cuda.synchronize()
    assert int(counters[0]) == 5 and bool((out[0] == -7.0).all())


def test_inclusion_is_proportional_to_the_level_on_the_device():
    """the statement and the margin of test_sample_map_cpu.py: 200 draws from one advancing counter"""
    from nn import _ops
    levels = [_dev(SC.halves_map())]
    counters = torch.tensor([0], dtype=torch.int32, device="cuda")
    out = [torch.zeros((1024, 2), device="cuda")]
    draws = []
    for _ in range(200):
        _ops.index_draw_weighted(64, 64, 1024, 123, counters, out, levels)
        draws.append(out[0].clone())
    torch.cuda.synchronize()
    assert int(counters[0]) == 200
    draws = [d.cpu().numpy() for d in draws]
    ratio = SC.inclusion_ratio(draws)
    print(f"inclusion frequency on the device, level 65535 over level 16384: {ratio:.4f} (expected 4)")
    assert abs(ratio / 4.0 - 1.0) < 0.03
    twin = RAND.PhiloxStream(123, 0)                                     # and the first and last draws are the host twin's
    first = SU.make_indices_weighted_np(64, 64, 1024, twin, SC.halves_map())
    twin.skip(198)
    last = SU.make_indices_weighted_np(64, 64, 1024, twin, SC.halves_map())
    assert np.array_equal(draws[0], first) and np.array_equal(draws[-1], last)


# ------------------------------------------------------------------ engine
def _engine_run(mode, levels, monkeypatch):
    """three steps at 64 px, two mask regions; -> (index sets used in each step, variables after the steps)"""
    import _region_worker as W
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    dev = torch.device("cuda", 0)
    eng, _ = W.problem(dev, None, h=64, w=64, regions=2)
    masks = []
    for a, b in ((0, 32), (32, 64)):
        m = np.zeros((64, 64), dtype=bool); m[:, a:b] = True
        masks.append(m)
    assert eng.enable_device_draw(11, 100, masks, **({} if levels is None else dict(sample_levels=levels)))
    if mode == "graph":
        eng.capture_graph()
        assert eng._graph is not None and eng._graph_drawn
    used = []
    for _ in range(3):
        eng.step()
        torch.cuda.synchronize()
        used.append([i.cpu().numpy().copy() for i in eng._draw["idx"]])
    assert eng.draws_done() == 6 and eng._draw["counters"].tolist() == [106, 107]
    return used, [v.clone() for v in eng.variables], masks, eng.sample_size


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_engine_draws_the_host_twins_indices(mode, monkeypatch):
    levels = SC.BY_NAME["random_64x64"]["regions"][0][0]
    per_region = [levels, SC.halves_map()]
    used, _, masks, n = _engine_run(mode, per_region, monkeypatch)
    twin = RAND.PhiloxStream(11, 100)
    for step in range(3):
        for r in range(2):
            want = SU.make_indices_weighted_np(64, 64, n, twin, per_region[r], masks[r])
            assert np.array_equal(used[step][r], want), (mode, step, r)
    one, _, _, _ = _engine_run(mode, levels, monkeypatch)               # one array: used for every region
    twin = RAND.PhiloxStream(11, 100)
    for r in range(2):
        assert np.array_equal(one[0][r], SU.make_indices_weighted_np(64, 64, n, twin, levels, masks[r]))


@pytest.mark.parametrize("mode", ["eager", "graph"])
def test_engine_with_flat_levels_equals_the_engine_without(mode, monkeypatch):
    flat = np.full((64, 64), 65535, dtype=np.uint16)
    used_a, var_a, _, _ = _engine_run(mode, flat, monkeypatch)
    used_b, var_b, _, _ = _engine_run(mode, None, monkeypatch)
    assert all(np.array_equal(x, y) for sa, sb in zip(used_a, used_b) for x, y in zip(sa, sb))
    assert all(torch.equal(a, b) for a, b in zip(var_a, var_b))


# ------------------------------------------------------------------ command line
def test_run_with_sample_map(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")      # sorted tap scatter: two runs of one configuration are bitwise alike
    with Image.open(os.path.join(GOLD, "content_im.jpg")) as im:
        cw, ch = im.size
    white = np.full((ch, cw), 255, dtype=np.uint8)
    half = white.copy()
    half[:, cw // 2:] = 0
    for name, arr in (("white.png", white), ("half.png", half)):
        Image.fromarray(arr).save(tmp_path / name)
    base = [os.path.join(GOLD, "content_im.jpg"), os.path.join(GOLD, "style_im.jpg"), "--max_size", "64", "--level", "1",
            "--max_iter", "5"]
    runs = {"plain": [], "white": ["--sample_map", str(tmp_path / "white.png")],
            "half": ["--sample_map", str(tmp_path / "half.png")],
            "half_host": ["--sample_map", str(tmp_path / "half.png"), "--host_draw"]}
    data, traces = {}, {}
    for k, extra in runs.items():
        traces[k] = []
        RS.run(RS.build_parser().parse_args(base + ["-o", str(tmp_path / f"{k}.jpg")] + extra), trace=traces[k])
        data[k] = open(tmp_path / f"{k}.jpg", "rb").read()
    assert data["white"] == data["plain"]                # all 65535: the unweighted draw's bits, hence the same steps
    assert data["half"] != data["plain"]
    assert data["half_host"] == data["half"]             # the host loop draws the same weighted sequence
    assert traces["half_host"][0]["steps"] == traces["half"][0]["steps"]
    assert all(np.isfinite(st[k]) for st in traces["half"][0]["steps"] for k in ("loss", "loss_c", "loss_s"))
