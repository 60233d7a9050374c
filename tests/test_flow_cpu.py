"""Optical flow of --video sequences without a GPU: the numpy restatement of strotss_optical_flow on
known motion (the acceptance table's two conditions), the .flo writer, the --compute_flow / --save_flow command line and
its refusals, the header's declarations, and the status codes of refused strotss_optical_flow calls (checked before
anything launches).  And the conditions of the device tests' cases (_flow_cases.py): the restatement runs on each, its
level count is the expected one, the float32 yardstick is positive and below the cap, degenerate frames give exactly 0, and
strotss_flow_workspace_bytes is the total the restatement's levels imply."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _flow_cases as FC  # noqa: E402
import _flow_ref as R  # noqa: E402
import _temporal_ref as T  # noqa: E402

EINVAL, EALIGN = -1, -2
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)        # non-null, not 16-byte aligned
FLOW_SYMBOLS = ("strotss_flow_default_params", "strotss_flow_workspace_bytes", "strotss_optical_flow")


def _args(*extra, content="c.jpg"):
    import run_strotss as RS
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


# ------------------------------------------------------------------ the restatement on known motion
@pytest.mark.parametrize("h,w,shift", R.KNOWN_MOTION, ids=[f"{h}x{w}" for h, w, _ in R.KNOWN_MOTION])
def test_restatement_recovers_a_translation(h, w, shift):
    prev, cur = R.translated_pair(h, w, shift)
    dx, dy = shift
    fb = R.optical_flow(cur, prev)                       # frame t -> t-1: -shift
    ff = R.optical_flow(prev, cur)                       # frame t-1 -> t: +shift
    assert fb.shape == (h, w, 2) and fb.dtype == np.float64
    mean_b, max_b = R.interior_epe(fb, (-dx, -dy))
    mean_f, max_f = R.interior_epe(ff, (dx, dy))
    agree = R.certainty_agreement(fb, ff, shift)
    print(f"{h} x {w}, shift {shift}: interior EPE backward mean {mean_b:.4f} max {max_b:.3f}, forward mean {mean_f:.4f} "
          f"max {max_f:.3f}, certainty agreement {agree:.4f}")
    assert mean_b < R.MAX_INTERIOR_MEAN_EPE and mean_f < R.MAX_INTERIOR_MEAN_EPE
    assert agree >= R.MIN_AGREEMENT


def test_restatement_is_dtype_parametrised_and_has_the_pyramid_of_the_statement():
    assert R.level_sizes(48, 64) == [(48, 64), (24, 32), (12, 16)]
    assert R.level_sizes(42, 63) == [(42, 63), (21, 32)]
    assert R.level_sizes(768, 1024)[-1] == (12, 16) and len(R.level_sizes(768, 1024)) == 7
    assert len(R.level_sizes(768, 1024, max_levels=3)) == 3
    a, b = R.smooth_pair(42, 63, 5)
    f64, f32 = R.optical_flow(a, b), R.optical_flow(a, b, np.float32)
    assert f64.dtype == np.float64 and f32.dtype == np.float32
    d = float(np.abs(f32 - f64).max())
    print(f"42 x 63 smooth pair: max |F_f32 - F_f64| = {d:.3e}, max |F| = {np.abs(f64).max():.2f}")
    assert 0 < d < 1e-3 and np.abs(f64).max() > 0.5      # float32 rounding, and a real motion
    # identical frames: no motion at all
    assert not R.optical_flow(a, a).any()


def test_blur_and_sampling_rules():
    g = np.zeros((7, 9))
    g[3, 4] = 256.0
    k = np.array([1, 4, 6, 4, 1.0])
    assert np.array_equal(R.blur(g)[1:6, 2:7], np.outer(k, k))
    assert np.allclose(R.blur(np.full((5, 6), 0.25)), 0.25)          # clamped edges keep a constant
    img = np.arange(12.0).reshape(3, 4)
    ys, xs = np.mgrid[0:3, 0:4].astype(np.float64)
    assert np.array_equal(R.bilinear(img, xs, ys), img)
    assert np.array_equal(R.bilinear(img, xs + 0.5, ys)[:, :3], img[:, :3] + 0.5)
    assert np.array_equal(R.bilinear(img, xs - 9, ys + 9), np.broadcast_to(img[2, 0], (3, 4)))
    ref = T.bilinear(img[..., None], xs + 0.3, ys - 0.6)[..., 0]
    assert np.array_equal(R.bilinear(img, xs + 0.3, ys - 0.6), ref)    # the rule of _temporal_ref.bilinear
    assert np.array_equal(R.upsample(np.full((2, 2), 1.5), 4, 3), np.full((4, 3), 3.0))


# ------------------------------------------------------------------ the cases of the device tests meet their conditions
ALL_CASES = FC.stage_cases() + FC.grid_cases() + [c[:5] for c in FC.threshold_cases()]


def test_case_lists_are_the_ones_the_device_tests_need():
    assert (FC.FLOW_TW, FC.FLOW_TH) == tuple(
        int(re.search(r"#define\s+%s\s+(\d+)" % n, open(os.path.join(PKG, "csrc", "flow.hip")).read()).group(1))
        for n in ("FLOW_TW", "FLOW_TH"))
    shapes = set(FC.STAGE_SHAPES)
    assert {(2, 2), (2, 300), (300, 2), (3, 5), (42, 63)} <= shapes
    for d in (-1, 0, 1):                                 # one below, on and above each tile side, the other side odd
        assert any(h == FC.FLOW_TH + d and w % 2 for h, w in shapes) and any(w == FC.FLOW_TW + d and h % 2 for h, w in shapes)
    assert any(h % 2 and w % 2 and ((h + 1) // 2) % 2 and ((w + 1) // 2) % 2 for h, w in shapes)
    assert len(FC.stage_cases()) == len(FC.STAGE_SETS) * len(FC.STAGE_SHAPES)
    for name, p in FC.STAGE_SETS.items():
        assert p["min_side"] == 1 and p["iters"] % p["iters_per_launch"] == 0, name
    assert all(FC.STAGE_SETS[n]["iters_per_launch"] == 1 for n in ("first_sweep", "two_levels", "second_warp", "odd_sweeps"))
    launches = {n: p["iters"] // p["iters_per_launch"] for n, p in FC.STAGE_SETS.items()}
    assert launches["odd_sweeps"] % 2 == 1 and launches["one_blocked_launch"] == 1          # odd ping-pong parity per warp
    # a stage set has the levels it names wherever a side can be halved at all
    for cid, h, w, _, p in FC.stage_cases():
        assert FC.n_levels(h, w, p) == p["max_levels"], cid
    moved = {k: sorted(m[k] for m in FC.GRID_MOVES if k in m) for k in ("alpha2", "warps", "iters", "max_levels", "min_side")}
    assert moved == dict(alpha2=[1e-3, 0.1], warps=[1, 3], iters=[8, 24], max_levels=[1, 2, 8], min_side=[1, 6, 20])
    assert len(FC.grid_cases()) == 2 * 12 and {(h, w) for _, h, w, _, _ in FC.grid_cases()} == {(42, 63), (97, 130)}


@pytest.mark.parametrize("case", FC.threshold_cases(), ids=[c[0] for c in FC.threshold_cases()])
def test_threshold_cases_sit_on_the_level_rule(case):
    cid, h, w, seed, params, levels, other, other_levels = case
    assert params["min_side"] == 12
    assert FC.n_levels(h, w, params) == levels and FC.n_levels(h, w, other) == other_levels
    assert abs(levels - other_levels) == 1
    f_own, y_own = FC.reference(h, w, seed, params)
    f_other, y_other = FC.reference(h, w, seed, other)
    gap = float(np.abs(f_own - f_other).max())
    print(f"{cid}: {levels} levels against {other_levels}: max |F - F_other| = {gap:.3e}, yardsticks {y_own:.3e} {y_other:.3e}")
    # the other level count is another flow by far more than the device test's tolerance (4 x yardstick; a flow within it
    # of one statement is then at least 9 tolerances from the other): the rule decides, not the bound
    assert gap > 10 * 4.0 * max(y_own, y_other)


def test_threshold_pairs_of_the_level_rule():
    sizes = {(t["h"], t["w"]): t["levels"] for t in FC.THRESHOLDS}
    assert sizes[(24, 40)] == sizes[(23, 40)] + 1                    # 24 // 2 = 12 >= 12 gains a level, 23 // 2 = 11 does not
    assert sizes[(48, 50)] == sizes[(47, 50)] == sizes[(46, 50)] + 1  # ceil(47 / 2) = 24 keeps the third level, 23 loses it
    assert R.level_sizes(47, 50) == [(47, 50), (24, 25), (12, 13)] and R.level_sizes(46, 50) == [(46, 50), (23, 25)]


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_case_yardstick_is_positive_and_below_the_cap(case):
    cid, h, w, seed, params = case
    f64, yard = FC.reference(h, w, seed, params)
    assert f64.shape == (h, w, 2) and f64.dtype == np.float64 and np.isfinite(f64).all()
    print(f"{cid}: {FC.n_levels(h, w, params)} levels, max |F_f32ref - F_f64ref| = {yard:.3e}, max |F| = {np.abs(f64).max():.3f}")
    assert 0 < yard < FC.YARDSTICK_CAP
    assert np.abs(f64).max() > 1e3 * yard                # a real flow, far above its own rounding


def test_degenerate_frames():
    for name in FC.ZERO_FLOW:                            # exactly 0 in both number formats
        f64, f32 = FC.degenerate_reference(name)
        assert f64.dtype == np.float64 and f32.dtype == np.float32
        assert (f64 == 0).all() and (f32 == 0).all(), name
    a, b = FC.degenerate_pair("identical")
    assert b is a
    a, b = FC.degenerate_pair("constants")
    assert len(np.unique(a)) == 1 and len(np.unique(b)) == 1 and a[0, 0, 0] != b[0, 0, 0]
    a, b = FC.degenerate_pair("blocks")
    assert set(np.unique(a)) == set(np.unique(b)) == {0.0, 1.0} and np.array_equal(a[:-1, :-1], b[1:, 1:])
    h, w = FC.DEGENERATE_SHAPE
    a, b = FC.degenerate_pair("far_translation")
    assert np.array_equal(b[:, int(round(0.4 * w)):], a[:, :w - int(round(0.4 * w))])
    for name in FC.FINITE_FLOW:
        f64, f32 = FC.degenerate_reference(name)
        yard = float(np.abs(f32.astype(np.float64) - f64).max())
        print(f"{name}: max |F_f32ref - F_f64ref| = {yard:.3e}, max |F| = {np.abs(f64).max():.3f}")
        assert np.isfinite(f64).all() and 0 < yard < FC.YARDSTICK_CAP
    # the far translation does carry the warp's samples outside the frame
    f64 = FC.degenerate_reference("far_translation")[0]
    xs = np.arange(w)[None, :] + f64[..., 0]
    assert (xs > w - 1).any() or (xs < 0).any()


# ------------------------------------------------------------------ .flo files
def test_write_flo_then_read_flo_is_bit_exact(tmp_path):
    from nn import strotss_utils as SU
    rng = np.random.default_rng(0)
    flow = (rng.standard_normal((7, 9, 2)) * 5).astype(np.float32)
    flow[0, 0] = (-0.0, np.float32(1e-42))                           # a signed zero and a subnormal survive
    flow[1, 1] = (np.float32(3.4e38), np.float32(-1e-30))
    path = str(tmp_path / "a.flo")
    SU.write_flo(path, torch.from_numpy(flow))
    got = SU.read_flo(path)
    assert got.dtype == torch.float32 and tuple(got.shape) == (7, 9, 2)
    assert np.array_equal(got.numpy().view(np.uint32), flow.view(np.uint32))
    T.write_flo(tmp_path / "ref.flo", flow)                          # byte layout: that of the tests' own writer
    assert open(path, "rb").read() == open(tmp_path / "ref.flo", "rb").read()
    SU.write_flo(path, flow[:, ::2])                                 # a numpy view, not contiguous
    assert np.array_equal(SU.read_flo(path).numpy(), flow[:, ::2])
    with pytest.raises(ValueError):
        SU.write_flo(path, np.zeros((4, 4, 3), np.float32))


# ------------------------------------------------------------------ command line
def test_compute_flow_flags_parse():
    a = _args("--video", "--compute_flow", "--save_flow", "d", "-o", "out")
    assert a.video and a.compute_flow and a.save_flow == "d" and a.flow_dir is None
    a = _args()
    assert not a.compute_flow and a.save_flow is None


def test_compute_flow_wiring_and_refusals(tmp_path, monkeypatch):
    import argparse
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    T.translated_sequence(frames, flows, n_frames=3, h=12, w=16)
    empty = str(tmp_path / "nothing_here")
    # with --compute_flow no flow file is looked for, with any offsets
    got, lam = RS._video_inputs(_args("--video", "--compute_flow", content=frames))
    assert len(got) == 3 and lam == RS.DEFAULT_TEMPORAL_WEIGHT
    assert len(RS._video_inputs(_args("--video", "--compute_flow", "--temporal_frames", "1", "2", "--save_flow", empty,
                                      content=frames))[0]) == 3
    assert not os.path.exists(empty)                     # nothing is written before a frame is optimised
    for extra in (("--compute_flow",),                                    # without --video
                  ("--video", "--save_flow", empty, "--flow_dir", flows),  # --save_flow without --compute_flow
                  ("--save_flow", empty),
                  ("--video", "--compute_flow", "--flow_dir", flows)):     # both sources
        with pytest.raises(ValueError):
            RS._video_inputs(_args(*extra, content=frames))
        with pytest.raises(ValueError):                  # run() refuses before it loads anything
            RS.run(_args(*extra, "-o", str(tmp_path / "out"), content=frames))
    assert not (tmp_path / "out").exists()
    # --video with neither source: the refusal and its message as before
    with pytest.raises(ValueError, match=re.escape("--video needs --flow_dir (the optical flow between consecutive frames)")):
        RS._video_inputs(_args("--video", content=frames))
    # the other refusals of --video hold with --compute_flow
    with pytest.raises(ValueError):
        RS._video_inputs(_args("--video", "--compute_flow", "--strips", content=frames))
    with pytest.raises(ValueError):
        RS._video_inputs(_args("--video", "--compute_flow", "--temporal_weight", "-1", content=frames))
    # bare Namespaces (no such attributes) still work
    assert RS._video_inputs(argparse.Namespace(content_path="c.jpg")) is None


# ------------------------------------------------------------------ the C ABI
def test_header_and_binding_declare_the_flow_entries():
    from nn import _hip
    text = open(os.path.join(ROOT, "include", "strotss_hip.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for s in FLOW_SYMBOLS:
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert s in _hip.SIGNATURES
    m = re.search(r"typedef\s+struct\s*\{([^}]*)\}\s*strotss_flow_params_t\s*;", code)
    assert m, "strotss_flow_params_t"
    fields = [f for f in re.split(r"[;,\s]+", m.group(1)) if f and f not in ("float", "int")]
    assert fields == ["alpha2", "warps", "iters", "min_side", "max_levels", "iters_per_launch"]
    assert [f[0] for f in _hip.FlowParamsT._fields_] == fields
    assert "strotss_abi_version" in code and _hip.ABI_VERSION == 8


@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def _params(lib, **kw):
    from nn import _hip
    p = _hip.FlowParamsT()
    lib.strotss_flow_default_params(C.byref(p))
    for k, v in kw.items():
        setattr(p, k, v)
    return p


BAD_PARAMS = [dict(alpha2=0.0), dict(alpha2=-1.0), dict(alpha2=float("nan")), dict(alpha2=float("inf")), dict(warps=0),
              dict(iters=0), dict(iters_per_launch=0), dict(iters_per_launch=3), dict(iters_per_launch=16),
              dict(iters=30, iters_per_launch=8), dict(iters=4, iters_per_launch=8)]


def test_flow_defaults_and_workspace_bytes(lib):
    from nn import _ops
    p = _params(lib)
    assert (round(p.alpha2, 6), p.warps, p.iters, p.min_side, p.max_levels, p.iters_per_launch) == (0.01, 5, 32, 12, 8, 8)
    q = _ops.flow_params(iters_per_launch=1, warps=3)
    assert (q.iters_per_launch, q.warps, q.iters) == (1, 3, 32)
    with pytest.raises(ValueError):
        _ops.flow_params(sweeps=3)
    nb = lib.strotss_flow_workspace_bytes(48, 64, None)
    assert nb == lib.strotss_flow_workspace_bytes(48, 64, C.byref(p))
    # both pyramids (3 levels), u and v twice, four coefficients: at least that many floats
    assert nb >= 4 * (2 * (48 * 64 + 24 * 32 + 12 * 16) + 8 * 48 * 64)
    assert lib.strotss_flow_workspace_bytes(768, 1024, None) > lib.strotss_flow_workspace_bytes(384, 512, None) > nb
    for h, w in ((1, 64), (64, 1), (0, 0), (-3, 8)):
        assert lib.strotss_flow_workspace_bytes(h, w, None) == 0
    for bad in BAD_PARAMS:
        assert lib.strotss_flow_workspace_bytes(48, 64, C.byref(_params(lib, **bad))) == 0, bad
    assert lib.strotss_flow_workspace_bytes(48, 64, C.byref(_params(lib, iters=30, iters_per_launch=2))) == nb


@pytest.mark.parametrize("case", ALL_CASES, ids=[c[0] for c in ALL_CASES])
def test_workspace_bytes_are_what_the_levels_imply(lib, case):
    cid, h, w, seed, params = case
    want = FC.workspace_bytes(h, w, params)
    # every level adds two planes of at least 256 bytes: a level count off by one is another total, without a GPU
    assert lib.strotss_flow_workspace_bytes(h, w, C.byref(_params(lib, **params))) == want


def test_workspace_bytes_of_the_forced_level_counts(lib):
    for cid, h, w, seed, params, levels, other, other_levels in FC.threshold_cases():
        own = lib.strotss_flow_workspace_bytes(h, w, C.byref(_params(lib, **params)))
        forced = lib.strotss_flow_workspace_bytes(h, w, C.byref(_params(lib, **other)))
        assert own == FC.workspace_bytes(h, w, params) and forced == FC.workspace_bytes(h, w, other), cid
        assert (own > forced) == (levels > other_levels) and own != forced, cid


def test_optical_flow_refuses_before_launching(lib):
    big = 1 << 30

    def call(a=P, b=P, h=48, w=64, params=None, out=P, ws=P, nb=big):
        return lib.strotss_optical_flow(a, b, h, w, None if params is None else C.byref(params), out, ws, nb, None)
    assert call(a=None) == EINVAL and call(b=None) == EINVAL and call(out=None) == EINVAL and call(ws=None) == EINVAL
    assert call(h=1) == EINVAL and call(w=1) == EINVAL and call(h=0) == EINVAL and call(w=-5) == EINVAL
    for bad in BAD_PARAMS:
        assert call(params=_params(lib, **bad)) == EINVAL, bad
    need = lib.strotss_flow_workspace_bytes(48, 64, None)
    assert call(nb=need - 1) == EINVAL and call(nb=0) == EINVAL          # a too-small workspace
    assert call(a=ODD) == EALIGN and call(b=ODD) == EALIGN and call(out=ODD) == EALIGN and call(ws=ODD) == EALIGN
