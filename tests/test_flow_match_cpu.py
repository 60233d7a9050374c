"""CPU-only: the statement of the optical flow's patch-matching stage (tests/_flow_match_ref.py) and
the conditions of the cases test_hip_flow_match.py runs on the device (tests/_flow_match_cases.py): the stage improves the
flow of a two-layer pair, keeps the translations' accuracy, its cases are decided in float64 far enough for float32 to
decide alike, the whole-flow cases' yardsticks are below the cap; the split bilinear rule is _flow_ref.bilinear; the
command line's refusals and defaults, the C ABI's refusals."""
import ctypes as C
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "strotss-tensorflow_amd")
for p in (ROOT, PKG, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import _flow_match_cases as MC  # noqa: E402
import _flow_match_ref as M  # noqa: E402
import _flow_ref as R  # noqa: E402
import _temporal_ref as T  # noqa: E402

EINVAL, EALIGN = -1, -2
P = C.c_void_p(0x10000)          # "some buffer": non-null, 16-byte aligned, never touched
ODD = C.c_void_p(0x10004)        # non-null, not 16-byte aligned


def _args(*extra, content="c.jpg"):
    import run_strotss as RS
    return RS.build_parser().parse_args([content, "s.jpg", *extra])


# ------------------------------------------------------------------ the statement
def test_radius_zero_is_the_unmatched_statement():
    a, b = R.smooth_pair(30, 41, 3)
    for dt in (np.float64, np.float32):
        assert np.array_equal(M.optical_flow(a, b, dt, 0), R.optical_flow(a, b, dt))


def test_split_sampling_is_the_bilinear_rule():
    """whole part + fraction, the taps clamped: _flow_ref.bilinear at the same point, to float64's rounding"""
    rng = np.random.default_rng(5)
    b = rng.random((13, 17))
    f = rng.uniform(-25, 25, (2, 400))
    qx, qy = rng.integers(-4, 22, 400), rng.integers(-4, 18, 400)
    (iu, fu), (iv, fv) = M.split(f[0]), M.split(f[1])
    got = M.sample(b, qx + iu, fu, qy + iv, fv)
    want = R.bilinear(b, qx + f[0], qy + f[1])
    assert np.abs(got - want).max() < 1e-13
    # a whole-numbered flow: fraction 0, the pixel itself
    assert np.array_equal(M.sample(b, *sum((M.split(np.float64([3.0])) for _ in range(2)), ())), b[3:4, 3])


def test_offsets_scan_order_and_ties():
    assert M.offsets(1) == [(-1, -1), (0, -1), (1, -1), (-1, 0), (0, 0), (1, 0), (-1, 1), (0, 1), (1, 1)]
    c = np.ones((9, 1, 3))
    c[[2, 6], 0, 1] = 0.5               # two equal minima: the first in scan order
    c[4, 0, 2] = 0.5
    c[1, 0, 2] = 0.5                    # d = 0 ties with an earlier offset: d = 0
    assert M.choose(c, 1)[0].tolist() == [4, 2, 4]
    # constant frames: every cost equal, the flow stays, bit for bit (-0.0 included)
    a, b = np.full((6, 7), 0.25), np.full((6, 7), 0.75)
    u = np.full((6, 7), -0.0)
    uo, vo, pick = M.stage(a, b, u, u + 1.5, 2)
    assert (pick == 12).all() and np.array_equal(np.signbit(uo), np.signbit(u)) and np.array_equal(vo, u + 1.5)


# ------------------------------------------------------------------ 1. the two-layer pair
@pytest.mark.parametrize("seed", MC.PAIR_SEEDS)
def test_matching_improves_the_two_layer_pair(seed):
    a, b, truth = MC.pair(seed)
    plain = MC.pair_unmatched_epe(seed)
    matched = R.interior_epe(M.optical_flow(a, b, np.float64, MC.PAIR_RADIUS), truth)[0]
    print(f"two-layer pair, seed {seed}: interior mean EPE unmatched {plain:.4f}, R = {MC.PAIR_RADIUS} {matched:.4f} px, "
          f"ratio {matched / plain:.4f}")
    assert abs(plain - {0: 0.4025, 1: 0.3593}[seed]) < 5e-4           # the pair is the one the figures were measured on
    assert matched < plain
    assert matched < MC.PAIR_FACTOR * plain


# ------------------------------------------------------------------ 2. translations keep their accuracy
@pytest.mark.parametrize("h,w,shift", R.KNOWN_MOTION, ids=[f"{h}x{w}" for h, w, _ in R.KNOWN_MOTION])
def test_matched_flow_recovers_a_translation(h, w, shift):
    prev, cur = R.translated_pair(h, w, shift)
    dx, dy = shift
    fb = M.optical_flow(cur, prev, np.float64, MC.PAIR_RADIUS)
    ff = M.optical_flow(prev, cur, np.float64, MC.PAIR_RADIUS)
    mean_b, max_b = R.interior_epe(fb, (-dx, -dy))
    mean_f, max_f = R.interior_epe(ff, (dx, dy))
    agree = R.certainty_agreement(fb, ff, shift)
    print(f"{h} x {w}, shift {shift}, R = {MC.PAIR_RADIUS}: interior EPE backward mean {mean_b:.4f} max {max_b:.3f}, forward "
          f"mean {mean_f:.4f} max {max_f:.3f}, certainty agreement {agree:.4f}")
    assert mean_b < R.MAX_INTERIOR_MEAN_EPE and mean_f < R.MAX_INTERIOR_MEAN_EPE
    assert agree >= R.MIN_AGREEMENT


# ------------------------------------------------------------------ 3. conditioning of the stage cases
@pytest.mark.parametrize("case", MC.stage_cases(), ids=[c[0] for c in MC.stage_cases()])
def test_stage_cases_are_decided_and_float32_decides_alike(case):
    name, h, w, radius, seed = case
    a, b, u, v = MC.stage_inputs(h, w, seed)
    ref = MC.stage_reference(h, w, radius, seed)
    undecided = 1.0 - ref["decided"].mean()
    moved = (ref["pick"] != M.offsets(radius).index((0, 0))).mean()
    assert max(np.abs(u).max(), np.abs(v).max()) <= MC.FLOW_AMPLITUDE
    # the float32 statement: what the kernel is the twin of, held to the device test's own assertions
    uo, vo, _ = M.stage(a, b, u, v, radius)
    assert uo.dtype == np.float32
    n_und, n_other = MC.check_stage(name, ref, radius, u, v, uo, vo)
    finite = ref["margin"][np.isfinite(ref["margin"])]
    print(f"{name}: E = {ref['e']:.3e}, undecided {n_und} of {h * w} ({100 * undecided:.2f} %), of which float32 chose "
          f"otherwise {n_other}; moved {100 * moved:.1f} %; smallest decided margin "
          f"{finite[finite > ref['e']].min() if (finite > ref['e']).any() else float('inf'):.3e}")
    assert undecided <= MC.MAX_UNDECIDED
    if h * w >= 1000:
        assert moved > 0.05, "a case must move flows (the kept ones: test_hip_flow_match.py's constant and identical frames)"


def test_cost_error_formula():
    a = np.float32([[0.5, -2.0]])
    assert M.cost_error(a, a * 0.5) == 2 * 25 * M.gamma32(8) * 2.0
    assert abs(M.gamma32(8) - 8 * 2.0 ** -24) < 1e-12


# ------------------------------------------------------------------ 4. the whole-flow cases' yardsticks
@pytest.mark.parametrize("h,w,seed", MC.FLOW_CASES, ids=[f"{h}x{w}" for h, w, _ in MC.FLOW_CASES])
def test_whole_flow_yardsticks_are_below_the_cap(h, w, seed):
    f64, yard = MC.flow_reference(h, w, seed)
    plain = R.optical_flow(*R.smooth_pair(h, w, seed))
    print(f"{h} x {w}, R = {MC.FLOW_RADIUS}: max |F_f32ref - F_f64ref| = {yard:.3e} px, max |F| = {np.abs(f64).max():.2f}, "
          f"max |F_matched - F_unmatched| = {np.abs(f64 - plain).max():.3e}")
    assert np.isfinite(f64).all() and 0 < yard < MC.YARDSTICK_CAP
    assert np.abs(f64 - plain).max() > 100 * MC.YARDSTICK_CAP, "the stage must move this case's flow"


# ------------------------------------------------------------------ 5. the command line
def test_flow_match_parser_defaults():
    assert _args().flow_match is None
    assert _args("--video", "--compute_flow", "--flow_match").flow_match == 2
    assert _args("--video", "--compute_flow", "--flow_match", "3").flow_match == 3
    import run_strotss as RS
    assert RS._flow_match_radius(_args()) == 0
    assert RS._flow_match_radius(_args("--video", "--compute_flow", "--flow_match", "4")) == 4
    import argparse
    assert RS._flow_match_radius(argparse.Namespace()) == 0


def test_flow_match_refusals(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.delenv("WORLD_SIZE", raising=False)
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    T.translated_sequence(frames, flows, n_frames=3, h=12, w=16)
    got, _ = RS._video_inputs(_args("--video", "--compute_flow", "--flow_match", content=frames))
    assert len(got) == 3
    for extra in (("--flow_match",),                                        # without --compute_flow
                  ("--video", "--flow_dir", flows, "--flow_match", "2"),    # flows that are read are not matched
                  ("--video", "--compute_flow", "--flow_match", "0"),
                  ("--video", "--compute_flow", "--flow_match", "5"),
                  ("--video", "--compute_flow", "--flow_match", "-1")):
        with pytest.raises(ValueError, match="--flow_match"):
            RS._video_inputs(_args(*extra, content=frames))
        with pytest.raises(ValueError, match="--flow_match"):               # run() refuses before it loads anything
            RS.run(_args(*extra, "-o", str(tmp_path / "out"), content=frames))
    assert not (tmp_path / "out").exists()


# ------------------------------------------------------------------ the C ABI
@pytest.fixture(scope="module")
def lib():
    from nn import _hip
    if not os.path.exists(_hip.LIB_PATH):
        import __graft_entry__ as ge
        ge.build()
    return _hip.load_library()


def test_header_and_binding_declare_the_match_entries():
    from nn import _hip
    code = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "strotss_hip.h")).read(), flags=re.S)
    for s in ("strotss_optical_flow_match", "strotss_flow_match_stage"):
        assert re.search(r"\b" + s + r"\s*\(", code), s
        assert s in _hip.SIGNATURES
    assert re.search(r"#define\s+STROTSS_FLOW_MATCH_MAX_RADIUS\s+4\b", code)
    assert len(_hip.SIGNATURES["strotss_optical_flow_match"][1]) == len(_hip.SIGNATURES["strotss_optical_flow"][1]) + 1
    assert _hip.ABI_VERSION == 8


def test_match_entries_refuse_before_any_launch(lib):
    """every refusal returns before the first launch, so it needs no GPU (and the pointers are never touched)"""
    nb = lib.strotss_flow_workspace_bytes(48, 64, None)
    flow = lambda r, **kw: lib.strotss_optical_flow_match(kw.get("a", P), P, kw.get("h", 48), 64, None, r, kw.get("out", P),
                                                          P, kw.get("nb", nb), None)          # noqa: E731
    for r in (-1, 5, 100):
        assert flow(r) == EINVAL
    for r in (0, 2):
        assert flow(r, a=None) == EINVAL and flow(r, h=1) == EINVAL and flow(r, nb=nb - 1) == EINVAL
        assert flow(r, out=ODD) == EALIGN

    def stage(r=2, h=5, w=7, ptrs=(P, P, P, P), outs=(C.c_void_p(0x20000), C.c_void_p(0x30000))):
        return lib.strotss_flow_match_stage(ptrs[0], ptrs[1], h, w, ptrs[2], ptrs[3], r, outs[0], outs[1], None)
    for r in (-1, 0, 5):
        assert stage(r=r) == EINVAL
    assert stage(h=0) == EINVAL and stage(w=0) == EINVAL and stage(h=1 << 15, w=1 << 14) == EINVAL
    for i in range(4):
        assert stage(ptrs=tuple(None if j == i else P for j in range(4))) == EINVAL
        assert stage(ptrs=tuple(ODD if j == i else P for j in range(4))) == EALIGN
    assert stage(outs=(None, P)) == EINVAL and stage(outs=(C.c_void_p(0x20000), None)) == EINVAL
    assert stage(outs=(ODD, C.c_void_p(0x30000))) == EALIGN
    assert stage(outs=(P, C.c_void_p(0x30000))) == EINVAL               # an output that is an input
    assert stage(outs=(C.c_void_p(0x20000), C.c_void_p(0x20000))) == EINVAL
