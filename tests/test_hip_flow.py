"""strotss_optical_flow on the MI355X: the temporally blocked solver against the plain one bit for
bit, the flow against the float64 restatement with the float32 restatement's own distance as the yardstick, accuracy on
known motion, reproducibility and refusals, and --video --compute_flow end to end.  Then the cases of _flow_cases.py
(test_flow_cpu.py proves their conditions): the stage sets, which make the flow a few operations of one or two kernels so
that no later sweep forgets an early error, at the small and tile-edge shapes; the blocked solver at those shapes; every
parameter moved from its default; the level rule on its threshold; degenerate frames.  Every test prints the figures its
assertions are judged by; the measured ones are in DESIGN.md section 14."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_cases as FC  # noqa: E402
import _flow_ref as R  # noqa: E402
import _temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
SIZES = [(48, 64), (42, 63), (257, 300), (170, 256)]       # whole tiles, odd with partial tiles, several tiles each way
F32_YARDSTICK = 4.0     # |F_hip - F_f64| <= 4 x max |F_f32ref - F_f64ref|: the kernel contracts to FMAs and the numpy
#                         float32 restatement does not (the yardstick logic of DESIGN.md section 6's trajectory test)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _flow(a, b, **params):
    from nn import _ops
    out = _ops.optical_flow(_dev(a), _dev(b), _ops.flow_params(**params) if params else None)
    torch.cuda.synchronize()
    return out


# ------------------------------------------------------------------ 1. the blocked solver is the plain one, bit for bit
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_blocked_sweeps_equal_the_plain_form_bit_for_bit(hw):
    h, w = hw
    a, b = R.smooth_pair(h, w, h * w)
    plain = _flow(a, b, iters=32, iters_per_launch=1)
    assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0.5
    for k in (8, 4, 2):
        blocked = _flow(a, b, iters=32, iters_per_launch=k)
        same = torch.equal(blocked.view(torch.int32), plain.view(torch.int32))
        if not same:
            d = (blocked - plain).abs()
            bad = torch.nonzero(d.sum(-1) > 0)
            print(f"{h} x {w}, {k} sweeps per launch: {len(bad)} pixels differ, max {float(d.max()):.3e}, first at "
                  f"{bad[:5].tolist()}")
        assert same, (hw, k)


# ------------------------------------------------------------------ 2. against float64
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_flow_matches_float64_within_the_float32_yardstick(hw):
    h, w = hw
    a, b = R.smooth_pair(h, w, h * w)
    f64 = R.optical_flow(a, b)
    f32 = R.optical_flow(a, b, np.float32)
    yard = float(np.abs(f32.astype(np.float64) - f64).max())
    got = _flow(a, b).cpu().numpy().astype(np.float64)
    dist = float(np.abs(got - f64).max())
    print(f"{h} x {w}: max |F_f32ref - F_f64ref| = {yard:.3e} (CPU), max |F_hip - F_f64ref| = {dist:.3e} (GPU), "
          f"ratio {dist / yard:.2f}, max |F| = {np.abs(f64).max():.2f}")
    assert yard > 0
    assert dist <= F32_YARDSTICK * yard, (hw, dist, yard)


# ------------------------------------------------------------------ 3. accuracy on known motion
@pytest.mark.parametrize("h,w,shift", R.KNOWN_MOTION, ids=[f"{h}x{w}" for h, w, _ in R.KNOWN_MOTION])
def test_flow_recovers_a_translation(h, w, shift):
    prev, cur = R.translated_pair(h, w, shift)
    dx, dy = shift
    fb = _flow(cur, prev).cpu().numpy()
    ff = _flow(prev, cur).cpu().numpy()
    mean_b, max_b = R.interior_epe(fb, (-dx, -dy))
    mean_f, max_f = R.interior_epe(ff, (dx, dy))
    agree = R.certainty_agreement(fb, ff, shift)
    print(f"{h} x {w}, shift {shift}: interior EPE backward mean {mean_b:.4f} max {max_b:.3f}, forward mean {mean_f:.4f} "
          f"max {max_f:.3f}, certainty agreement {agree:.4f}")
    assert mean_b < R.MAX_INTERIOR_MEAN_EPE and mean_f < R.MAX_INTERIOR_MEAN_EPE
    assert agree >= R.MIN_AGREEMENT


# ------------------------------------------------------------------ 4. reproducible; refusals write nothing
def test_two_calls_are_bitwise_equal():
    a, b = R.smooth_pair(170, 256, 3)
    first, second = _flow(a, b), _flow(a, b)
    assert torch.equal(first.view(torch.int32), second.view(torch.int32))
    other = torch.cuda.Stream()                          # on the caller's stream: another stream gives the same flow
    with torch.cuda.stream(other):
        third = _flow(a, b)
    assert torch.equal(first.view(torch.int32), third.view(torch.int32))


def test_bad_arguments_return_the_codes_and_write_nothing():
    from nn import _hip, _ops
    lib = _hip.lib()
    h, w = 48, 64
    a, b = (_dev(x) for x in R.smooth_pair(h, w, 1))
    nb = int(lib.strotss_flow_workspace_bytes(h, w, None))
    ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
    out = torch.full((h, w, 2), 7.0, device=DEV)
    st = torch.cuda.current_stream().cuda_stream

    def call(fa=a.data_ptr(), fb=b.data_ptr(), h_=h, w_=w, params=None, o=out.data_ptr(), wsp=ws.data_ptr(), n=nb):
        return lib.strotss_optical_flow(fa, fb, h_, w_, None if params is None else C.byref(params), o, wsp, n, st)
    assert call(fa=None) == -1 and call(fb=None) == -1 and call(o=None) == -1 and call(wsp=None) == -1
    assert call(h_=1) == -1 and call(w_=0) == -1
    for bad in (dict(alpha2=0.0), dict(alpha2=float("nan")), dict(warps=0), dict(iters=0), dict(iters_per_launch=3),
                dict(iters=30, iters_per_launch=8)):
        assert call(params=_ops.flow_params(**bad)) == -1, bad
    assert call(n=nb - 1) == -1
    assert call(fa=a.data_ptr() + 4) == -2 and call(o=out.data_ptr() + 4) == -2 and call(wsp=ws.data_ptr() + 4) == -2
    torch.cuda.synchronize()
    assert bool((out == 7.0).all()) and bool((ws == 0x5A).all())
    with pytest.raises(ValueError):
        _ops.optical_flow(a, b[:24])
    assert call() == 0                                   # and the same call with good arguments runs
    torch.cuda.synchronize()
    assert bool(torch.isfinite(out).all()) and not bool((out == 7.0).all())


# ------------------------------------------------------------------ 5. stage by stage, parameter by parameter
def _against_float64(cid, got, f64, yard):
    """print the figures and assert |F_hip - F_f64| <= F32_YARDSTICK x yardstick"""
    err = np.abs(got.astype(np.float64) - f64)
    dist = float(err.max())
    y, x, k = np.unravel_index(int(err.argmax()), err.shape)
    print(f"{cid}: yardstick max |F_f32ref - F_f64ref| = {yard:.3e}, max |F_hip - F_f64ref| = {dist:.3e} at (y {y}, x {x}, "
          f"{'uv'[k]}), ratio {dist / yard:.2f}, max |F| = {np.abs(f64).max():.3f}")
    assert np.isfinite(got).all(), cid
    assert dist <= F32_YARDSTICK * yard, (cid, dist, yard)
    return dist


@pytest.mark.parametrize("case", FC.stage_cases(), ids=[c[0] for c in FC.stage_cases()])
def test_stage_sets_match_float64(case):
    cid, h, w, seed, params = case
    a, b = FC.frames(h, w, seed)
    f64, yard = FC.reference(h, w, seed, params)
    _against_float64(cid, _flow(a, b, **params).cpu().numpy(), f64, yard)


@pytest.mark.parametrize("hw", FC.STAGE_SHAPES, ids=[f"{h}x{w}" for h, w in FC.STAGE_SHAPES])
def test_blocked_sweeps_equal_the_plain_form_at_small_and_tile_edge_shapes(hw):
    h, w = hw
    a, b = FC.frames(h, w, 1000 + 7 * h + w)
    for iters in (8, 24):                                # K = 8: 1 and 3 launches per warp, odd ping-pong parities
        plain = _flow(a, b, iters=iters, iters_per_launch=1)
        assert torch.isfinite(plain).all() and float(plain.abs().max()) > 0
        for k in (8, 4, 2):
            blocked = _flow(a, b, iters=iters, iters_per_launch=k)
            d = (blocked - plain).abs()
            bad = torch.nonzero(d.sum(-1) > 0)
            print(f"{h} x {w}, {iters} sweeps, {k} per launch ({iters // k} launches per warp): {len(bad)} pixels differ, "
                  f"max {float(d.max()):.3e}, first at {bad[:5].tolist()}")
            assert torch.equal(blocked.view(torch.int32), plain.view(torch.int32)), (hw, iters, k)


@pytest.mark.parametrize("case", FC.grid_cases(), ids=[c[0] for c in FC.grid_cases()])
def test_every_parameter_moved_matches_float64(case):
    cid, h, w, seed, params = case
    a, b = FC.frames(h, w, seed)
    f64, yard = FC.reference(h, w, seed, params)
    _against_float64(cid, _flow(a, b, **params).cpu().numpy(), f64, yard)


@pytest.mark.parametrize("case", FC.threshold_cases(), ids=[c[0] for c in FC.threshold_cases()])
def test_level_rule_on_its_threshold(case):
    cid, h, w, seed, params, levels, other, other_levels = case
    a, b = FC.frames(h, w, seed)
    f64, yard = FC.reference(h, w, seed, params)
    g64, yard_other = FC.reference(h, w, seed, other)
    own = _flow(a, b, **params).cpu().numpy()
    forced = _flow(a, b, **other).cpu().numpy()
    _against_float64(f"{cid}, {levels} levels", own, f64, yard)
    _against_float64(f"{cid} forced to {other_levels} levels", forced, g64, yard_other)
    gap = float(np.abs(own.astype(np.float64) - forced).max())
    print(f"{cid}: max |F_hip - F_hip forced to {other_levels} levels| = {gap:.3e}")
    assert gap > F32_YARDSTICK * max(yard, yard_other)    # the level rule, not the tolerance, decides


@pytest.mark.parametrize("name", FC.ZERO_FLOW)
def test_identical_and_constant_frames_give_exactly_zero(name):
    a, b = FC.degenerate_pair(name)
    for k in (1, 8):                                     # both solver forms; == 0, so that -0.0 passes
        got = _flow(a, b, iters_per_launch=k)
        nonzero = int((got != 0).sum())
        print(f"{name}, {k} sweeps per launch: {nonzero} non-zero values, max |F| = {float(got.abs().max()):.3e}")
        assert bool((got == 0).all()), (name, k)


@pytest.mark.parametrize("name", FC.FINITE_FLOW)
def test_block_frames_and_a_far_translation_match_float64(name):
    a, b = FC.degenerate_pair(name)
    f64, f32 = FC.degenerate_reference(name)
    yard = float(np.abs(f32.astype(np.float64) - f64).max())
    _against_float64(name, _flow(a, b).cpu().numpy(), f64, yard)


# ------------------------------------------------------------------ 6. --video --compute_flow end to end
H, W, SHIFT = 48, 64, (3, 2)
CONSISTENCY_RATIO = 0.3         # E(default lambda) < ratio * E(0), the criterion of test_video_end_to_end


def _video_run(tmp_path, frames, style, name, *extra):
    import run_strotss as RS
    out = tmp_path / name
    base = [frames, style, "--video", "--max_size", "64", "--level", "1", "--max_iter", "30", "-o", str(out)]
    RS.run(RS.build_parser().parse_args(base + list(extra)))
    return out


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def _style(tmp_path):
    from PIL import Image
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    return style


def test_compute_flow_end_to_end(tmp_path, monkeypatch):
    from nn import strotss_utils as SU
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, exact = str(tmp_path / "frames"), str(tmp_path / "exact_flows")
    paths = T.translated_sequence(frames, exact, n_frames=3, h=H, w=W, shift=SHIFT)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    style = _style(tmp_path)
    saved = str(tmp_path / "saved_flows")
    computed = _video_run(tmp_path, frames, style, "computed", "--compute_flow", "--save_flow", saved)
    assert sorted(os.listdir(computed)) == sorted(s + ".jpg" for s in stems)
    assert sorted(os.listdir(saved)) == ["backward_2_1.flo", "backward_3_2.flo", "forward_1_2.flo", "forward_2_3.flo"]
    # (a) the saved flows read back are the same floats: the same JPEG bytes
    reread = _video_run(tmp_path, frames, style, "reread", "--flow_dir", saved)
    for s in stems:
        assert open(computed / f"{s}.jpg", "rb").read() == open(reread / f"{s}.jpg", "rb").read(), s
    dx, dy = SHIFT
    fb = SU.read_flo(os.path.join(saved, "backward_3_2.flo")).numpy()
    ff = SU.read_flo(os.path.join(saved, "forward_2_3.flo")).numpy()
    print(f"saved flows of frame 3: interior EPE backward mean {R.interior_epe(fb, (-dx, -dy))[0]:.4f}, forward mean "
          f"{R.interior_epe(ff, (dx, dy))[0]:.4f}, certainty agreement {R.certainty_agreement(fb, ff, SHIFT):.4f}")
    # (b) the term does its job with computed flows: the consistency error along the EXACT flows
    zero = _video_run(tmp_path, frames, style, "zero", "--compute_flow", "--temporal_weight", "0")
    with_exact = _video_run(tmp_path, frames, style, "exact", "--flow_dir", exact)
    efb = np.broadcast_to(-np.float32(SHIFT), (H, W, 2))
    eff = np.broadcast_to(np.float32(SHIFT), (H, W, 2))
    e0, e1, ex = (T.consistency_error([_read(d / f"{s}.jpg") for s in stems], efb, eff) for d in (zero, computed, with_exact))
    print(f"consistency error along the exact flows: lambda 0 {e0:.6f}, computed flows {e1:.6f} (ratio {e1 / e0:.4f}), "
          f"exact flows {ex:.6f} (ratio {ex / e0:.4f}); E_computed / E_exact_flows = {e1 / ex:.3f}")
    assert e1 < CONSISTENCY_RATIO * e0, (e0, e1, ex)
    # the first frame has no earlier one: the same bytes with and without the term
    assert open(zero / f"{stems[0]}.jpg", "rb").read() == open(computed / f"{stems[0]}.jpg", "rb").read()


def test_compute_flow_feeds_the_long_term_path(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames = str(tmp_path / "frames")
    paths = T.translated_sequence(frames, str(tmp_path / "unused"), n_frames=4, h=H, w=W, shift=SHIFT)
    saved = str(tmp_path / "saved")
    out = _video_run(tmp_path, frames, _style(tmp_path), "long", "--compute_flow", "--temporal_frames", "1", "2",
                     "--save_flow", saved)
    assert sorted(os.listdir(out)) == sorted(os.path.splitext(os.path.basename(p))[0] + ".jpg" for p in paths)
    assert sorted(os.listdir(saved)) == sorted(
        [f"backward_{t}_{t - 1}.flo" for t in (2, 3, 4)] + [f"forward_{t - 1}_{t}.flo" for t in (2, 3, 4)]
        + [f"backward_{t}_{t - 2}.flo" for t in (3, 4)] + [f"forward_{t - 2}_{t}.flo" for t in (3, 4)])
    from nn import strotss_utils as SU
    fb2 = SU.read_flo(os.path.join(saved, "backward_4_2.flo")).numpy()           # two frames back: twice the shift
    truth = (-2 * SHIFT[0], -2 * SHIFT[1])
    mean2 = R.interior_epe(fb2, truth)[0]
    f4, f2 = (_read(paths[t - 1]).astype(np.float32) for t in (4, 2))
    ref2 = R.interior_epe(R.optical_flow(f4, f2), truth)[0]
    print(f"backward_4_2.flo: interior mean EPE {mean2:.4f} against (-6, -4); the float64 restatement on these frames {ref2:.4f}")
    # the computed j = 2 flow is the restatement's flow of frames 4 and 2 (float32 differences are ~1e-4 px, test 2)
    assert abs(mean2 - ref2) < 0.01
