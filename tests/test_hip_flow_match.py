"""The optical flow's patch-matching stage on the MI355X: strotss_flow_match_stage element by element
against the float64 statement at the cases of _flow_match_cases.py (test_flow_match_cpu.py proves their conditions), the
ties that d = 0 wins, strotss_optical_flow_match against the float64 matched flow and under both solver forms, its
match_radius = 0 path against strotss_optical_flow bit for bit, refusals, the two-layer pair, and --flow_match end to end.
Every test prints the figures its assertions are judged by."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_match_cases as MC  # noqa: E402
import _flow_match_ref as M  # noqa: E402
import _flow_ref as R  # noqa: E402
import _temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
F32_YARDSTICK = 4.0             # test_hip_flow.py's: |F_hip - F_f64| <= 4 x max |F_f32ref - F_f64ref|
EINVAL, EALIGN = -1, -2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _flow(a, b, radius, **params):
    from nn import _ops
    out = _ops.optical_flow(_dev(a), _dev(b), _ops.flow_params(**params) if params else None, match_radius=radius)
    torch.cuda.synchronize()
    return out


def _stage(a, b, u, v, radius):
    from nn import _ops
    uo, vo = _ops.flow_match_stage(_dev(a), _dev(b), _dev(u), _dev(v), radius)
    torch.cuda.synchronize()
    return uo.cpu().numpy(), vo.cpu().numpy()


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


# ------------------------------------------------------------------ 1. the stage alone, element by element
@pytest.mark.parametrize("case", MC.stage_cases(), ids=[c[0] for c in MC.stage_cases()])
def test_stage_chooses_the_float64_offsets(case):
    name, h, w, radius, seed = case
    a, b, u, v = MC.stage_inputs(h, w, seed)
    ref = MC.stage_reference(h, w, radius, seed)
    uo, vo = _stage(a, b, u, v, radius)
    n_und, n_other = MC.check_stage(name, ref, radius, u, v, uo, vo)
    twin = M.stage(a, b, u, v, radius)                  # the float32 statement: not asserted, the kernel is meant as its twin
    print(f"{name}: {h * w - n_und} decided pixels chose the float64 offset, {n_und} undecided of which {n_other} chose another "
          f"allowed one; equal to the float32 statement bit for bit: "
          f"{np.array_equal(uo.view(np.int32), twin[0].view(np.int32)) and np.array_equal(vo.view(np.int32), twin[1].view(np.int32))}")


# ------------------------------------------------------------------ 2. d = 0 wins every tie
@pytest.mark.parametrize("radius", MC.STAGE_RADII)
def test_ties_keep_the_flow_bit_for_bit(radius):
    h, w = 37, 75
    u, v = M.smooth_flow(h, w, 77)
    const_a, const_b = np.full((h, w), 0.25, np.float32), np.full((h, w), 0.75, np.float32)
    uo, vo = _stage(const_a, const_b, u, v, radius)     # constant frames: every cost equal, whatever the flow
    assert np.array_equal(uo.view(np.int32), u.view(np.int32)) and np.array_equal(vo.view(np.int32), v.view(np.int32))
    a = R.grey(R.smooth_pair(h, w, 11)[0], np.float32)
    zero = np.zeros((h, w), np.float32)
    ta = _dev(a)
    from nn import _ops
    uo, vo = _ops.flow_match_stage(ta, ta, _dev(zero), _dev(zero), radius)   # B IS A: C(p, 0) = 0, nothing is strictly below
    torch.cuda.synchronize()
    assert not uo.cpu().numpy().any() and not vo.cpu().numpy().any()
    assert not np.signbit(uo.cpu().numpy()).any()


# ------------------------------------------------------------------ 3. the whole flow
@pytest.mark.parametrize("h,w,seed", MC.FLOW_CASES, ids=[f"{h}x{w}" for h, w, _ in MC.FLOW_CASES])
def test_matched_flow_against_float64_and_between_solver_forms(h, w, seed):
    a, b = R.smooth_pair(h, w, seed)
    f64, yard = MC.flow_reference(h, w, seed)
    got = _flow(a, b, MC.FLOW_RADIUS)
    dist = float(np.abs(got.cpu().numpy().astype(np.float64) - f64).max())
    print(f"{h} x {w}, R = {MC.FLOW_RADIUS}: max |F_f32ref - F_f64ref| = {yard:.3e} (CPU), max |F_hip - F_f64ref| = {dist:.3e} "
          f"(GPU), ratio {dist / yard:.2f}")
    assert 0 < yard < MC.YARDSTICK_CAP
    assert dist <= F32_YARDSTICK * yard, (dist, yard)
    plain = _flow(a, b, MC.FLOW_RADIUS, iters_per_launch=1)
    blocked = _flow(a, b, MC.FLOW_RADIUS, iters_per_launch=8)
    assert _same_bits(plain, blocked) and _same_bits(plain, got)
    assert not _same_bits(plain, _flow(a, b, 0, iters_per_launch=1))          # the stage is in


# ------------------------------------------------------------------ 4. the default path, reproducibility, refusals
def test_radius_zero_is_strotss_optical_flow_and_refusals_write_nothing():
    from nn import _hip, _ops
    lib = _hip.lib()
    h, w = 42, 63
    a, b = (_dev(x) for x in R.smooth_pair(h, w, h * w))
    nb = int(lib.strotss_flow_workspace_bytes(h, w, None))
    st = _ops.stream_ptr()

    def call(entry, *radius, out=None, ws=None, nbytes=nb, fa=a):
        out = torch.full((h, w, 2), 7.0, device=DEV) if out is None else out
        ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV) if ws is None else ws
        rc = entry(_ops.ptr(fa) if fa is not None else None, _ops.ptr(b), h, w, None, *radius, _ops.ptr(out), _ops.ptr(ws),
                   nbytes, st)
        torch.cuda.synchronize()
        return rc, out, ws
    rc0, old, _ = call(lib.strotss_optical_flow)
    rc1, new, _ = call(lib.strotss_optical_flow_match, 0)
    assert rc0 == 0 and rc1 == 0 and _same_bits(old, new)
    for r in (0, 2):                                    # two calls, from differently filled scratch: equal bits
        _, first, _ = call(lib.strotss_optical_flow_match, r)
        _, second, _ = call(lib.strotss_optical_flow_match, r, ws=torch.zeros(nb, dtype=torch.uint8, device=DEV))
        assert _same_bits(first, second) and torch.isfinite(first).all()
    assert _same_bits(_ops.optical_flow(a, b), old) and _same_bits(_ops.optical_flow(a, b, match_radius=0), old)
    for kw, code in ((dict(radius=-1), EINVAL), (dict(radius=5), EINVAL), (dict(radius=2, nbytes=nb - 1), EINVAL),
                     (dict(radius=2, fa=None), EINVAL)):
        radius = kw.pop("radius")
        rc, out, ws = call(lib.strotss_optical_flow_match, radius, **kw)
        assert rc == code and bool((out == 7.0).all()) and bool((ws == 0x5A).all()), (radius, kw)
    with pytest.raises(ValueError):
        _ops.optical_flow(a, b, match_radius=5)
    # the stage entry: refused calls leave both outputs untouched
    g = torch.rand(h, w, device=DEV)
    uo, vo = torch.full((h, w), 7.0, device=DEV), torch.full((h, w), 7.0, device=DEV)
    for radius in (0, 5):
        assert lib.strotss_flow_match_stage(_ops.ptr(g), _ops.ptr(g), h, w, _ops.ptr(g), _ops.ptr(g), radius, _ops.ptr(uo),
                                            _ops.ptr(vo), st) == EINVAL
    assert lib.strotss_flow_match_stage(_ops.ptr(g), _ops.ptr(g), h, w, _ops.ptr(g), _ops.ptr(g), 2, _ops.ptr(uo), _ops.ptr(uo),
                                        st) == EINVAL
    torch.cuda.synchronize()
    assert bool((uo == 7.0).all()) and bool((vo == 7.0).all())
    with pytest.raises(ValueError):
        _ops.flow_match_stage(g, g, g, g, 0)


# ------------------------------------------------------------------ 5. the two-layer pair on the device
@pytest.mark.parametrize("seed", MC.PAIR_SEEDS)
def test_matching_improves_the_two_layer_pair_on_the_device(seed):
    a, b, truth = MC.pair(seed)
    plain = R.interior_epe(_flow(a, b, 0).cpu().numpy(), truth)[0]
    matched = R.interior_epe(_flow(a, b, MC.PAIR_RADIUS).cpu().numpy(), truth)[0]
    print(f"two-layer pair, seed {seed}, HIP: interior mean EPE unmatched {plain:.4f}, R = {MC.PAIR_RADIUS} {matched:.4f} px, "
          f"ratio {matched / plain:.4f}")
    assert matched < plain
    assert matched < MC.PAIR_FACTOR * plain


# ------------------------------------------------------------------ 6. --video --compute_flow --flow_match end to end
def test_flow_match_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from nn import strotss_utils as SU
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    h, w, n = 48, 64, 3
    # the two-layer sequence: the background moves by (+1, 0) per frame and a 16 x 20 block by (-4, +2) per frame against
    # the frame, so the backward flow of frame t (against t-1) is (-1, 0) and (4, -2): the pair of section 31 at half size
    big = T.texture(h + 32, w + 32, 0)
    fg = T.texture(h + 32, w + 32, 7)[16:32, 16:36]
    frames = tmp_path / "frames"
    frames.mkdir()
    truth = None
    for t in range(n):
        f = big[16:16 + h, 16 + (n - 1 - t):16 + (n - 1 - t) + w].copy()
        r, c = 22 - 2 * (n - 1 - t), 14 + 4 * (n - 1 - t)
        f[r:r + 16, c:c + 20] = fg
        Image.fromarray((f * 255).round().astype(np.uint8)).save(frames / f"frame_{t + 1:02d}.png")
        if t == n - 1:
            truth = np.empty((h, w, 2))
            truth[...] = (-1, 0)
            truth[r:r + 16, c:c + 20] = (4, -2)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    epe = {}
    for name, extra in (("plain", ()), ("matched", ("--flow_match",))):
        out, saved = tmp_path / name, tmp_path / (name + "_flows")
        RS.run(RS.build_parser().parse_args([str(frames), style, "--video", "--compute_flow", *extra, "--save_flow", str(saved),
                                             "--max_size", "64", "--level", "1", "--max_iter", "30", "-o", str(out)]))
        assert sorted(os.listdir(out)) == [f"frame_{t:02d}.jpg" for t in (1, 2, 3)]
        assert sorted(os.listdir(saved)) == ["backward_2_1.flo", "backward_3_2.flo", "forward_1_2.flo", "forward_2_3.flo"]
        fb = SU.read_flo(os.path.join(saved, "backward_3_2.flo")).numpy()
        assert fb.shape == (h, w, 2)
        epe[name] = R.interior_epe(fb, truth)[0]
    print(f"backward_3_2.flo, interior mean EPE: without --flow_match {epe['plain']:.4f}, with {epe['matched']:.4f} px")
    assert epe["matched"] < epe["plain"]
