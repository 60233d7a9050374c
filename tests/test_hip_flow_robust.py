"""The robust optical flow on the MI355X: one weight update and its sweeps (strotss_flow_robust_stage)
against the float32 statement bit for bit at the cases of _flow_robust_cases.py and under every solver form,
strotss_optical_flow_robust against the float64 statement within the float32 yardstick test_flow_robust_cpu.py measures,
the two-layer pair, robust = NULL against strotss_optical_flow_match bit for bit, the scratch contract and the refusals
with tests/_scratch_guard.py's guard bands, and --flow_robust end to end.  Every test prints the figures its assertions are
judged by."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _flow_ref as R  # noqa: E402
import _flow_robust_cases as RC  # noqa: E402
import _flow_robust_ref as RB  # noqa: E402
import _temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
EINVAL, EALIGN = -1, -2


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _flow(a, b, radius=0, robust={}, **params):
    from nn import _ops
    out = _ops.optical_flow(_dev(a), _dev(b), _ops.flow_params(**params) if params else None, match_radius=radius,
                            robust=robust)
    torch.cuda.synchronize()
    return out


def _same_bits(x, y):
    return torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _bits(x):
    return np.ascontiguousarray(x).view(np.int32)


# ------------------------------------------------------------------ 1. one weight update and its sweeps, bit for bit
@pytest.mark.parametrize("case", RC.stage_cases(), ids=[c[0] for c in RC.stage_cases()])
def test_stage_equals_the_float32_statement_bit_for_bit(case):
    from nn import _ops
    name, h, w, k, seed = case
    coef, u, v = RC.stage_inputs(h, w, seed)
    want = RC.stage_reference(h, w, seed)
    got = _ops.flow_robust_stage(_dev(coef), _dev(u), _dev(v), None, RC.STAGE_SWEEPS, k)
    torch.cuda.synchronize()
    uo, vo, s = (t.cpu().numpy() for t in got[:3])
    gk = got[3].cpu().numpy()
    parts = (("u", uo, want[0]), ("v", vo, want[1]), ("s", s, want[2]), ("1/G", gk[..., 0], want[3]), ("k", gk[..., 1], want[4]))
    print(f"{name}: max |device - float32 statement|: " + ", ".join(
        f"{n} {np.abs(g.astype(np.float64) - r).max():.3e}" for n, g, r in parts))
    for n, g, r in parts:
        assert g.dtype == np.float32 and r.dtype == np.float32
        assert np.array_equal(_bits(g), _bits(r)), (name, n, int((_bits(g) != _bits(r)).sum()))


# ------------------------------------------------------------------ 2. the whole flow
@pytest.mark.parametrize("h,w,seed,radius", RC.FLOW_CASES, ids=[f"{h}x{w}-R{r}" for h, w, _, r in RC.FLOW_CASES])
def test_robust_flow_against_float64_and_between_solver_forms(h, w, seed, radius):
    a, b = R.smooth_pair(h, w, seed)
    f64, yard = RC.flow_reference(h, w, seed, radius)
    got = _flow(a, b, radius)
    dist = float(np.abs(got.cpu().numpy().astype(np.float64) - f64).max())
    print(f"{h} x {w}, R = {radius}: max |F_f32ref - F_f64ref| = {yard:.3e} (CPU), max |F_hip - F_f64ref| = {dist:.3e} (GPU), "
          f"ratio {dist / yard:.2f}")
    assert 0 < yard < RC.YARDSTICK_CAP
    assert dist <= RC.F32_YARDSTICK * yard, (dist, yard)
    plain = _flow(a, b, radius, iters_per_launch=1)
    for k in (2, 4, 8):
        assert _same_bits(plain, _flow(a, b, radius, iters_per_launch=k)), k
    assert _same_bits(plain, got)
    assert not _same_bits(plain, _flow(a, b, radius, None, iters_per_launch=1))        # the robust solver is in
    assert not _same_bits(plain, _flow(a, b, radius, {"outer": 8}, iters_per_launch=1))  # and its parameters arrive
    assert not _same_bits(plain, _flow(a, b, radius, {"alpha": 0.05}, iters_per_launch=1))


# ------------------------------------------------------------------ 3. the two-layer pair on the device
@pytest.mark.parametrize("seed", RC.PAIR_SEEDS)
def test_robust_flow_keeps_the_block_on_the_device(seed):
    a, b, truth = RC.pair(seed)
    hs = RC.pair_horn_schunck_epe(seed)                # the reference: _flow_ref.optical_flow in float64
    robust = R.interior_epe(_flow(a, b).cpu().numpy(), truth)[0]
    both = R.interior_epe(_flow(a, b, RC.PAIR_RADIUS).cpu().numpy(), truth)[0]
    print(f"two-layer pair, seed {seed}, HIP: interior mean EPE robust {robust:.4f} (ratio {robust / hs:.4f} to the reference's "
          f"{hs:.4f}), robust + R = {RC.PAIR_RADIUS} {both:.4f} px")
    assert robust < RC.PAIR_FACTOR * hs
    assert both < hs


# ------------------------------------------------------------------ 4. robust = NULL is strotss_optical_flow_match
def test_null_robust_is_strotss_optical_flow_match():
    from nn import _hip, _ops
    lib = _hip.lib()
    h, w = 42, 63
    a, b = (_dev(x) for x in R.smooth_pair(h, w, h * w))
    nb = int(lib.strotss_flow_workspace_bytes(h, w, None))
    assert int(lib.strotss_flow_robust_workspace_bytes(h, w, None, None)) == nb
    st = _ops.stream_ptr()
    for r in (0, 2):
        old, new = torch.full((h, w, 2), 7.0, device=DEV), torch.full((h, w, 2), 7.0, device=DEV)
        ws = torch.full((nb,), 0x5A, dtype=torch.uint8, device=DEV)
        assert lib.strotss_optical_flow_match(_ops.ptr(a), _ops.ptr(b), h, w, None, r, _ops.ptr(old), _ops.ptr(ws), nb, st) == 0
        ws.fill_(0x5A)
        assert lib.strotss_optical_flow_robust(_ops.ptr(a), _ops.ptr(b), h, w, None, None, r, _ops.ptr(new), _ops.ptr(ws), nb,
                                               st) == 0
        torch.cuda.synchronize()
        assert _same_bits(old, new) and torch.isfinite(new).all()
        assert _same_bits(_ops.optical_flow(a, b, match_radius=r), old)
        assert _same_bits(_ops.optical_flow(a, b, match_radius=r, robust=None), old)


# ------------------------------------------------------------------ 5. scratch: inside the declared bytes, from any fill
def test_scratch_contract_and_refusals_write_nothing():
    import _scratch_guard as G
    from nn import _hip, _ops
    lib = _hip.lib()
    h, w = 42, 63
    a, b = (_dev(x) for x in R.smooth_pair(h, w, h * w))
    st = _ops.stream_ptr()
    rp = _ops.flow_robust_params({})
    for radius, params in ((0, None), (2, None), (0, _ops.flow_params(iters_per_launch=1))):
        pp = None if params is None else C.byref(params)
        nb = int(lib.strotss_flow_robust_workspace_bytes(h, w, pp, C.byref(rp)))
        assert nb > int(lib.strotss_flow_workspace_bytes(h, w, pp))
        results = []
        for zero in (False, True):                      # the quiet-NaN pattern, then zeros
            out, guard = G.guarded((h, w, 2), torch.float32, 7.0, DEV, "flow")
            blk = G.Block("robust flow workspace", nb, DEV, zero=zero)
            rc = lib.strotss_optical_flow_robust(_ops.ptr(a), _ops.ptr(b), h, w, pp, C.byref(rp), radius, _ops.ptr(out),
                                                 _ops.ptr(blk.view), nb, st)
            torch.cuda.synchronize()
            assert rc == 0
            guard.check()
            blk.check()
            assert guard.untouched() == 0 and torch.isfinite(out).all()
            assert 0 <= blk.high_water() < nb
            results.append(out.clone())
        assert _same_bits(results[0], results[1]), (radius, params is None)
        print(f"42 x 63, R = {radius}, {'default' if params is None else 'one-sweep'} form: {nb} declared bytes, guards intact, "
              f"equal bits from NaN-filled and zeroed scratch")
    # refusals: nothing launched, output and workspace as they were
    nb = int(lib.strotss_flow_robust_workspace_bytes(h, w, None, C.byref(rp)))

    def bad(**kw):
        q = _ops.flow_robust_params({})
        for key, val in kw.items():
            setattr(q, key, val)
        return q
    refused = [(bad(alpha=0.0), {}, EINVAL), (bad(alpha=float("nan")), {}, EINVAL), (bad(eps_d=-1.0), {}, EINVAL),
               (bad(eps_s=float("inf")), {}, EINVAL), (bad(outer=0), {}, EINVAL), (bad(outer=9), {}, EINVAL),
               (bad(outer=3), {}, EINVAL), (bad(outer=8), {}, EINVAL),          # 4 sweeps per update, 8 per launch
               (rp, dict(nbytes=nb - 1), EINVAL), (rp, dict(nbytes=int(lib.strotss_flow_workspace_bytes(h, w, None))), EINVAL),
               (rp, dict(radius=5), EINVAL), (rp, dict(misalign=True), EALIGN)]
    for q, kw, code in refused:
        out, guard = G.guarded((h, w, 2), torch.float32, 7.0, DEV, "flow")
        blk = G.Block("robust flow workspace", nb, DEV)
        op = _ops.ptr(out) + (4 if kw.get("misalign") else 0)
        rc = lib.strotss_optical_flow_robust(_ops.ptr(a), _ops.ptr(b), h, w, None, C.byref(q), kw.get("radius", 0), op,
                                             _ops.ptr(blk.view), kw.get("nbytes", nb), st)
        torch.cuda.synchronize()
        assert rc == code, (kw, rc)
        guard.check()
        blk.check()
        assert guard.untouched() == out.numel() and blk.high_water() == -1, kw
    with pytest.raises(ValueError):
        _ops.optical_flow(a, b, robust={"alpha": -1.0})
    with pytest.raises(_hip.StrotssHipError):
        _ops.optical_flow(a, b, robust={"outer": 8})    # valid on its own, not with 8 sweeps per launch: the library's 0 bytes


# ------------------------------------------------------------------ 6. --video --compute_flow --flow_robust end to end
def test_flow_robust_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    from nn import strotss_utils as SU
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    h, w, n = 48, 64, 3
    seq, truth = RC.two_layer_frames(h, w, n)
    frames = tmp_path / "frames"
    frames.mkdir()
    for t, f in enumerate(seq):
        Image.fromarray((f * 255).round().astype(np.uint8)).save(frames / f"frame_{t + 1:02d}.png")
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    epe = {}
    for name, extra in (("plain", ()), ("robust", ("--flow_robust",))):
        out, saved = tmp_path / name, tmp_path / (name + "_flows")
        RS.run(RS.build_parser().parse_args([str(frames), style, "--video", "--compute_flow", *extra, "--save_flow", str(saved),
                                             "--max_size", "64", "--level", "1", "--max_iter", "30", "-o", str(out)]))
        assert sorted(os.listdir(out)) == [f"frame_{t:02d}.jpg" for t in (1, 2, 3)]
        assert sorted(os.listdir(saved)) == ["backward_2_1.flo", "backward_3_2.flo", "forward_1_2.flo", "forward_2_3.flo"]
        fb = SU.read_flo(os.path.join(saved, "backward_3_2.flo")).numpy()
        assert fb.shape == (h, w, 2)
        epe[name] = R.interior_epe(fb, truth)[0]
    print(f"backward_3_2.flo, interior mean EPE: without --flow_robust {epe['plain']:.4f}, with {epe['robust']:.4f} px")
    assert epe["robust"] < epe["plain"]
