"""Temporal consistency on the MI355X: strotss_flow_warp against the float64 warp and certainty, strotss_temporal_fwd_bwd
against float64 (gscale 0 / certainty 0: the gradient bit for bit untouched), the engine's step with the term against the
oracle composed in float64, lambda = 0 against an engine without the term (bit for bit), graph / eager / host-draw equality
in deterministic mode, and --video end to end on a translated texture: lambda = 0 is the single-image run of every frame,
the default lambda lowers the consistency error."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import strotss_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 2179


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------ 1. the warp and its certainty
@pytest.mark.parametrize("with_forward", [False, True])
@pytest.mark.parametrize("hw", [(40, 56), (33, 71)])
def test_flow_warp_matches_float64(with_forward, hw):
    from nn import _ops
    h, w = hw
    # the inputs of _temporal_ref.random_warp_case: test_temporal_cpu.py proves that every threshold test of theirs is a
    # margin away from equality, so the array_equal below does not hang on how the device contracts its float64 to FMAs
    prev, fb, ff = T.random_warp_case(h, w, with_forward)
    warped, cert = _ops.flow_warp(_dev(prev)[None], _dev(fb), None if ff is None else _dev(ff))
    torch.cuda.synchronize()
    ref_w, ref_c = T.warp64(prev, fb), T.certainty64(fb, ff)
    assert float(np.abs(warped[0].cpu().numpy() - ref_w).max()) < 2e-6
    got_c = cert.cpu().numpy()
    assert np.array_equal(got_c, ref_c.astype(np.float32))
    assert 0.2 * h * w < got_c.sum() < h * w            # both kinds of pixels are present
    if with_forward:                                    # the band with the wrong forward flow: disoccluded pixels
        assert got_c.sum() < T.certainty64(fb).sum()


@pytest.mark.parametrize("shift", [(3, 2), (-5, 0), (0, -7), (1, 1)])
def test_flow_warp_integer_shifts_are_exact(shift):
    from nn import _ops
    h, w = 48, 64
    prev = np.random.default_rng(3).random((h, w, 3)).astype(np.float32)
    fb = np.broadcast_to(np.float32(shift), (h, w, 2))
    ff = np.broadcast_to(-np.float32(shift), (h, w, 2))
    for f in (None, ff):
        warped, cert = _ops.flow_warp(_dev(prev)[None], _dev(fb), None if f is None else _dev(f))
        torch.cuda.synchronize()
        assert np.array_equal(warped[0].cpu().numpy(), T.warp64(prev, fb).astype(np.float32))
        assert np.array_equal(cert.cpu().numpy(), T.certainty64(fb, f).astype(np.float32))
        dx, dy = shift
        assert cert.sum().item() == (w - abs(dx)) * (h - abs(dy))


@pytest.mark.parametrize("hw", T.WARP_SHAPES, ids=[f"{h}x{w}" for h, w in T.WARP_SHAPES])
def test_flow_warp_shapes_channels_borders_and_non_finite_flows(hw):
    """The cases of _temporal_ref.warp_cases (test_temporal_cpu.py proves their conditions) with 1, 3 and 4 channels, with
    and without the forward flow: warped finite everywhere (the rule of DESIGN.md section 12 for out-of-range, infinite and
    NaN coordinates), within 2e-6 of the float64 warp and equal to it for whole-pixel shifts; the certainty equal bit for bit."""
    from nn import _ops
    h, w = hw
    prevs = {c: T.warp_prev(h, w, c) for c in T.WARP_CHANNELS}
    worst, checked = 0.0, 0
    for name, fb, ff in T.warp_cases(h, w):
        ref_w = {c: T.warp64(prevs[c], fb) for c in T.WARP_CHANNELS}
        for f in (None, ff):
            ref_c = T.certainty64(fb, f).astype(np.float32)
            for c in T.WARP_CHANNELS:
                warped, cert = _ops.flow_warp(_dev(prevs[c])[None], _dev(fb), None if f is None else _dev(f))
                torch.cuda.synchronize()
                got_w, got_c = warped[0].cpu().numpy(), cert.cpu().numpy()
                assert got_w.shape == (h, w, c) and np.isfinite(got_w).all(), (name, c)
                err = float(np.abs(got_w - ref_w[c]).max())
                worst = max(worst, err)
                assert err < 2e-6, (name, c, err)
                if name.startswith("whole") or name == "far":
                    assert np.array_equal(got_w, ref_w[c].astype(np.float32)), (name, c)
                wrong = np.argwhere(got_c.view(np.uint32) != ref_c.view(np.uint32))
                assert len(wrong) == 0, (name, c, f is not None, wrong[:5].tolist())
                checked += 1
        print(f"{h} x {w} {name}: certain pixels {int(T.certainty64(fb).sum())} without / {int(T.certainty64(fb, ff).sum())} "
              f"with the forward flow of {h * w}")
    print(f"{h} x {w}: {checked} calls, max |warped - warp64| = {worst:.3e}")


# ------------------------------------------------------------------ 2. the term of one step
BIG = (513, 513)        # 263169 pixels: 257 full workgroups and one of a single pixel -- 258 partial sums, so the last
                        # workgroup's loop over them (256 per trip) makes a second trip, for partials 256 and 257


@pytest.mark.parametrize("hw", [(64, 64), (42, 63), (257, 300), (1, 3), BIG])
def test_temporal_fwd_bwd_matches_float64(hw):
    from nn import _ops
    h, w = hw
    rng = np.random.default_rng(h + w)
    x, tgt = rng.random((h, w, 3)), rng.random((h, w, 3))
    c = rng.random((h, w))
    c[rng.random((h, w)) < 0.3] = 0.0
    if hw == BIG:       # the last pixel (the last partial's only one): full certainty and the image's largest difference
        x[-1, -1], tgt[-1, -1], c[-1, -1] = 1.0, 0.0, 1.0
    g0 = rng.standard_normal((h, w, 3)).astype(np.float32) * 1e-3
    lam = 3.5
    g = _dev(g0)
    loss = torch.zeros(1, device=DEV)
    xd, td, cd = _dev(x), _dev(tgt), _dev(c)
    _ops.temporal_fwd_bwd(xd, td, cd, lam, g, loss)
    torch.cuda.synchronize()
    ref_l, ref_g = T.temporal_loss64(xd.cpu().double().numpy(), td.cpu().double().numpy(), cd.cpu().double().numpy())
    ref_g = g0.astype(np.float64) + lam * ref_g
    assert abs(loss.item() - ref_l) <= 1e-5 * abs(ref_l)
    if hw == BIG:       # on the host, from the float64 reference: without that pixel's term the loss FAILS the bound, so a
        dropped = ref_l - 1.0 * 3.0 / (3 * h * w)                   # dropped last partial cannot hide inside 1e-5
        assert -(-h * w // 1024) == 258
        assert abs(loss.item() - dropped) > 1e-5 * abs(dropped), (loss.item(), dropped)
    got = g.cpu().double().numpy()
    assert float(np.abs(got - ref_g).max()) <= 1e-5 * float(np.abs(ref_g).max())
    assert np.array_equal(got[c == 0], g0[c == 0].astype(np.float64))        # no certainty: untouched
    # gscale 0 and certainty 0: the gradient bit for bit, the loss still computed
    for lam_, cc in ((0.0, cd), (lam, torch.zeros_like(cd))):
        g = _dev(g0)
        g[0, 0, 0] = -0.0
        before = g.clone()
        _ops.temporal_fwd_bwd(xd, td, cc, lam_, g, loss)
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.int32), before.view(torch.int32))
    assert loss.item() == 0.0
    # repeated calls: the same bits (fixed-order reduction; the workspace's ticket returns to 0)
    outs = []
    for _ in range(3):
        _ops.temporal_fwd_bwd(xd, td, cd, lam, _dev(g0), loss)
        outs.append(loss.clone())
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0], o) for o in outs)


# ------------------------------------------------------------------ 3. the engine's step against the oracle (float64)
def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def _temporal_inputs(h, w, seed=9):
    rng = np.random.default_rng(seed)
    tgt = _img(h, w, 50 + seed)[0]
    cert = (rng.random((h, w)) > 0.25).astype(np.float32)
    cert[:, : w // 5] = 0.0
    return tgt, torch.from_numpy(cert)


def _engine_case(h, w, regions=1, blend=False, cw=False, n=1024, seed=0, lam=40.0, oracle=True, temporal=True):
    from nn import _ops, engine
    from nn.model import VGGParams, synthetic_weights
    wts = synthetic_weights('16', 0)
    content = _img(h, w, 1)
    styles = [_img(56, 60, 2)] + ([_img(40, 72, 3)] if blend else [])
    weights = [0.6, 0.4] if blend else [1.0]
    rng = np.random.default_rng(seed)
    alpha = 8.0
    denom = 2.0 + alpha + 1.0 / alpha
    vgg = O.VGG(wts, dtype=torch.float64)
    params = VGGParams(wts, '16', None, DEV)
    with torch.no_grad():
        cf = [content.double()] + vgg(content.double())
    s_samples, targets = [], []
    for s in styles:
        with torch.no_grad():
            sf = [s.double()] + vgg(s.double())
        s_idx = O.make_indices(s.shape[1], s.shape[2], False, n, rng)
        with torch.no_grad():
            s_samples.append(O.sample_features(sf, s_idx, False))
        feats = _ops.hypercol_gather(engine.extract_features(params, s.to(DEV)), torch.from_numpy(s_idx).to(DEV), False)
        targets.append(engine.StyleTarget.build(feats, s_idx.shape[0], D))
    masks = [None]
    if regions == 2:
        m0 = np.zeros((h, w), dtype=bool)
        m0[:, : w // 2] = True
        masks = [m0, ~m0]
    idx = [O.make_indices(h, w, True, n, rng, None if m is None else m.astype(np.float32)) for m in masks]
    init = O.make_laplacian(content.double()) + sum(wk * s.double().mean(dim=(1, 2), keepdim=True)
                                                    for wk, s in zip(weights, styles))
    if blend:
        st = [engine.StyleBlend(targets, weights)]
    else:
        st = [targets[0]] * len(masks)
        s_samples = s_samples * len(masks)
    wmap = None
    if cw:
        wmap = torch.from_numpy(np.tile(np.linspace(0.0, 1.2, w, dtype=np.float32), (h, 1)))
    tgt, cert = _temporal_inputs(h, w)
    tt = engine.TemporalTarget(tgt.to(DEV), cert.to(DEV), lam) if temporal else None
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), st, init.float().to(DEV), alpha, denom,
                            2e-3, sample_size=n, content_weight=None if wmap is None else wmap.to(DEV), temporal=tt)
    idx_dev = [torch.from_numpy(i).to(DEV) for i in idx]
    if not oracle:
        return eng, idx_dev, None
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_sum = 0.0
    for r, ix in enumerate(idx):
        c_feat = O.sample_features(cf, ix, True)
        p_feat = O.sample_features(pred, ix, True)
        if cw:
            cj = O.sample_features([wmap.double()[None, :, :, None]], ix, True)[:, 0]
            dz = [O.cosine_distance(z, z) for z in (p_feat, c_feat)]
            a_, b_ = (d_ / torch.clamp(d_.sum(dim=0), min=1e-12) for d_ in dz)
            lc = (cj[None, :] * (a_ - b_).abs()).sum() / p_feat.shape[0]
        else:
            lc = O.self_similarity(p_feat, c_feat)
        ls = (sum(wk * O.style_loss(s, p_feat, alpha) for wk, s in zip(weights, s_samples)) if blend
              else O.style_loss(s_samples[r], p_feat, alpha))
        loss = loss + (alpha * lc + ls) / denom
        lc_sum = lc_sum + lc
    loss = loss / len(idx)
    lt = (cert.double()[None, :, :, None] * (img - tgt.double()[None]) ** 2).sum() / (3 * h * w)
    total = loss + lam * lt
    grads = torch.autograd.grad(total, variables)
    return eng, idx_dev, dict(loss=float(total), loss_c=float(lc_sum) / len(idx), loss_t=float(lt), grads=grads)


@pytest.mark.parametrize("case", [dict(h=64, w=64), dict(h=42, w=64), dict(h=64, w=64, regions=2),
                                  dict(h=48, w=64, blend=True, cw=True)], ids=["64x64", "42x64", "2-regions", "blend-K2-cw"])
def test_engine_temporal_step_matches_the_oracle(case):
    eng, idx, ref = _engine_case(**case)
    eng.forward_backward(idx)
    torch.cuda.synchronize()
    got = eng.losses()
    for key in ("loss", "loss_c", "loss_t"):
        assert abs(got[key] - ref[key]) < 5e-5 * max(1.0, abs(ref[key])), (key, got[key], ref[key])
    g0, r0 = eng.gvars[0].cpu().double(), ref["grads"][0]
    assert float((g0 - r0).norm() / r0.norm()) < 2e-3
    # the term is a real part of the step: lambda * L_t is a sizeable share of the loss
    assert 40.0 * ref["loss_t"] > 0.05 * ref["loss"]


@pytest.mark.parametrize("graph", [False, True])
def test_lambda_zero_is_the_step_without_the_term(graph, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    a, idx, _ = _engine_case(64, 64, lam=0.0, oracle=False)
    b, _, _ = _engine_case(64, 64, oracle=False, temporal=False)
    if graph:
        a.capture_graph(idx)
        b.capture_graph(idx)
    for _ in range(3):
        a.step(idx)
        b.step(idx)
    torch.cuda.synchronize()
    la, lb = a.losses(), b.losses()
    assert la["loss_t"] > 0 and "loss_t" not in lb
    assert {k: v for k, v in la.items() if k != "loss_t"} == lb
    for x, y in zip(a.variables + a.gvars, b.variables + b.gvars):
        assert torch.equal(x, y)


@pytest.mark.parametrize("regions", [1, 2])
def test_temporal_step_graph_eager_and_host_draw_agree(regions, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    from nn import rand
    from nn import strotss_utils as SU
    h, w, n, seed, steps = 64, 64, 1024, 17, 3
    masks = [None]
    if regions == 2:
        m0 = np.zeros((h, w), dtype=bool)
        m0[:, : w // 2] = True
        masks = [m0, ~m0]

    def make():
        return _engine_case(h, w, regions=regions, cw=True, oracle=False)[0]
    graph, eager, host = make(), make(), make()
    assert graph.deterministic and graph.enable_device_draw(seed, 0, masks) and eager.enable_device_draw(seed, 0, masks)
    graph.capture_graph()
    rng = rand.PhiloxStream(seed, 0)
    for _ in range(steps):
        graph.step()
        eager.step()
        host.step([torch.from_numpy(SU.make_indices_np(h, w, True, n, rng, m)).to(DEV) for m in masks])
    torch.cuda.synchronize()
    assert graph.losses() == eager.losses() == host.losses()
    for a, b, c in zip(graph.variables, eager.variables, host.variables):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_engine_refuses_bad_targets_and_sharding():
    from nn import engine
    eng, _, _ = _engine_case(64, 64, n=256, oracle=False, temporal=False)
    args = (eng.params, eng.content_feat, eng.style_targets, eng.stylized(), 8.0, 10.0, 2e-3)
    tgt, cert = _temporal_inputs(64, 64)
    for bad in (engine.TemporalTarget(tgt[:32], cert, 1.0), engine.TemporalTarget(tgt, cert[:, :10], 1.0),
                engine.TemporalTarget(tgt, cert, -1.0), engine.TemporalTarget(tgt, cert, float("nan"))):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=256, temporal=bad)
    with pytest.raises(ValueError):
        engine.StepEngine(*args, sample_size=256, temporal=engine.TemporalTarget(tgt, cert, 1.0), dist_group=object())


def test_temporal_target_at_scale_is_the_bilinear_resize():
    from nn import _ops
    from nn import strotss_utils as SU
    h, w = 48, 64
    warped = _dev(np.random.default_rng(0).random((1, h, w, 3)))
    cert = _dev((np.random.default_rng(1).random((h, w)) > 0.5))
    t, c = SU.temporal_target_at_scale(warped, cert, 24, 32)
    assert tuple(t.shape) == (24, 32, 3) and tuple(c.shape) == (24, 32)
    assert torch.equal(t, _ops.resize_bilinear(warped[0].contiguous(), 24, 32))
    assert torch.equal(c, _ops.resize_bilinear(cert[:, :, None].contiguous(), 24, 32)[..., 0])
    t, c = SU.temporal_target_at_scale(warped, cert, h, w)
    assert torch.equal(t, warped[0]) and torch.equal(c, cert)
    # the flow resize on the device: a constant field keeps its value, scaled
    fl = _dev(np.broadcast_to(np.float32([2.0, -1.0]), (h, w, 2)))
    r = SU.resize_flow(fl, 24, 48)
    assert torch.allclose(r[..., 0], torch.full((24, 48), 1.5, device=DEV))
    assert torch.allclose(r[..., 1], torch.full((24, 48), -0.5, device=DEV))


def test_temporal_for_frame_reads_the_flow_files(tmp_path):
    import run_strotss as RS
    from PIL import Image
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    T.translated_sequence(frames, flows, n_frames=2, h=48, w=64, shift=(3, 2))
    args = RS._resolve(RS.build_parser().parse_args([frames, "s.jpg", "--video", "--flow_dir", flows]))
    for h, w in ((48, 64), (24, 32)):                   # at the frames' size, and at half of it: the flows scaled by 0.5
        prev = np.random.default_rng(h).random((h, w, 3)).astype(np.float32)
        warped, cert = RS._flow_warp_for_frame(args, 2, _dev(prev)[None])[1:]
        torch.cuda.synchronize()
        k = h / 48
        fb = np.broadcast_to(np.float32([-3 * k, -2 * k]), (h, w, 2))
        ff = np.broadcast_to(np.float32([3 * k, 2 * k]), (h, w, 2))
        assert float(np.abs(warped[0].cpu().numpy() - T.warp64(prev, fb)).max()) < 2e-6
        assert np.array_equal(cert.cpu().numpy(), T.certainty64(fb, ff).astype(np.float32))
    # reliable_2_1.pgm replaces the certainty: its value / 255
    Image.fromarray(np.full((48, 64), 128, dtype=np.uint8)).save(os.path.join(flows, "reliable_2_1.pgm"))
    _, cert = RS._flow_warp_for_frame(args, 2, _dev(prev)[None])[1:]
    assert tuple(cert.shape) == (24, 32) and torch.allclose(cert, torch.full_like(cert, 128 / 255))


# ------------------------------------------------------------------ 4. --video end to end
H, W, SHIFT = 48, 64, (3, 2)
CONSISTENCY_RATIO = 0.3         # E(default lambda) < ratio * E(0): measured 0.094


def _video_run(tmp_path, frames, flows, style, name, *extra):
    import run_strotss as RS
    out = tmp_path / name
    base = [frames, style, "--video", "--flow_dir", flows, "--max_size", "64", "--level", "1", "--max_iter", "30",
            "-o", str(out)]
    RS.run(RS.build_parser().parse_args(base + list(extra)))
    return out


def _read(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.float64) / 255.0


def test_video_end_to_end(tmp_path, monkeypatch):
    import run_strotss as RS
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    paths = T.translated_sequence(frames, flows, n_frames=3, h=H, w=W, shift=SHIFT)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    zero = _video_run(tmp_path, frames, flows, style, "zero", "--temporal_weight", "0")
    dflt = _video_run(tmp_path, frames, flows, style, "default")
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    assert sorted(os.listdir(zero)) == sorted(os.listdir(dflt)) == sorted(s + ".jpg" for s in stems)
    # lambda = 0: every frame is the independent single-image run of that frame, byte for byte
    for p, s in zip(paths, stems):
        single = tmp_path / f"single_{s}.jpg"
        RS.run(RS.build_parser().parse_args([p, style, "--max_size", "64", "--level", "1", "--max_iter", "30",
                                             "-o", str(single)]))
        assert open(single, "rb").read() == open(zero / f"{s}.jpg", "rb").read(), s
    # the default lambda: a lower consistency error along the exact flow
    fb = np.broadcast_to(-np.float32(SHIFT), (H, W, 2))
    ff = np.broadcast_to(np.float32(SHIFT), (H, W, 2))
    e0 = T.consistency_error([_read(zero / f"{s}.jpg") for s in stems], fb, ff)
    e1 = T.consistency_error([_read(dflt / f"{s}.jpg") for s in stems], fb, ff)
    print(f"consistency error: lambda 0 {e0:.6f}, default lambda {RS.DEFAULT_TEMPORAL_WEIGHT:g} {e1:.6f}")
    assert e1 < CONSISTENCY_RATIO * e0, (e0, e1)
    # the first frame has no previous one: the same bytes either way
    assert open(zero / f"{stems[0]}.jpg", "rb").read() == open(dflt / f"{stems[0]}.jpg", "rb").read()
    # --temporal_init runs, too
    init = _video_run(tmp_path, frames, flows, style, "init", "--temporal_init")
    e2 = T.consistency_error([_read(init / f"{s}.jpg") for s in stems], fb, ff)
    print(f"consistency error with --temporal_init: {e2:.6f}")
    assert np.isfinite(e2)
