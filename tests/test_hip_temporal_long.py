"""Long-term temporal consistency on the MI355X: strotss_temporal_long_certainty bit for bit against
the float32 restatement, strotss_temporal_multi_fwd_bwd against float64 (count 1: strotss_temporal_fwd_bwd bit for bit;
zero weights or certainties: the gradient bit for bit untouched), the engine's step with three targets against the oracle
composed in float64, a one-element list against the TemporalTarget engine bit for bit, graph / eager / host-draw equality
in deterministic mode, and --temporal_frames end to end on an occluder crossing a static background."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import strotss_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _temporal_long_ref as TL  # noqa: E402
import _temporal_ref as T  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 2179


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


# ------------------------------------------------------------------ 1. the combined certainties
@pytest.mark.parametrize("hw", [(64, 64), (42, 63), (257, 300)])
@pytest.mark.parametrize("count", [1, 2, 3, 4])
@pytest.mark.parametrize("kind", ["binary", "fractional"])
def test_long_certainty_matches_the_float32_restatement(hw, count, kind):
    from nn import _ops
    h, w = hw
    rng = np.random.default_rng(h * w + count)
    st = rng.random((count, h, w)).astype(np.float32)
    if kind == "binary":
        st = (st > 0.4).astype(np.float32)
    else:
        st[rng.random(st.shape) < 0.2] = 0.0
        st[rng.random(st.shape) < 0.1] = 1.0
    got = _ops.temporal_long_certainty(_dev(st))
    torch.cuda.synchronize()
    want = TL.long_certainty32(st)
    assert np.array_equal(got.cpu().numpy().view(np.int32), want.view(np.int32))
    # in place, as the header allows
    x = _dev(st)
    _ops.temporal_long_certainty(x, out=x)
    torch.cuda.synchronize()
    assert np.array_equal(x.cpu().numpy().view(np.int32), want.view(np.int32))


# ------------------------------------------------------------------ 2. the terms of one step
def _multi_inputs(h, w, count, seed):
    rng = np.random.default_rng(seed)
    x = rng.random((h, w, 3))
    tg = [rng.random((h, w, 3)) for _ in range(count)]
    cs = []
    for _ in range(count):
        c = rng.random((h, w))
        c[rng.random((h, w)) < 0.3] = 0.0
        cs.append(c)
    g0 = rng.standard_normal((h, w, 3)).astype(np.float32) * 1e-3
    return x, tg, cs, g0


def _multi(xd, tds, cds, gs, g, loss, ws=None):
    """ws: the Workspaces of an earlier call (its zeroed workspace is used again), None: a fresh one; -> the one used"""
    from nn import _ops
    ws = _ops.Workspaces() if ws is None else ws
    _ops.temporal_multi_fwd_bwd(xd, tds, cds, gs, g, loss, ws=ws)
    return ws


BIG = (513, 513)        # 263169 pixels = 258 workgroups: the last-arriving one sums partials 256 and 257 on a second trip


@pytest.mark.parametrize("hw", [(64, 64), (42, 63), (257, 300), (1, 3), BIG])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_multi_fwd_bwd_matches_float64(hw, count):
    h, w = hw
    x, tg, cs, g0 = _multi_inputs(h, w, count, h + w + count)
    if hw == BIG:       # the last pixel (the last partial's only one): full certainty and the image's largest difference
        x[-1, -1] = 1.0
        for t, c in zip(tg, cs):
            t[-1, -1], c[-1, -1] = 0.0, 1.0
    gs = [3.5, 0.75, 12.0, 2.0][:count]
    xd, tds, cds = _dev(x), [_dev(t) for t in tg], [_dev(c) for c in cs]
    g = _dev(g0)
    loss = torch.zeros(count, device=DEV)
    ws = _multi(xd, tds, cds, gs, g, loss)
    torch.cuda.synchronize()
    ref_l, ref_g = TL.multi_loss64(xd.cpu().double().numpy(), [t.cpu().double().numpy() for t in tds],
                                   [c.cpu().double().numpy() for c in cds], gs)
    ref_g = g0.astype(np.float64) + ref_g
    got_l = loss.cpu().double().numpy()
    for j in range(count):
        assert abs(got_l[j] - ref_l[j]) <= 1e-5 * abs(ref_l[j]), (j, got_l[j], ref_l[j])
        if hw == BIG:   # on the host, from the float64 reference: without that pixel's term the loss FAILS the bound, so
            dropped = ref_l[j] - 1.0 * 3.0 / (3 * h * w)            # a dropped last partial cannot hide inside 1e-5
            assert abs(got_l[j] - dropped) > 1e-5 * abs(dropped), (j, got_l[j], dropped)
    got = g.cpu().double().numpy()
    assert float(np.abs(got - ref_g).max()) <= 1e-5 * float(np.abs(ref_g).max())
    none = np.all([c == 0 for c in cs], axis=0)                  # no certainty for any j: untouched
    assert np.array_equal(got[none], g0[none].astype(np.float64))
    # repeated calls: the same bits (fixed-order reductions; the workspace's ticket returns to 0)
    outs = []
    for _ in range(3):
        g = _dev(g0)
        _multi(xd, tds, cds, gs, g, loss, ws)
        outs.append((loss.clone(), g))
    torch.cuda.synchronize()
    assert all(torch.equal(outs[0][0], o[0]) and torch.equal(outs[0][1], o[1]) for o in outs)


@pytest.mark.parametrize("hw", [(64, 64), (42, 63), (257, 300), (1, 3)])
def test_count_one_is_the_single_term_kernel(hw):
    from nn import _ops
    h, w = hw
    x, tg, cs, g0 = _multi_inputs(h, w, 1, 7 * h + w)
    xd, td, cd = _dev(x), _dev(tg[0]), _dev(cs[0])
    g1, g2 = _dev(g0), _dev(g0)
    l1, l2 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    _ops.temporal_fwd_bwd(xd, td, cd, 3.5, g1, l1, ws=_ops.Workspaces())
    _multi(xd, [td], [cd], [3.5], g2, l2)
    torch.cuda.synchronize()
    assert torch.equal(l1.view(torch.int32), l2.view(torch.int32))
    assert torch.equal(g1.view(torch.int32), g2.view(torch.int32))


@pytest.mark.parametrize("hw", [(64, 64), (42, 63), (1, 3)])
@pytest.mark.parametrize("count", [2, 3, 4])
def test_zero_weights_or_certainties_leave_the_gradient(hw, count):
    h, w = hw
    x, tg, cs, g0 = _multi_inputs(h, w, count, 3 * h + w + count)
    xd, tds, cds = _dev(x), [_dev(t) for t in tg], [_dev(c) for c in cs]
    loss = torch.zeros(count, device=DEV)
    zeros = [torch.zeros_like(c) for c in cds]
    for gs, cc in (([0.0] * count, cds), ([2.0] * count, zeros)):
        g = _dev(g0)
        g[0, 0, 0] = -0.0
        before = g.clone()
        _multi(xd, tds, cc, gs, g, loss)
        torch.cuda.synchronize()
        assert torch.equal(g.view(torch.int32), before.view(torch.int32))
    assert loss.abs().sum().item() == 0.0                          # zero certainties: every term 0
    # a zero weight drops its own term only
    gs = [2.0] + [0.0] * (count - 1)
    g_a, g_b = _dev(g0), _dev(g0)
    _multi(xd, tds, cds, gs, g_a, loss)
    _multi(xd, tds, [cds[0]] + zeros[1:], gs, g_b, loss)
    torch.cuda.synchronize()
    assert torch.equal(g_a, g_b)


# ------------------------------------------------------------------ 3. the engine's step against the oracle (float64)
def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def _long_targets(h, w, count=3, seed=9):
    """count (target, combined certainty) pairs: binary raw certainties with disjoint-ish holes, combined as the run does"""
    rng = np.random.default_rng(seed)
    raw = (rng.random((count, h, w)) > 0.3).astype(np.float32)
    raw[0, :, : w // 4] = 0.0                                       # nearest frame blind on the left: older ones fill in
    comb = TL.long_certainty32(raw)
    return [(_img(h, w, 50 + seed + j)[0], torch.from_numpy(comb[j].copy())) for j in range(count)]


LAMS = (40.0, 25.0, 60.0)


def _engine_case(h, w, regions=1, blend=False, cw=False, n=1024, seed=0, temporal="multi", oracle=True):
    """temporal: "multi" (three targets), "list1" ([TemporalTarget]), "single" (TemporalTarget), None"""
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
    pairs = _long_targets(h, w, 3 if temporal == "multi" else 1)
    lams = LAMS[:len(pairs)]
    tts = [engine.TemporalTarget(tg.to(DEV), c.to(DEV), lam) for (tg, c), lam in zip(pairs, lams)]
    tt = {"multi": tts, "list1": tts[:1], "single": tts[0], None: None}[temporal]
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
    lts = [(c.double()[None, :, :, None] * (img - tg.double()[None]) ** 2).sum() / (3 * h * w) for tg, c in pairs]
    total = loss + sum(lam * lt for lam, lt in zip(lams, lts))
    grads = torch.autograd.grad(total, variables)
    return eng, idx_dev, dict(loss=float(total), loss_c=float(lc_sum) / len(idx), loss_t=float(sum(lts)),
                              terms=[float(lt) for lt in lts], grads=grads)


@pytest.mark.parametrize("case", [dict(h=64, w=64), dict(h=42, w=64), dict(h=64, w=64, regions=2),
                                  dict(h=48, w=64, blend=True, cw=True)], ids=["64x64", "42x64", "2-regions", "blend-K2-cw"])
def test_engine_three_targets_match_the_oracle(case):
    eng, idx, ref = _engine_case(**case)
    eng.forward_backward(idx)
    torch.cuda.synchronize()
    got = eng.losses()
    for key in ("loss", "loss_c", "loss_t"):
        assert abs(got[key] - ref[key]) < 5e-5 * max(1.0, abs(ref[key])), (key, got[key], ref[key])
    assert len(got["loss_t_terms"]) == 3
    for a, b in zip(got["loss_t_terms"], ref["terms"]):
        assert abs(a - b) < 5e-5 * max(1.0, abs(b)), (a, b)
    g0, r0 = eng.gvars[0].cpu().double(), ref["grads"][0]
    assert float((g0 - r0).norm() / r0.norm()) < 2e-3
    # the terms are a real part of the step, each of them present
    assert sum(lam * lt for lam, lt in zip(LAMS, ref["terms"])) > 0.05 * ref["loss"] and min(ref["terms"]) > 0


@pytest.mark.parametrize("graph", [False, True])
def test_one_element_list_is_the_temporal_target_engine(graph, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    a, idx, _ = _engine_case(64, 64, temporal="list1", oracle=False)
    b, _, _ = _engine_case(64, 64, temporal="single", oracle=False)
    if graph:
        a.capture_graph(idx)
        b.capture_graph(idx)
    for _ in range(3):
        a.step(idx)
        b.step(idx)
    torch.cuda.synchronize()
    la, lb = a.losses(), b.losses()
    assert la == lb and "loss_t_terms" not in la
    for x, y in zip(a.variables + a.gvars, b.variables + b.gvars):
        assert torch.equal(x, y)


@pytest.mark.parametrize("regions", [1, 2])
def test_three_target_step_graph_eager_and_host_draw_agree(regions, monkeypatch):
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
    assert len(graph.losses()["loss_t_terms"]) == 3
    for a, b, c in zip(graph.variables, eager.variables, host.variables):
        assert torch.equal(a, b) and torch.equal(a, c)


def test_engine_refuses_bad_target_sets():
    from nn import engine
    eng, _, _ = _engine_case(64, 64, n=256, temporal=None, oracle=False)
    args = (eng.params, eng.content_feat, eng.style_targets, eng.stylized(), 8.0, 10.0, 2e-3)
    (tg, c), = _long_targets(64, 64, 1)
    good = engine.TemporalTarget(tg, c, 1.0)
    for bad in ([], [good] * 5, [good, engine.TemporalTarget(tg[:32], c, 1.0)],
                [good, engine.TemporalTarget(tg, c[:, :10], 1.0)], [good, engine.TemporalTarget(tg, c, -1.0)],
                [engine.TemporalTarget(tg, c, float("inf")), good], [good, (tg, c)]):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=256, temporal=bad)
    with pytest.raises(ValueError):
        engine.StepEngine(*args, sample_size=256, temporal=[good, good], dist_group=object())


def test_temporal_targets_at_scale_is_the_one_target_resize_per_target():
    from nn import strotss_utils as SU
    rng = np.random.default_rng(0)
    pairs = [(_dev(rng.random((1, 48, 64, 3))), _dev(rng.random((48, 64)))) for _ in range(3)]
    got = SU.temporal_targets_at_scale(pairs, 24, 32)
    assert len(got) == 3
    for (w_, c_), (tg, cc) in zip(pairs, got):
        rt, rc = SU.temporal_target_at_scale(w_, c_, 24, 32)
        assert torch.equal(tg, rt) and torch.equal(cc, rc)


def test_temporal_targets_for_frame_reads_and_combines(tmp_path):
    import run_strotss as RS
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    paths, occluder = TL.occluder_sequence(frames, flows, n_frames=3, offsets=(1, 2))
    args = RS._resolve(RS.build_parser().parse_args([frames, "s.jpg", "--video", "--flow_dir", flows,
                                                     "--temporal_frames", "1", "2"]))
    rng = np.random.default_rng(1)
    results = [_dev(rng.random((1, 48, 64, 3))) for _ in range(2)]     # frames 2 and 1
    pairs = RS._temporal_targets_for_frame(args, 3, results)
    torch.cuda.synchronize()
    assert len(pairs) == 2
    raw = []
    for j, (warped, cert) in zip((1, 2), pairs):
        w1, c1 = RS._flow_warp_for_frame(args, 3, results[j - 1], j)[1:]
        assert torch.equal(warped, w1)
        raw.append(c1.cpu().numpy())
    comb = TL.long_certainty32(np.stack(raw))
    for j in range(2):
        assert np.array_equal(pairs[j][1].cpu().numpy(), comb[j])
    # the background frame 2's occluder hid, visible in frame 1: pulled toward frame 1 only
    hole = occluder(2) & ~occluder(3) & ~occluder(1)
    assert hole.any() and (comb[0][hole] == 0).all() and (comb[1][hole] == 1).all()
    # frame 2: only j = 1 applies -- the one-target pair, raw
    one = RS._temporal_targets_for_frame(args, 2, results[1:])
    assert len(one) == 1 and torch.equal(one[0][1], RS._flow_warp_for_frame(args, 2, results[1], 1)[2])


# ------------------------------------------------------------------ 4. --temporal_frames end to end
LONG_TERM_RATIO = 0.3           # E(J = {1, 2}) < ratio * E(J = {1}) on the reappearing pixels: measured 0.118


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


def test_long_term_end_to_end(tmp_path, monkeypatch):
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    frames, flows = str(tmp_path / "frames"), str(tmp_path / "flows")
    paths, occluder = TL.occluder_sequence(frames, flows, n_frames=4, offsets=(1, 2))
    style = str(tmp_path / "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    plain = _video_run(tmp_path, frames, flows, style, "plain")
    short = _video_run(tmp_path, frames, flows, style, "short", "--temporal_frames", "1")
    long_ = _video_run(tmp_path, frames, flows, style, "long", "--temporal_frames", "1", "2")
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    for s in stems:                    # --temporal_frames 1 is the run without the flag, byte for byte
        assert open(plain / f"{s}.jpg", "rb").read() == open(short / f"{s}.jpg", "rb").read(), s
    for s in stems[:2]:                # frames 1 and 2 have no frame t-2: the same bytes
        assert open(short / f"{s}.jpg", "rb").read() == open(long_ / f"{s}.jpg", "rb").read(), s
    # the background the occluder hid in frame t-1, visible in t-2 and t: out_t against out_{t-2}

    def err(out):
        e = []
        for t in (3, 4):
            hole = occluder(t - 1) & ~occluder(t) & ~occluder(t - 2)
            d = _read(out / f"{stems[t - 1]}.jpg") - _read(out / f"{stems[t - 3]}.jpg")
            e.append((d[hole] ** 2).mean())
        return float(np.mean(e))
    e_short, e_long = err(short), err(long_)
    print(f"reappearing background: E(J=1) {e_short:.6f}, E(J=1,2) {e_long:.6f}, ratio {e_long / e_short:.4f}")
    assert e_long < LONG_TERM_RATIO * e_short, (e_short, e_long)
