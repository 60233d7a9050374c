"""Content-weight map on the MI355X: the weighted self-similarity entries against the unweighted ones (all-ones weights: bit for
bit) and against a float64 autograd restatement of the weighted loss, the weight gather folded into the feature gather against a
level-0 hypercolumn gather, the engine's weighted step against the oracle composed in float64, graph / eager / host-draw
equality in deterministic mode, and run() with --content_weight_map end to end."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 2179


def weighted_selfsim64(x, y, c):
    """(1/n) sum_j c_j sum_i |A[i,j] - B[i,j]|, A / B the column-normalised cosine matrices of x / y (float64 autograd)"""
    def cols(z):
        dz = O.cosine_distance(z, z)
        return dz / torch.clamp(dz.sum(dim=0), min=1e-12)
    return (c[None, :] * (cols(x) - cols(y)).abs()).sum() / x.shape[0]


def _feat(n, d, seed, dup=()):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, d)), 0) + 0.01 * rng.random((n, d))
    x[:, :3] = rng.random((n, 3))
    for grp in dup:                      # exact duplicate rows (tied minima, equal self-similarity columns)
        x[list(grp[1:])] = x[grp[0]]
    return x


def _fbuf(ops, x):
    n, d = x.shape
    b = torch.zeros(ops.pad32(n), ops.pad32(d), dtype=torch.float32, device=DEV)
    b[:n, :d] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


def _wbuf(ops, c):
    b = torch.zeros(ops.pad32(len(c)), dtype=torch.float32, device=DEV)
    b[:len(c)] = torch.as_tensor(c, dtype=torch.float32, device=DEV)
    return b


def _weights(n, seed):
    rng = np.random.default_rng(seed)
    c = rng.random(n).astype(np.float32)
    c[rng.permutation(n)[:n // 8]] = 0.0          # some samples exactly without content weight
    return c


def _target(ops, x):
    from nn.engine import StyleTarget
    return StyleTarget.build(_fbuf(ops, x), x.shape[0], x.shape[1])


def _grouped_available(ops):
    if not ops.step_losses_available():
        pytest.skip("bf16x3 core switched off")


# ------------------------------------------------------------------ 1. all-ones weights: the unweighted entries, bit for bit
def test_all_ones_weights_are_the_unweighted_entries_bitwise():
    from nn import _ops as ops
    _grouped_available(ops)
    n, ns = 1000, 777
    y, c = _feat(n, D, 2, dup=[(0, 5)]), _feat(n, D, 3)
    by, bc = _fbuf(ops, y), _fbuf(ops, c)
    ones = _wbuf(ops, np.ones(n, dtype=np.float32))
    # separate entry
    g0, g1 = torch.zeros_like(by), torch.zeros_like(by)
    l0, l1 = torch.zeros(1, device=DEV), torch.zeros(1, device=DEV)
    ops.selfsim_fwd_bwd(by, bc, n, D, 0.7, g0, l0)
    ops.selfsim_weighted_fwd_bwd(by, bc, ones, n, D, 0.7, g1, l1)
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and torch.equal(l0, l1)
    g = (0.7, 0.3, 0.9, 0.4)
    targets = [_target(ops, _feat(ns, D, 10, dup=[(1, 9)])), _target(ops, _feat(1024, D, 11))]
    # grouped, K = 1: strotss_step_losses_fwd_bwd
    t = targets[0]
    g0, g1 = torch.zeros_like(by), torch.zeros_like(by)
    l0, l1 = torch.zeros(4, device=DEV), torch.zeros(4, device=DEV)
    ops.step_losses_fwd_bwd(by, bc, n, D, t.feats, t.inv_norm, t.panels, t.ns, t.mean, t.cov, *g, g0, l0[0:], l0[1:], l0[2:],
                            l0[3:])
    ops.step_losses_cw_fwd_bwd(by, bc, n, D, ones, ops.make_style_set([t], [1.0]), *g, g1, l1[0:], l1[1:], l1[2:], l1[3:])
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and torch.equal(l0, l1)
    # grouped, K = 2: strotss_step_losses_blend_fwd_bwd
    s = ops.make_style_set(targets, [0.6, 0.4])
    g0, g1 = torch.zeros_like(by), torch.zeros_like(by)
    l0, l1 = torch.zeros((4, 4), device=DEV), torch.zeros((4, 4), device=DEV)
    ops.step_losses_blend_fwd_bwd(by, bc, n, D, s, *g, g0, l0[0], l0[1], l0[2], l0[3])
    ops.step_losses_cw_fwd_bwd(by, bc, n, D, ones, s, *g, g1, l1[0], l1[1], l1[2], l1[3])
    torch.cuda.synchronize()
    assert torch.equal(g0, g1) and torch.equal(l0, l1)


# ------------------------------------------------------------------ 2. random weights against float64, grouped against separate
@pytest.mark.parametrize("n", [1024, 1000, 777])
def test_weighted_losses_match_float64_and_the_separate_entries(n):
    from nn import _ops as ops
    _grouped_available(ops)
    alpha = 4.0
    inv_alpha = 1.0 / alpha
    y, c = _feat(n, D, 20 + n, dup=[(2, 30), (100, 101, 102)]), _feat(n, D, 21 + n, dup=[(7, 8)])
    cw = _weights(n, n)
    by, bc, wb = _fbuf(ops, y), _fbuf(ops, c), _wbuf(ops, cw)
    # the separate entry against float64 autograd
    g = torch.zeros_like(by)
    l = torch.zeros(1, device=DEV)
    ops.selfsim_weighted_fwd_bwd(by, bc, wb, n, D, 1.0, g, l)
    torch.cuda.synchronize()
    p = torch.as_tensor(y, dtype=torch.float64).requires_grad_(True)
    ref = weighted_selfsim64(p, torch.as_tensor(c, dtype=torch.float64), torch.as_tensor(cw, dtype=torch.float64))
    ref.backward()
    assert abs(l.item() - ref.item()) < 5e-5 * max(1.0, abs(ref.item())), (l.item(), ref.item())
    gg = g[:n, :D].cpu().double()
    assert float((gg - p.grad).norm() / p.grad.norm()) < 3e-3
    # the grouped step (K = 1 and K = 2) against the separate entries the fallback path calls
    xs = [_feat(1000, D, 40, dup=[(1, 9, 17)]), _feat(1024, D, 41)]
    targets = [_target(ops, x) for x in xs]
    for weights in ([1.0], [0.7, 0.3]):
        k = len(weights)
        gsum = (alpha, 1.0, 1.0, inv_alpha)
        ga = torch.zeros_like(by)
        la = torch.zeros((4, 4), device=DEV)
        ops.step_losses_cw_fwd_bwd(by, bc, n, D, wb, ops.make_style_set(targets[:k], weights), *gsum, ga, la[0], la[1], la[2],
                                   la[3])
        gb = torch.zeros_like(by)
        lc = torch.zeros(1, device=DEV)
        ops.selfsim_weighted_fwd_bwd(by, bc, wb, n, D, alpha, gb, lc)
        lb = torch.zeros((3, 4), device=DEV)
        for i, (t, w) in enumerate(zip(targets[:k], weights)):
            ops.moment_fwd_bwd(t.mean, t.cov, by, n, D, w, gb, lb[0, i:])
            ops.remd_cos_fwd_bwd_after_selfsim(t.feats, t.inv_norm, t.panels, t.ns, by, n, D, w, gb, lb[1, i:])
            ops.palette_remd_fwd_bwd(t.feats, t.ns, by, n, inv_alpha * w, gb, lb[2, i:])
        torch.cuda.synchronize()
        assert abs(la[0, 0].item() - lc.item()) <= 1e-5 * max(1.0, abs(lc.item()))
        assert abs(la[0, 0].item() - ref.item()) < 5e-5 * max(1.0, abs(ref.item()))
        assert float((la[1:, :k] - lb[:, :k]).abs().max()) <= 1e-5 * max(1.0, float(lb.abs().max()))
        assert float((ga - gb).abs().max()) <= 1e-5 * float(gb.abs().max()), k


# ------------------------------------------------------------------ 3. the weight gather: a level-0 gather of the map
@pytest.mark.parametrize("masked", [False, True])
def test_weight_gather_is_a_level0_gather_bitwise(masked):
    from nn import _hip, _ops as ops
    h, w, n = 64, 48, 512
    g = torch.Generator().manual_seed(5)
    img = torch.rand(1, h, w, 3, generator=g).to(DEV)
    wmap = (torch.rand(1, h, w, 1, generator=g) * 1.5).to(DEV)
    masks = [None]
    if masked:
        m0 = np.zeros((h, w), dtype=bool)
        m0[:, : w // 2] = True
        masks = [m0, ~m0]
    dev_masks = [None if m is None else torch.from_numpy(m.astype(np.uint8)).to(DEV) for m in masks]
    idx = [torch.zeros((n, 2), dtype=torch.float32, device=DEV) for _ in masks]
    counters = torch.arange(len(masks), dtype=torch.int32, device=DEV)
    ops.index_draw(h, w, n, 11, counters, idx, dev_masks)
    mt = _hip.make_maps([img], [[]])
    mw = _hip.make_maps([wmap], [[]])
    for r, ix in enumerate(idx):
        ref = ops.hypercol_gather([wmap], ix, True)[:n, 0]
        rows = ops.pad32(n) + 32
        out_a = torch.full((rows, 32), 7.0, device=DEV)
        out_b = torch.full((rows, 32), 7.0, device=DEV)
        wout = torch.full((rows,), 7.0, device=DEV)
        rc = _hip.lib().strotss_hypercol_gather2_cw(C.byref(mt), C.byref(mt), C.byref(mw), ix.data_ptr(), n, 1,
                                                    out_a.data_ptr(), out_b.data_ptr(), 32, None, 0, wout.data_ptr(), rows,
                                                    _hip.stream_ptr())
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(wout[:n], ref)
        assert torch.equal(wout[n:], torch.zeros(rows - n, device=DEV))
        assert torch.equal(out_a[:n], ops.hypercol_gather([img], ix, True)[:n, :32])
        # the draw's coordinates are integers: the weight IS the map's pixel
        rc_ = ix.long()
        assert torch.equal(wout[:n], wmap[0, rc_[:, 0], rc_[:, 1], 0])
        if masks[r] is not None:
            assert bool(torch.from_numpy(masks[r]).to(DEV)[rc_[:, 0], rc_[:, 1]].all())


# ------------------------------------------------------------------ 4. the engine's step against the oracle (float64)
def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def ramp_map(h, w):
    """a ramp over the columns, 0 .. 1.2, with a band of exact zeros"""
    m = np.tile(np.linspace(0.0, 1.2, w, dtype=np.float32), (h, 1))
    m[h // 3: h // 3 + max(2, h // 8)] = 0.0
    return torch.from_numpy(m)


def _engine_case(h, w, regions=1, blend=False, n=1024, seed=0, oracle=True):
    from nn import engine
    from nn import _ops
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
    wmap = ramp_map(h, w)
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), st, init.float().to(DEV), alpha, denom,
                            2e-3, sample_size=n, content_weight=wmap.to(DEV))
    if not oracle:
        return eng, [torch.from_numpy(i).to(DEV) for i in idx], None, None, None
    # oracle: mean over regions of (alpha * weighted content loss + style loss) / denom
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    w64 = wmap.double()[None, :, :, None]
    loss = lc_sum = 0.0
    for r, ix in enumerate(idx):
        c_feat = O.sample_features(cf, ix, True)
        p_feat = O.sample_features(pred, ix, True)
        cj = O.sample_features([w64], ix, True)[:, 0]
        lc = weighted_selfsim64(p_feat, c_feat, cj)
        ls = (sum(wk * O.style_loss(s, p_feat, alpha) for wk, s in zip(weights, s_samples)) if blend
              else O.style_loss(s_samples[r], p_feat, alpha))
        loss = loss + (alpha * lc + ls) / denom
        lc_sum = lc_sum + lc
    loss = loss / len(idx)
    grads = torch.autograd.grad(loss, variables)
    return eng, [torch.from_numpy(i).to(DEV) for i in idx], float(loss), float(lc_sum) / len(idx), grads


@pytest.mark.parametrize("case", [dict(h=64, w=64), dict(h=42, w=64), dict(h=64, w=64, regions=2),
                                  dict(h=48, w=64, blend=True)], ids=["64x64", "42x64", "2-regions", "blend-K2"])
def test_engine_weighted_step_matches_the_oracle(case):
    eng, idx, loss, lc, grads = _engine_case(**case)
    eng.forward_backward(idx)
    torch.cuda.synchronize()
    got = eng.losses()
    assert abs(got["loss"] - loss) < 5e-5 * max(1.0, abs(loss)), (got["loss"], loss)
    assert abs(got["loss_c"] - lc) < 5e-5 * max(1.0, abs(lc)), (got["loss_c"], lc)
    g0, r0 = eng.gvars[0].cpu().double(), grads[0]
    assert float((g0 - r0).norm() / r0.norm()) < 2e-3


def test_engine_weighted_fallback_matches_the_grouped_call(monkeypatch):
    eng, idx, _, _, _ = _engine_case(64, 64, oracle=False)
    eng.forward_backward(idx)
    torch.cuda.synchronize()
    monkeypatch.setenv("STROTSS_GROUPED_LOSSES", "0")           # the separate weighted entry + the style entries
    eng2, _, _, _, _ = _engine_case(64, 64, oracle=False)
    eng2.forward_backward(idx)
    torch.cuda.synchronize()
    la, lb = eng.losses(), eng2.losses()
    for key in ("loss", "loss_c", "loss_s"):
        assert abs(la[key] - lb[key]) <= 1e-5 * max(1.0, abs(la[key])), (key, la[key], lb[key])
    ga, gb = eng.gp[0], eng2.gp[0]
    assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())


# ------------------------------------------------------------------ 5. deterministic mode: graph == eager, host draw == device draw
@pytest.mark.parametrize("regions", [1, 2])
def test_weighted_step_graph_eager_and_host_draw_agree(regions, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    from nn import rand
    from nn import strotss_utils as SU
    h, w, n, seed, steps = 64, 64, 1024, 17, 3

    def make():
        eng, _, _, _, _ = _engine_case(h, w, regions=regions, oracle=False)
        return eng
    masks = [None]
    if regions == 2:
        m0 = np.zeros((h, w), dtype=bool)
        m0[:, : w // 2] = True
        masks = [m0, ~m0]
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


def test_engine_refuses_bad_maps_and_sharding():
    from nn import engine
    eng, _, _, _, _ = _engine_case(64, 64, n=256, oracle=False)
    st, init = eng.style_targets, eng.variables[0]
    args = (eng.params, eng.content_feat, st, eng.stylized(), 8.0, 10.0, 2e-3)
    for bad in (torch.zeros(32, 64), torch.full((64, 64), float("nan")), -torch.ones(64, 64)):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=256, content_weight=bad.to(DEV))
    with pytest.raises(ValueError):
        engine.StepEngine(*args, sample_size=256, content_weight=torch.ones(64, 64, device=DEV), dist_group=object())


# ------------------------------------------------------------------ 6. run() with --content_weight_map
def _write_images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    paths = []
    for name, (h, w) in (("c.jpg", (90, 120)), ("s.jpg", (100, 80))):
        arr = (rng.random((h // 10, w // 10, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).resize((w, h), Image.BILINEAR).save(tmp_path / name, quality=95)
        paths.append(str(tmp_path / name))
    white = np.full((90, 120), 255, dtype=np.uint8)
    half = white.copy()
    half[:, :60] = 0
    for name, arr in (("white.png", white), ("half.png", half)):
        Image.fromarray(arr).save(tmp_path / name)
        paths.append(str(tmp_path / name))
    return paths


def test_run_with_content_weight_map(tmp_path, monkeypatch):
    import run_strotss as RS
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")      # sorted tap scatter: two runs of one configuration are bitwise alike
    c, s, white, half = _write_images(tmp_path)
    base = [c, s, "--level", "1", "--max_iter", "4"]
    outs = {k: str(tmp_path / f"{k}.jpg") for k in ("plain", "white", "half")}
    RS.run(RS.build_parser().parse_args(base + ["-o", outs["plain"]]))
    RS.run(RS.build_parser().parse_args(base + ["-o", outs["white"], "--content_weight_map", white]))
    tr = []
    RS.run(RS.build_parser().parse_args(base + ["-o", outs["half"], "--content_weight_map", half]), trace=tr)
    data = {k: open(p, "rb").read() for k, p in outs.items()}
    assert data["plain"] == data["white"]               # all ones: every weighted kernel is the unweighted one bit for bit
    assert data["half"] != data["plain"]
    assert all(np.isfinite(st[k]) for st in tr[0]["steps"] for k in ("loss", "loss_c", "loss_s"))
    with pytest.raises(ValueError):
        RS.run(RS.build_parser().parse_args(base + ["-o", str(tmp_path / "x.jpg"), "--content_weight_map", half, "--strips"]))
