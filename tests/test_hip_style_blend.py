"""Style blending on the MI355X: strotss_step_losses_blend_fwd_bwd against the single-style call (one style: bit for bit; several:
the sum of single-style calls) and against float64 autograd of sum_k w_k style_loss + alpha content_loss; the engine's blended
step against the oracle, its fallback and its captured graph; run() with --style_mix end to end."""
import os

import numpy as np
import pytest
import torch

from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda"
D = 2179


def _feat(n, d, seed, dup=()):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, d)), 0) + 0.01 * rng.random((n, d))
    x[:, :3] = rng.random((n, 3))
    for grp in dup:                      # exact duplicate rows: tied minima (reduce_min splits among them)
        x[list(grp[1:])] = x[grp[0]]
    return x


def _fbuf(ops, x):
    n, d = x.shape
    b = torch.zeros(ops.pad32(n), ops.pad32(d), dtype=torch.float32, device=DEV)
    b[:n, :d] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


def _target(ops, x):
    from nn.engine import StyleTarget
    return StyleTarget.build(_fbuf(ops, x), x.shape[0], x.shape[1])


def _blend_call(ops, targets, weights, by, bc, n, d, g, ls):
    k = len(targets)
    out = torch.zeros((4, 4), dtype=torch.float32, device=DEV)      # [content | moment_k | remd_k | palette_k]
    s = ops.make_style_set(targets, weights)
    ops.step_losses_blend_fwd_bwd(by, bc, n, d, s, g[0], g[1], g[2], g[3], ls, out[0], out[1], out[2], out[3])
    torch.cuda.synchronize()
    return out[0, 0].item(), out[1:, :k].cpu().numpy().astype(np.float64)


def test_one_style_blend_is_the_single_style_call_bitwise():
    from nn import _ops as ops
    if not ops.step_losses_available():
        pytest.skip("bf16x3 core switched off")
    n, ns = 1024, 1000
    x, y, c = _feat(ns, D, 1, dup=[(3, 7, 11)]), _feat(n, D, 2, dup=[(0, 5)]), _feat(n, D, 3)
    by, bc = _fbuf(ops, y), _fbuf(ops, c)
    t = _target(ops, x)
    g1 = torch.zeros_like(by); l1 = torch.zeros(4, device=DEV)
    ops.step_losses_fwd_bwd(by, bc, n, D, t.feats, t.inv_norm, t.panels, t.ns, t.mean, t.cov, 0.7, 0.3, 0.9, 0.4, g1, l1[0:],
                            l1[1:], l1[2:], l1[3:])
    g2 = torch.zeros_like(by)
    lc, per = _blend_call(ops, [t], [1.0], by, bc, n, D, (0.7, 0.3, 0.9, 0.4), g2)
    assert torch.equal(g1, g2)
    got = np.array([lc, per[0, 0], per[1, 0], per[2, 0]], dtype=np.float32)
    assert np.array_equal(got, l1.cpu().numpy())


@pytest.mark.parametrize("k", [2, 3])
def test_blend_matches_float64_autograd_and_the_sum_of_single_calls(k):
    from nn import _ops as ops
    if not ops.step_losses_available():
        pytest.skip("bf16x3 core switched off")
    n, alpha = 1024, 4.0
    inv_alpha = 1.0 / max(alpha, 1.0)
    ns_all = (1024, 1000, 777)[:k]
    weights = [0.5, 0.3, 0.2][:k] if k == 3 else [0.7, 0.3]
    xs = [_feat(ns, D, 10 + i, dup=[(1, 9, 17), (40, 41)]) for i, ns in enumerate(ns_all)]
    y, c = _feat(n, D, 20, dup=[(2, 30), (100, 101, 102)]), _feat(n, D, 21)
    by, bc = _fbuf(ops, y), _fbuf(ops, c)
    targets = [_target(ops, x) for x in xs]
    g = (alpha, 1.0, 1.0, inv_alpha)
    gb = torch.zeros_like(by)
    lc, per = _blend_call(ops, targets, weights, by, bc, n, D, g, gb)
    gb = gb[:n, :D].cpu().double()
    # float64 autograd of alpha * content_loss + sum_k w_k * style_loss
    p = torch.as_tensor(y, dtype=torch.float64).requires_grad_(True)
    ct = torch.as_tensor(c, dtype=torch.float64)
    lc_ref = O.content_loss(ct, p)
    terms = []
    for x in xs:
        xt = torch.as_tensor(x, dtype=torch.float64)
        yuv = O.convert_rgb_to_yuv
        terms.append((O.moment_matching(xt, p), O.relaxed_emd(xt, p), O.relaxed_emd(yuv(xt), yuv(p), "both")))
    total = alpha * lc_ref + sum(w * (m + r + inv_alpha * q) for w, (m, r, q) in zip(weights, terms))
    total.backward()
    assert abs(lc - lc_ref.item()) < 5e-5 * max(1.0, abs(lc_ref.item()))
    for i, (m, r, q) in enumerate(terms):
        for j, ref in enumerate((m, r, q)):
            assert abs(per[j, i] - float(ref)) < 5e-5 * max(1.0, abs(float(ref))), (i, j, per[j, i], float(ref))
    ref_g = p.grad
    assert float((gb - ref_g).norm() / ref_g.norm()) < 3e-3
    # the sum of K single-style calls (the content term once)
    gs = torch.zeros_like(by)
    for i, (t, w) in enumerate(zip(targets, weights)):
        l = torch.zeros(4, device=DEV)
        ops.step_losses_fwd_bwd(by, bc, n, D, t.feats, t.inv_norm, t.panels, t.ns, t.mean, t.cov, alpha if i == 0 else 0.0,
                                w * g[1], w * g[2], w * g[3], gs, l[0:], l[1:], l[2:], l[3:])
        torch.cuda.synchronize()
        lv = l.cpu().numpy().astype(np.float64)
        assert np.abs(lv[1:] - per[:, i]).max() <= 1e-5 * max(1.0, np.abs(lv[1:]).max()), (lv, per[:, i])
    gs = gs[:n, :D].cpu().double()
    assert float((gb - gs).abs().max()) <= 1e-5 * float(gs.abs().max())


def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def _blend_setup(weights=(0.6, 0.4), n_samples=1024, h=48, w=64):
    from nn import _ops, engine
    from nn.model import VGGParams, synthetic_weights
    wts = synthetic_weights('16', 0)
    content, styles = _img(h, w, 1), [_img(56, 60, 2), _img(40, 72, 3)]
    rng = np.random.default_rng(0)
    alpha = 8.0
    denom = 2.0 + alpha + 1.0 / max(alpha, 1.0)
    vgg = O.VGG(wts, dtype=torch.float64)
    params = VGGParams(wts, '16', None, DEV)
    with torch.no_grad():
        cf = [content.double()] + vgg(content.double())
    s_samples, targets = [], []
    for s in styles:
        s64 = s.double()
        with torch.no_grad():
            sf = [s64] + vgg(s64)
        s_idx = O.make_indices(s.shape[1], s.shape[2], False, n_samples, rng)
        with torch.no_grad():
            s_samples.append(O.sample_features(sf, s_idx, False))
        feats = _ops.hypercol_gather(engine.extract_features(params, s.to(DEV)), torch.from_numpy(s_idx).to(DEV), False)
        targets.append(engine.StyleTarget.build(feats, s_idx.shape[0], D))
    wn = engine.normalise_style_weights(weights)
    init = O.make_laplacian(content.double()) + sum(wk * s.double().mean(dim=(1, 2), keepdim=True) for wk, s in zip(wn, styles))
    idx = [O.make_indices(h, w, True, n_samples, rng) for _ in range(3)]
    cfeat = engine.extract_features(params, content.to(DEV))

    def make(**kw):
        return engine.StepEngine(params, cfeat, [engine.StyleBlend(targets, list(weights))], init.float().to(DEV), alpha, denom,
                                 2e-3, sample_size=n_samples, **kw)
    return dict(vgg=vgg, cf=cf, s_samples=s_samples, weights=wn, init=init, idx=idx, alpha=alpha, denom=denom, make=make)


def test_engine_blend_step_matches_the_oracle():
    S = _blend_setup()
    eng = S["make"]()
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(S["init"])]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + S["vgg"](img)
    c_feat = O.sample_features(S["cf"], S["idx"][0], True)
    p_feat = O.sample_features(pred, S["idx"][0], True)
    lc = O.content_loss(c_feat, p_feat)
    ls = sum(w * O.style_loss(s, p_feat, S["alpha"]) for w, s in zip(S["weights"], S["s_samples"]))
    loss = (S["alpha"] * lc + ls) / S["denom"]
    grads = torch.autograd.grad(loss, variables)
    eng.forward_backward([torch.from_numpy(S["idx"][0]).to(DEV)])
    torch.cuda.synchronize()
    got = eng.losses()
    for key, ref in (("loss", loss), ("loss_c", lc), ("loss_s", ls)):
        assert abs(got[key] - float(ref)) < 5e-5 * max(1.0, abs(float(ref))), (key, got[key], float(ref))
    assert len(got["per_style"]) == 2 and abs(sum(p["weight"] for p in got["per_style"]) - 1.0) < 1e-12
    blended = sum(p["weight"] * p["loss_s"] for p in got["per_style"])
    assert abs(blended - got["loss_s"]) < 1e-9 * max(1.0, abs(blended))
    g0, r0 = eng.gvars[0].cpu().double(), grads[0]
    assert float((g0 - r0).norm() / r0.norm()) < 2e-3


def test_engine_blend_fallback_and_graph_replay(monkeypatch):
    S = _blend_setup()
    idx = [torch.from_numpy(S["idx"][0]).to(DEV)]
    a = S["make"]()
    a.forward_backward(idx)
    torch.cuda.synchronize()
    monkeypatch.setenv("STROTSS_GROUPED_LOSSES", "0")          # the K-loop of separate entries
    b = S["make"]()
    b.forward_backward(idx)
    torch.cuda.synchronize()
    monkeypatch.delenv("STROTSS_GROUPED_LOSSES")
    la, lb = a.losses(), b.losses()
    for key in ("loss", "loss_c", "loss_s", "l_moment", "l_remd", "l_palette"):
        assert abs(la[key] - lb[key]) <= 1e-5 * max(1.0, abs(la[key])), (key, la[key], lb[key])
    ga, gb = a.gp[0], b.gp[0]
    assert float((ga - gb).abs().max()) <= 1e-5 * float(ga.abs().max())
    # captured graph == eager, bit for bit, in deterministic mode
    e = S["make"](deterministic=True)
    g = S["make"](deterministic=True)
    g.capture_graph([i.clone() for i in idx])
    for step in range(2):
        ii = [torch.from_numpy(S["idx"][step]).to(DEV)]
        e.step(ii)
        g.step(ii)
    torch.cuda.synchronize()
    assert e.losses() == g.losses()
    for x, y in zip(e.variables, g.variables):
        assert torch.equal(x, y)


def test_engine_refuses_blends_with_regions():
    S = _blend_setup(n_samples=256)
    from nn import engine
    eng = S["make"]()
    blend = eng.style_targets[0]
    with pytest.raises(ValueError):
        engine.StepEngine(eng.params, eng.content_feat, [blend, blend], S["init"].float().to(DEV), 8.0, 10.0, 2e-3, sample_size=256)


def _write_images(tmp_path):
    from PIL import Image
    rng = np.random.default_rng(4)
    paths = []
    for name, (h, w) in (("c.jpg", (90, 120)), ("s.jpg", (100, 80)), ("s2.jpg", (70, 110))):
        arr = (rng.random((h // 10, w // 10, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).resize((w, h), Image.BILINEAR).save(tmp_path / name, quality=95)
        paths.append(str(tmp_path / name))
    return paths


def test_run_with_style_mix(tmp_path, monkeypatch):
    import run_strotss as RS
    from nn import strotss_utils, utils
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")      # sorted tap scatter: two runs of one configuration are bitwise alike
    c, s, s2 = _write_images(tmp_path)
    base = [c, s, "--level", "1", "--max_iter", "4"]
    single, zero = str(tmp_path / "single.jpg"), str(tmp_path / "zero.jpg")
    RS.run(RS.build_parser().parse_args(base + ["-o", single]))
    RS.run(RS.build_parser().parse_args(base + ["-o", zero, "--style_mix", s2, "--style_weights", "1", "0"]))
    with open(single, "rb") as f1, open(zero, "rb") as f2:
        assert f1.read() == f2.read()                   # a zero-weight style is never loaded: the single-style run
    tr = []
    out = str(tmp_path / "mix.jpg")
    RS.run(RS.build_parser().parse_args([c, s, "-o", out, "--level", "2", "--max_iter", "5", "--style_mix", s2,
                                         "--style_weights", "3", "1"]), trace=tr)
    assert os.path.exists(out) and len(tr) == 2
    for rec in tr:
        for st in rec["steps"]:
            assert all(np.isfinite(st[k]) for k in ("loss", "loss_c", "loss_s")) and len(st["per_style"]) == 2
    content = utils.load_image(c)
    styles = [utils.load_image(p) for p in (s, s2)]
    c64 = utils.resize(content, 64)
    init = strotss_utils.make_laplacian(c64) + (0.75 * utils.resize(styles[0], 64).mean(dim=(1, 2), keepdim=True)
                                                + 0.25 * utils.resize(styles[1], 64).mean(dim=(1, 2), keepdim=True))
    assert float((tr[0]["init"].cpu().double() - init.cpu().double()).abs().max()) < 1e-6
