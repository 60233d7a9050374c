"""The pixel-space priors on the MI355X: strotss_pool_mean, strotss_detail_fwd_bwd and
strotss_tv_fwd_bwd against the float64 restatement of tests/_pixel_prior_ref.py on every case of
tests/_pixel_prior_cases.py (losses to 1e-5 relative, gradients element-wise within 8 x the float32 restatement's own error
of max|ref|), the zero-weight, exact-copy and constant-image cases bit for bit, accumulation into a pre-filled gradient,
every argument refusal, the engine's step with both terms against the float64 step of tests/_pixel_prior_step.py, zero
weights against an engine without the terms (bit for bit, eager and captured), graph / eager / host-draw equality in
deterministic mode, two engines with all four pixel-space terms stepped alternately against one stepped alone, and
--detail_weight / --tv_weight end to end.

End to end at --max_size 64 --level 1 --max_iter 30, deterministic, on tests/golden's images (DESIGN.md section 26 records the
same figures): E_d, the mean squared D_4 of the written result against the content, with --detail_weight off and at
SUGGESTED_DETAIL_WEIGHT; E_tv, L_tv of the written result, with --tv_weight off and at SUGGESTED_TV_WEIGHT.  Each ratio
bound is the geometric mean of the measured ratio and 1."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _pixel_prior_cases as PC  # noqa: E402
import _pixel_prior_ref as PR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GSCALES = [1.5, 0.5, 2.0]


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ------------------------------------------------------------------ 1. the operators against float64
@pytest.mark.parametrize("ch", [1, 3])
@pytest.mark.parametrize("hw_p", [((1, 1), 1), ((3, 3), 4), ((5, 7), 2), ((42, 63), 4), ((33, 65), 16), ((257, 300), 8)],
                         ids=lambda v: f"{v[0][0]}x{v[0][1]}-p{v[1]}")
def test_pool_mean_matches_float64(hw_p, ch):
    from nn import _ops
    (h, w), p = hw_p
    a = np.random.default_rng(h * w + p).random((h, w, ch)).astype(np.float32)
    got = _ops.pool_mean(_dev(a), p).cpu().numpy()
    ref = PR.pool(a, p)
    assert got.shape == ref.shape == PR.grid(h, w, p) + (ch,)
    err = float(np.abs(got - ref).max())
    same = np.array_equal(got, PR.pool(a, p, np.float32))
    print(f"MEASURE pool_mean {h}x{w} p{p} ch{ch}: max |got - float64| {err:.3e}; the float32 restatement's bits: {same}")
    assert err <= 4 * 2.0 ** -24 * np.log2(max(p * p, 2))        # values in [0, 1]: log2(p^2) additions deep, one division


def _detail_call(P, x, gscales, g, weights="case", loss=None):
    """one strotss_detail_fwd_bwd on the case's content and cell weights -> the (count,) losses"""
    from nn import _ops
    pools = P["pools"]
    cd = _dev(P["c"])
    contents = [_ops.pool_mean(cd, p) for p in pools]
    wts = P["weights"] if weights == "case" else weights
    cells = [None if m is None else _dev(m) for m in wts]
    loss = torch.full((len(pools),), -1.0, device=DEV) if loss is None else loss
    _ops.detail_fwd_bwd(x, pools, contents, cells, gscales, g, loss, ws=_ops.Workspaces())       # a fresh zeroed workspace
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("label", PC.DETAIL_LABELS)
def test_detail_fwd_bwd_matches_float64(label):
    P = PC.detail_inputs(label)
    h, w, pools = P["h"], P["w"], P["pools"]
    gs = GSCALES[:len(pools)]
    xd = _dev(P["x"])
    g = torch.zeros((h, w, 3), device=DEV)
    loss = _detail_call(P, xd, gs, g)
    ref_l, ref_g = PR.detail(P["x"], P["c"], pools, P["weights"], gs)
    got_l, got_g = loss.cpu().numpy().astype(np.float64), g.cpu().numpy().astype(np.float64)
    fam = PR.family(pools)
    scale = float(np.abs(ref_g).max())
    err = float(np.abs(got_g - ref_g).max()) / scale if scale > 0 else float(np.abs(got_g).max())
    rel = max((abs(a - float(b)) / abs(float(b)) if float(b) != 0 else abs(a)) for a, b in zip(got_l, ref_l))
    print(f"MEASURE detail {label}: gradient {err:.3e} of max|ref| (bound {PR.TOL_GRAD[fam]:.1e}), loss {rel:.3e}")
    assert rel <= PR.LOSS_TOL, (got_l, ref_l)
    assert err <= PR.TOL_GRAD[fam], (label, err)
    if P["kind"] != "all_zero" and (h, w) != (1, 1) and label != "3x3-p4-absent":
        assert scale > 0 and all(float(v) > 0 for v in ref_l)
    # accumulation: a pre-filled gradient gives its contents plus the gradient (one float32 addition per pool size), a
    # second call from the same contents the same bits; the losses' bits repeat as well
    g1, g2 = _dev(P["g0"]), _dev(P["g0"])
    l1 = _detail_call(P, xd, gs, g1).clone()
    l2 = _detail_call(P, xd, gs, g2)
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(l1), _bits(loss))
    want = P["g0"].astype(np.float64) + got_g
    ulp = 2.0 ** -23 * float((np.abs(P["g0"]).astype(np.float64) + np.abs(got_g)).max())
    assert float(np.abs(g1.cpu().numpy() - want).max()) <= len(pools) * ulp
    # zero weights: every gscale 0 stores nothing (a -0.0 survives), the losses are still computed
    g3 = _dev(P["g0"])
    g3[0, 0, 0] = -0.0
    before = g3.clone()
    l3 = _detail_call(P, xd, [0.0] * len(pools), g3)
    assert torch.equal(_bits(g3), _bits(before)) and torch.equal(_bits(l3), _bits(loss))
    if P["kind"] in ("zeros_block", "all_zero"):
        # cells whose own and whose neighbours' weights are 0: their pixels bit for bit, a -0.0 included
        dead = np.ones((h, w), dtype=bool)
        for p, m in zip(pools, P["weights"]):
            dead &= PC.dead_pixels(h, w, p, m)
        assert dead.any() and (P["kind"] == "all_zero") == bool(dead.all())
        r, s = np.argwhere(dead)[0]
        g4 = _dev(P["g0"])
        g4[r, s, 1] = -0.0
        before = g4.clone()
        l4 = _detail_call(P, xd, gs, g4)
        dd = torch.from_numpy(dead).to(DEV)
        assert torch.equal(_bits(g4)[dd], _bits(before)[dd])
        if P["kind"] == "all_zero":
            assert float(l4.abs().max()) == 0.0
        else:
            assert not torch.equal(_bits(g4), _bits(before))


@pytest.mark.parametrize("label", ["2x3-p1_2-random", "42x63-p1_4-random", "33x65-p2_16-absent", "257x300-p1_2_8-absent"])
def test_detail_of_a_bit_copy_of_the_content_is_exactly_zero(label):
    P = PC.detail_inputs(label)
    g = _dev(P["g0"])
    g[0, 0, 0] = -0.0
    before = g.clone()
    loss = _detail_call(P, _dev(P["c"]).clone(), GSCALES[:len(P["pools"])], g)
    assert [float(v) for v in loss.tolist()] == [0.0] * len(P["pools"])
    assert torch.equal(_bits(g), _bits(before))


def _tv_call(P, x, gscale, g):
    from nn import _ops
    loss = torch.full((1,), -1.0, device=DEV)
    _ops.tv_fwd_bwd(x, gscale, g, loss, ws=_ops.Workspaces())        # a fresh zeroed workspace
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("label", PC.TV_LABELS)
def test_tv_fwd_bwd_matches_float64(label):
    P = PC.tv_inputs(label)
    h, w = P["h"], P["w"]
    xd, gs = _dev(P["x"]), 1.5
    g = torch.zeros((h, w, 3), device=DEV)
    loss = _tv_call(P, xd, gs, g)
    ref_l, ref_g = PR.tv(P["x"], gscale=gs)
    got_g = g.cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref_g).max())
    err = float(np.abs(got_g - ref_g).max()) / scale if scale > 0 else float(np.abs(got_g).max())
    # (1 x 1: the float64 statement itself leaves sqrt(eps^2) - eps = O(1e-19), the kernel an exact 0)
    rel = abs(loss.item() - float(ref_l)) / abs(float(ref_l)) if abs(float(ref_l)) > 1e-15 else abs(loss.item())
    print(f"MEASURE tv {label}: gradient {err:.3e} of max|ref| (bound {PR.TOL_GRAD['tv']:.1e}), loss {rel:.3e}")
    assert rel <= PR.LOSS_TOL and err <= PR.TOL_GRAD["tv"]
    assert (h, w) == (1, 1) or (scale > 0 and float(ref_l) > 0)
    g1, g2 = _dev(P["g0"]), _dev(P["g0"])
    l1 = _tv_call(P, xd, gs, g1).clone()
    l2 = _tv_call(P, xd, gs, g2)
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(l1), _bits(loss))
    want = P["g0"].astype(np.float64) + got_g
    ulp = 2.0 ** -23 * float((np.abs(P["g0"]).astype(np.float64) + np.abs(got_g)).max())
    assert float(np.abs(g1.cpu().numpy() - want).max()) <= ulp
    # gscale 0 stores nothing; a constant image: loss 0.0 and the gradient bit for bit
    for x_, gs_, exact in ((xd, 0.0, False), (torch.full((h, w, 3), 0.3, device=DEV), gs, True)):
        g3 = _dev(P["g0"])
        g3[0, 0, 0] = -0.0
        before = g3.clone()
        l3 = _tv_call(P, x_, gs_, g3)
        assert torch.equal(_bits(g3), _bits(before))
        assert l3.item() == 0.0 if exact else torch.equal(_bits(l3), _bits(loss))


# ------------------------------------------------------------------ 2. argument refusals: every code, nothing launched
def test_refusals_before_any_launch():
    from nn import _hip
    lib, C = _hip.lib(), _hip.C
    h, w = 8, 12
    img, gimg, pooled = (torch.rand(h * w * 3 + 4, device=DEV) for _ in range(3))
    loss = torch.full((4,), 7.0, device=DEV)
    ws = torch.zeros(4096, dtype=torch.uint8, device=DEV)
    g0, ws0 = gimg.clone(), ws.clone()
    st = _hip.stream_ptr()
    EINVAL, EALIGN, ERANGE = -1, -2, -3
    odd = img.data_ptr() + 4                                  # 4-byte aligned only

    def dset(count=1, pools=(1,), content=None, weight=None):
        s = _hip.DetailSetT()
        s.count = count
        for j, p in enumerate(pools):
            s.pool[j], s.gscale[j] = p, 1.0
            s.content[j] = pooled.data_ptr() if content is None else content
            s.weight[j] = weight
        return s

    def detail(s, img_=img.data_ptr(), h_=h, w_=w, gimg_=gimg.data_ptr(), loss_=loss.data_ptr(), ws_=ws.data_ptr(), byref=True):
        return lib.strotss_detail_fwd_bwd(img_, h_, w_, C.byref(s) if byref else None, gimg_, loss_, ws_, st)

    def tv(img_=img.data_ptr(), h_=h, w_=w, eps=PR.TV_EPS, gimg_=gimg.data_ptr(), loss_=loss.data_ptr(), ws_=ws.data_ptr()):
        return lib.strotss_tv_fwd_bwd(img_, h_, w_, eps, 1.0, gimg_, loss_, ws_, st)

    def pool(img_=img.data_ptr(), h_=h, w_=w, ch=3, p=2, out=pooled.data_ptr()):
        return lib.strotss_pool_mean(img_, h_, w_, ch, p, out, st)

    ok = dset()
    calls = [
        (detail(ok, img_=None), EINVAL), (detail(ok, gimg_=None), EINVAL), (detail(ok, loss_=None), EINVAL),
        (detail(ok, ws_=None), EINVAL), (detail(ok, byref=False), EINVAL), (detail(dset(content=0)), EINVAL),
        (detail(ok, h_=0), EINVAL), (detail(ok, w_=-1), EINVAL), (detail(ok, h_=1 << 15, w_=1 << 15), EINVAL),
        (detail(dset(count=0)), ERANGE), (detail(dset(count=4)), ERANGE), (detail(dset(pools=(3,))), ERANGE),
        (detail(dset(count=2, pools=(4, 1))), ERANGE), (detail(dset(count=2, pools=(2, 2))), ERANGE),
        (detail(dset(pools=(32,))), ERANGE),
        (detail(ok, img_=odd), EALIGN), (detail(ok, gimg_=gimg.data_ptr() + 4), EALIGN), (detail(ok, ws_=ws.data_ptr() + 8), EALIGN),
        (detail(dset(content=pooled.data_ptr() + 4)), EALIGN), (detail(dset(weight=pooled.data_ptr() + 4)), EALIGN),
        (tv(img_=None), EINVAL), (tv(gimg_=None), EINVAL), (tv(loss_=None), EINVAL), (tv(ws_=None), EINVAL),
        (tv(h_=0), EINVAL), (tv(w_=0), EINVAL), (tv(h_=1 << 15, w_=1 << 15), EINVAL),
        (tv(eps=0.0), ERANGE), (tv(eps=-1.0), ERANGE), (tv(eps=float("nan")), ERANGE), (tv(eps=float("inf")), ERANGE),
        (tv(img_=odd), EALIGN), (tv(gimg_=gimg.data_ptr() + 4), EALIGN), (tv(ws_=ws.data_ptr() + 8), EALIGN),
        (pool(img_=None), EINVAL), (pool(out=None), EINVAL), (pool(h_=0), EINVAL), (pool(ch=2), EINVAL),
        (pool(h_=1 << 15, w_=1 << 15), EINVAL), (pool(p=3), ERANGE), (pool(p=0), ERANGE), (pool(p=32), ERANGE),
        (pool(img_=odd), EALIGN), (pool(out=pooled.data_ptr() + 4), EALIGN),
    ]
    for k, (rc, want) in enumerate(calls):
        assert rc == want, (k, rc, want)
    assert lib.strotss_detail_workspace_bytes(0, 5) == lib.strotss_tv_workspace_bytes(5, -1) == 0
    assert lib.strotss_detail_workspace_bytes(1 << 15, 1 << 15) == lib.strotss_tv_workspace_bytes(1 << 15, 1 << 15) == 0
    assert lib.strotss_detail_workspace_bytes(h, w) >= 16 + 4 + 12 * 4 * 6 and lib.strotss_tv_workspace_bytes(h, w) >= 20
    torch.cuda.synchronize()
    assert torch.equal(gimg, g0) and torch.equal(ws, ws0) and float(loss.min()) == float(loss.max()) == 7.0


# ------------------------------------------------------------------ 3. the engine's step
def _engine(lb, deterministic=None, detail_weight="default", tv_weight="default", priors=True):
    """tests/test_hip_step_combos._engine on the rows of _pixel_prior_step, with detail= and tv_weight="""
    import _pixel_prior_step as PS
    import _step_cases as C
    from nn import _ops, engine
    from nn.model import VGGParams
    from oracle import strotss_oracle as O
    row, P = PS.ROWS[lb], PS.problem(lb)
    params = VGGParams(P["weights"], '16', None, DEV)
    cfeat = engine.extract_features(params, P["content"].to(DEV))
    sfeats = [engine.extract_features(params, s.to(DEV)) for s in P["styles"]]
    bw = C.blend_of(row)
    targets = []
    for sets in P["s_idx"]:
        ts = [engine.StyleTarget.build(_ops.hypercol_gather(sf, torch.from_numpy(si).to(DEV), False), si.shape[0], 2179)
              for sf, si in zip(sfeats, sets)]
        targets.append(ts[0] if bw is None else engine.StyleBlend(ts, list(bw)))
    c64, s64 = P["content"].double(), P["styles"][0].double()
    init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    temporal = [engine.TemporalTarget(tg.to(DEV), c.to(DEV), lam) for tg, c, lam in P["temporal"]] or None
    kw = {}
    if priors:
        dw = PS.DETAIL_WEIGHT if detail_weight == "default" else detail_weight
        kw = dict(detail=engine.DetailTarget(P["content"].to(DEV), PS.POOLS, dw, P["wmap"]),
                  tv_weight=PS.TV_WEIGHT if tv_weight == "default" else tv_weight)
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic,
                             content_weight=None if P["wmap"] is None else P["wmap"].to(DEV), temporal=temporal, **kw)


def _indices(lb):
    import _pixel_prior_step as PS
    return [torch.from_numpy(i).to(DEV) for i in PS.problem(lb)["idx"]]


def _labels():
    import _pixel_prior_step as PS
    return PS.LABELS


@pytest.mark.parametrize("lb", _labels())
def test_engine_step_with_both_terms_matches_the_float64_step(lb):
    import _pixel_prior_step as PS
    import test_hip_engine as THE
    from oracle import strotss_oracle as O
    eng = _engine(lb)
    eng.forward_backward(_indices(lb))
    torch.cuda.synchronize()
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(PS.problem(lb)["weights"], dtype=torch.float64)), eng)
    ref = PS.reference_step(lb, vgg=vgg)
    got = dict(eng.losses())
    got["grads"] = [g.detach().cpu().double() for g in eng.gvars]
    sc, gr = PS.step_distance(got, ref)
    print(f"MEASURE step {lb}: scalars {sc:.3e} (bound {PS.TOL_SCALAR:.0e}) gradient {gr:.3e} (bound {PS.GRAD_TOL:.0e}); "
          f"loss_detail {got['loss_detail']:.6e} loss_tv {got['loss_tv']:.6e}")
    assert sc < PS.TOL_SCALAR and gr < PS.GRAD_TOL, (lb, sc, gr)
    assert len(got["loss_detail_terms"]) == len(PS.POOLS) and ("loss_t" in got) == bool(PS.ROWS[lb][3])
    # both terms are real parts of the step
    assert PS.DETAIL_WEIGHT * ref["loss_detail"] > 0.05 * float(ref["loss"])
    assert PS.TV_WEIGHT * ref["loss_tv"] > 0.05 * float(ref["loss"])
    from nn import pixel_terms
    cells = next(t for t in eng._pixel_terms if isinstance(t, pixel_terms.DetailTerm)).cells
    if PS.ROWS[lb][2]:                         # with the map the cells are weighed: some weigh 0, some do not
        assert all(c is not None and float(c.min()) == 0.0 and float(c.max()) > 0 for c in cells)
    else:
        assert cells == [None] * len(PS.POOLS)


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_zero_weights_are_the_step_without_the_terms(graph, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    lb = _labels()[3]                          # the blend with a weight map and a temporal target
    a = _engine(lb, detail_weight=0.0, tv_weight=0.0)
    b = _engine(lb, priors=False)
    idx = _indices(lb)
    if graph:
        a.capture_graph(idx)
        b.capture_graph(idx)
    for _ in range(3):
        a.step(idx)
        b.step(idx)
    torch.cuda.synchronize()
    la, lb_ = a.losses(), b.losses()
    assert la["loss_detail"] > 0 and "loss_detail" not in lb_ and "loss_tv" not in la and "loss_tv" not in lb_
    assert {k: v for k, v in la.items() if k not in ("loss_detail", "loss_detail_terms")} == lb_
    for x, y in zip(a.variables + a.gvars, b.variables + b.gvars):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("regions", [1, 2])
def test_graph_eager_and_host_draw_steps_are_bitwise_alike(regions, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    import _pixel_prior_step as PS
    from nn import rand
    from nn import strotss_utils as SU
    lb = _labels()[2 if regions == 2 else 0]
    row, P = PS.ROWS[lb], PS.problem(lb)
    (h, w), n, seed, steps = row[4], P["n_samples"], 17, 3
    masks = [None]
    if regions == 2:                           # the draw's own regions: the two halves (2048 candidates each)
        m0 = np.zeros((h, w), dtype=bool)
        m0[:, : w // 2] = True
        masks = [m0, ~m0]
    graph, eager, host = _engine(lb), _engine(lb), _engine(lb)
    assert graph.deterministic and graph.enable_device_draw(seed, 0, masks) and eager.enable_device_draw(seed, 0, masks)
    graph.capture_graph()
    rng = rand.PhiloxStream(seed, 0)
    for _ in range(steps):
        graph.step()
        eager.step()
        host.step([torch.from_numpy(SU.make_indices_np(h, w, True, n, rng, m)).to(DEV) for m in masks])
    torch.cuda.synchronize()
    assert graph.losses() == eager.losses() == host.losses()
    assert graph.losses()["loss_detail"] > 0 and graph.losses()["loss_tv"] > 0
    for a, b, c in zip(graph.variables, eager.variables, host.variables):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


def test_engine_refuses_bad_priors_and_sharding():
    from nn import engine
    lb = _labels()[0]
    eng = _engine(lb, priors=False)
    args = (eng.params, eng.content_feat, eng.style_targets, eng.stylized(), 8.0, 10.0, 2e-3)
    c = torch.rand(64, 64, 3)
    DT = engine.DetailTarget
    for bad in (DT(c[:32], (1, 4), 1.0), DT(c, (4, 1), 1.0), DT(c, (3,), 1.0), DT(c, (1, 2, 4, 8), 1.0), DT(c, (1,), -1.0),
                DT(c, (1,), float("nan")), DT(c, (1,), 1.0, torch.rand(32, 64)), DT(c, (1,), 1.0, -torch.ones(64, 64)), "x"):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=384, detail=bad)
    for bad in (-1.0, float("nan"), float("inf"), "1"):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=384, tv_weight=bad)
    with pytest.raises(ValueError):
        engine.StepEngine(*args, sample_size=384, detail=DT(c, (1,), 1.0), dist_group=object())
    with pytest.raises(ValueError):
        engine.StepEngine(*args, sample_size=384, tv_weight=1.0, dist_group=object())


# ------------------------------------------------------------------ 4. all four pixel-space terms in one engine
def test_two_engines_stepped_alternately_are_each_the_engine_stepped_alone():
    """the terms' zeroed workspaces are each engine's own: nothing of them lives in the module-level instance, no two engines
    hold the same buffer, and interleaving two engines' steps changes no bit of either"""
    from _pixel_terms_cases import all_terms_engine, all_terms_indices, all_terms_state
    from nn import _ops
    idx = all_terms_indices(3)
    shared_before = {k: b.data_ptr() for k, b in _ops.workspaces.fixed.items()}
    a, b, alone = all_terms_engine(), all_terms_engine(), all_terms_engine()
    assert [type(t).__name__ for t in a._pixel_terms] == ["TemporalTerm", "DetailTerm", "TVTerm", "PhotoTerm"]
    for i in idx:
        a.step(i)
        b.step(i)
    for i in idx:
        alone.step(i)
    torch.cuda.synchronize()
    want = all_terms_state(alone)
    for eng in (a, b):
        got = all_terms_state(eng)
        assert len(got) == len(want) == 6 + 6 + 1 + 4
        for x, y in zip(got, want):
            assert torch.equal(_bits(x), _bits(y))
    assert a.losses() == b.losses() == alone.losses() and all(a.losses()[k] > 0 for k in ("loss_t", "loss_detail", "loss_tv",
                                                                                             "loss_photo"))
    ptrs = [t.workspace.data_ptr() for eng in (a, b, alone) for t in eng._pixel_terms]
    assert len(set(ptrs)) == 12
    assert all(t.workspace.data_ptr() in {v.data_ptr() for v in eng._ws.fixed.values()}
               for eng in (a, b, alone) for t in eng._pixel_terms)
    assert {k: v.data_ptr() for k, v in _ops.workspaces.fixed.items()} == shared_before


# ------------------------------------------------------------------ 5. end to end
SUGGESTED_DETAIL_WEIGHT, SUGGESTED_TV_WEIGHT = 10.0, 0.1     # DESIGN.md section 26's suggested starting values
DETAIL_RATIO = 0.299        # E_d(on) < ratio * E_d(off): measured 0.000988 / 0.011034 = 0.0895, sqrt(0.0895 * 1)
TV_RATIO = 0.932            # E_tv(on) < ratio * E_tv(off): measured 0.097291 / 0.112037 = 0.868, sqrt(0.868 * 1)


def _run(tmp_path, name, *extra):
    import run_strotss as RS
    from PIL import Image
    out = str(tmp_path / f"{name}.png")
    args = RS.build_parser().parse_args([os.path.join(ROOT, "tests", "golden", "content_im.jpg"),
                                         os.path.join(ROOT, "tests", "golden", "style_im.jpg"), "--max_size", "64", "--level", "1",
                                         "--max_iter", "30", "-o", out] + list(extra))
    RS.run(args)
    result = np.asarray(Image.open(out).convert("RGB"), dtype=np.float64) / 255.0
    content = RS._frame_at_result_size(RS._resolve(args), args.content_path).cpu().numpy().astype(np.float64)
    return result, content


def _e_d(result, content):
    d4 = PR.laplacian(PR.pool(result, 4) - PR.pool(content, 4))
    return float((d4 * d4).mean())


def test_cli_end_to_end(tmp_path, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    off, content = _run(tmp_path, "off")
    assert off.shape == content.shape
    det, _ = _run(tmp_path, "detail", "--detail_weight", f"{SUGGESTED_DETAIL_WEIGHT:g}")
    tvr, _ = _run(tmp_path, "tv", "--tv_weight", f"{SUGGESTED_TV_WEIGHT:g}")
    both, _ = _run(tmp_path, "both", "--detail_weight", str(SUGGESTED_DETAIL_WEIGHT), "--detail_pool", "2", "8", "--tv_weight",
                   f"{SUGGESTED_TV_WEIGHT:g}")
    e_d = (_e_d(off, content), _e_d(det, content))
    e_tv = (float(PR.tv(off)[0]), float(PR.tv(tvr)[0]))
    print(f"MEASURE end to end: E_d off {e_d[0]:.6e} on {e_d[1]:.6e} ratio {e_d[1] / e_d[0]:.4f}; "
          f"E_tv off {e_tv[0]:.6e} on {e_tv[1]:.6e} ratio {e_tv[1] / e_tv[0]:.4f}")
    assert e_d[1] < DETAIL_RATIO * e_d[0], e_d
    assert e_tv[1] < TV_RATIO * e_tv[0], e_tv
    assert np.isfinite(both).all() and not np.array_equal(both, off)
    # zero weights: the run without the flags, pixel for pixel
    zero, _ = _run(tmp_path, "zero", "--detail_weight", "0", "--tv_weight", "0")
    assert np.array_equal(zero, off)
