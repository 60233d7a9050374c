"""The step with the photorealism term on the MI355X (StepEngine(photo=)) against the step composed in
float64 by tests/_matting_step.py (64 x 64 and 42 x 64, one and two regions, a blend with a weight map, with and without the
detail and TV terms and a temporal target) within TOL_SCALAR and GRAD_TOL; weight 0 against an engine built without the
argument, bit for bit, eager and captured; graph, eager and host-draw steps bitwise alike in deterministic mode; the
constructor's refusals."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _matting_step as MS  # noqa: E402
import _pixel_prior_step as PS  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"


def _bits(t):
    return t.contiguous().view(torch.int32)


def _engine(lb, deterministic=None, photo="case"):
    """the engine of case `lb`; photo: "case" (the case's weight), a weight, or None (built without the argument)"""
    import _step_cases as C
    from nn import _ops, engine
    from nn.model import VGGParams
    from oracle import strotss_oracle as O
    row_lb, priors, weight = MS.BY_LABEL[lb]
    row, P = PS.ROWS[row_lb], PS.problem(row_lb)
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
        kw = dict(detail=engine.DetailTarget(P["content"].to(DEV), PS.POOLS, PS.DETAIL_WEIGHT, P["wmap"]), tv_weight=PS.TV_WEIGHT)
    if photo is not None:
        kw["photo"] = engine.PhotoTarget(P["content"].to(DEV), MS.RADIUS, MS.EPS, weight if photo == "case" else photo)
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic,
                             content_weight=None if P["wmap"] is None else P["wmap"].to(DEV), temporal=temporal, **kw)


def _indices(lb):
    return [torch.from_numpy(i).to(DEV) for i in MS.problem(lb)["idx"]]


@pytest.mark.parametrize("lb", MS.LABELS)
def test_engine_step_with_the_term_matches_the_float64_step(lb):
    import test_hip_engine as THE
    from oracle import strotss_oracle as O
    eng = _engine(lb)
    eng.forward_backward(_indices(lb))
    torch.cuda.synchronize()
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(MS.problem(lb)["weights"], dtype=torch.float64)), eng)
    ref = MS.reference_step(lb, vgg=vgg)
    got = dict(eng.losses())
    got["grads"] = [g.detach().cpu().double() for g in eng.gvars]
    sc, gr = MS.step_distance(lb, got, ref)
    share = MS.photo_share(lb, ref)
    print(f"MEASURE step {lb}: scalars {sc:.3e} (bound {MS.TOL_SCALAR:.0e}) gradient {gr:.3e} (bound {MS.GRAD_TOL:.0e}); "
          f"loss_photo {got['loss_photo']:.6e}, {share:.3f} of the loss")
    assert sc < MS.TOL_SCALAR and gr < MS.GRAD_TOL, (lb, sc, gr)
    assert 0.10 <= share <= 0.30
    assert ("loss_detail" in got) == ("loss_tv" in got) == MS.BY_LABEL[lb][1]


@pytest.mark.parametrize("graph", [False, True], ids=["eager", "captured"])
def test_weight_zero_is_the_step_without_the_term(graph, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    lb = MS.LABELS[1]                          # 42 x 64 with the detail, TV and temporal terms
    a, b = _engine(lb, photo=0.0), _engine(lb, photo=None)
    idx = _indices(lb)
    if graph:
        a.capture_graph(idx)
        b.capture_graph(idx)
    for _ in range(3):
        a.step(idx)
        b.step(idx)
    torch.cuda.synchronize()
    la, lb_ = a.losses(), b.losses()
    assert la["loss_photo"] > 0 and "loss_photo" not in lb_
    assert {k: v for k, v in la.items() if k != "loss_photo"} == lb_
    for x, y in zip(a.variables + a.gvars, b.variables + b.gvars):
        assert torch.equal(_bits(x), _bits(y))


@pytest.mark.parametrize("regions", [1, 2])
def test_graph_eager_and_host_draw_steps_are_bitwise_alike(regions, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    from nn import rand
    from nn import strotss_utils as SU
    lb = MS.LABELS[2 if regions == 2 else 0]
    row, P = PS.ROWS[MS.BY_LABEL[lb][0]], MS.problem(lb)
    (h, w), n, seed, steps = row[4], P["n_samples"], 17, 3
    masks = [None]
    if regions == 2:                           # the draw's own regions: the two halves
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
    assert graph.losses()["loss_photo"] > 0
    for a, b, c in zip(graph.variables, eager.variables, host.variables):
        assert torch.equal(_bits(a), _bits(b)) and torch.equal(_bits(a), _bits(c))


def test_engine_refuses_bad_targets_and_sharding():
    from nn import engine
    eng = _engine(MS.LABELS[0], photo=None)
    args = (eng.params, eng.content_feat, eng.style_targets, eng.stylized(), 8.0, 10.0, 2e-3)
    c = torch.rand(64, 64, 3)
    PT = engine.PhotoTarget
    for bad in (PT(c[:32], 1, 1e-4, 1.0), PT(c, 0, 1e-4, 1.0), PT(c, 5, 1e-4, 1.0), PT(c, 1, 1e-5, 1.0), PT(c, 1, 2.0, 1.0),
                PT(c, 1, 1e-4, -1.0), PT(c, 1, 1e-4, float("nan")), "x"):
        with pytest.raises(ValueError):
            engine.StepEngine(*args, sample_size=384, photo=bad)
    with pytest.raises(ValueError, match="one GPU"):
        engine.StepEngine(*args, sample_size=384, photo=PT(c, 1, 1e-4, 1.0), dist_group=object())
