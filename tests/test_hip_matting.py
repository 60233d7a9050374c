"""The photorealism term on the MI355X: strotss_matting_prepare element-wise against float64 within the
float32 rounding of the stored values, strotss_matting_fwd_bwd against the float64 restatement of tests/_matting_ref.py on
every case of tests/_matting_cases.py -- the gradient element-wise within 8 x the float32 restatement's own worst error of
max|ref|, the scalar within 8 x its error of (1/(3hw)) sum N |p| |p - q| -- what is held bit for bit with a -0.0 planted in
the gradient (gscale 0, the 1 x 1 image, two calls, a side stream), and both entries inside their declared scratch, from
dirty scratch."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import _matting_cases as MC  # noqa: E402
import _matting_ref as MR  # noqa: E402

pytestmark = pytest.mark.gpu

DEV = "cuda"
GSCALE = 1.5
U24 = 2.0 ** -24
# float64 work of the prepare kernel against numpy's: the window mean and second moments (at most 81 terms each), the
# adjugate and the determinant, every step backward stable on a matrix whose pivots are >= eps, so the distance is a small
# multiple of 2^-53 * cond(Sigma) <= 2^-53 * (3 + eps) / eps of the largest entry: 1e-11 of it covers eps = 1e-4
F64_SLACK = 1e-11


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a), dtype=torch.float32, device=DEV)


def _bits(t):
    return t.contiguous().view(torch.int32)


def _call(P, p, gscale, g, ws=None, stats=None):
    from nn import _ops
    guide = _dev(P["I"])
    stats = _ops.matting_prepare(guide, P["r"], P["eps"]) if stats is None else stats
    loss = torch.full((1,), -1.0, device=DEV)
    _ops.matting_fwd_bwd(p, guide, stats, P["r"], gscale, g, loss, ws=ws if ws is not None else _ops.Workspaces())
    torch.cuda.synchronize()
    return loss


@pytest.mark.parametrize("label", [lb for lb in MC.LABELS if MC.BY_LABEL[lb][3] == 1e-4 or MC.BY_LABEL[lb][:2] == (17, 33)])
def test_prepare_matches_float64_within_one_rounding(label):
    from nn import _ops
    P = MC.inputs(label)
    h, w = P["h"], P["w"]
    got = _ops.matting_prepare(_dev(P["I"]), P["r"], P["eps"]).cpu().numpy().astype(np.float64)
    mu, sinv = MR.stats64(P["I"], P["r"], P["eps"])
    ref = np.concatenate([mu, sinv], -1).transpose(2, 0, 1)
    assert got.shape == ref.shape == (9, h, w)
    big = np.concatenate([np.broadcast_to(np.abs(mu).max(-1), (3, h, w)), np.broadcast_to(np.abs(sinv).max(-1), (6, h, w))])
    excess = np.abs(got - ref) - (U24 * np.abs(ref) + F64_SLACK * big)       # gamma_1 = u of the stored value itself
    print(f"MEASURE prepare {label}: worst |got - ref| / (u |ref|) {float((np.abs(got - ref) / (U24 * np.abs(ref) + 1e-300)).max()):.3f}")
    assert float(excess.max()) <= 0, (label, float(excess.max()))


@pytest.mark.parametrize("label", MC.LABELS)
def test_fwd_bwd_matches_float64(label):
    P = MC.inputs(label)
    h, w = P["h"], P["w"]
    pd = _dev(P["p"])
    g = torch.zeros((h, w, 3), device=DEV)
    loss = _call(P, pd, GSCALE, g)
    got_g, got_l = g.cpu().numpy().astype(np.float64) / GSCALE, float(loss.item())
    eg, el = MR.ERR32[P["eps"]]
    gmax = float(np.abs(P["grad"]).max())
    err_g = float(np.abs(got_g - P["grad"]).max()) / gmax if gmax > 0 else float(np.abs(got_g).max())
    err_l = abs(got_l - P["loss"]) / P["scale"] if P["scale"] > 0 else abs(got_l)
    print(f"MEASURE matting {label}: gradient {err_g:.3e} of max|ref| = {err_g / eg:.2f} x ERR32, "
          f"loss {err_l:.3e} of its scale = {err_l / el:.2f} x ERR32")
    assert err_g <= 8 * eg and err_l <= 8 * el, (label, err_g, err_l)
    assert (h, w) == (1, 1) or (gmax > 0 and P["loss"] > 0)
    # accumulation into a pre-filled gradient: its contents plus the gradient, one float32 addition; the same bits twice
    g1, g2 = _dev(P["g0"]), _dev(P["g0"])
    l1 = _call(P, pd, GSCALE, g1).clone()
    l2 = _call(P, pd, GSCALE, g2)
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(l1), _bits(l2)) and torch.equal(_bits(l1), _bits(loss))
    want = P["g0"].astype(np.float64) + g.cpu().numpy().astype(np.float64)
    ulp = 2.0 ** -23 * float((np.abs(P["g0"]).astype(np.float64) + np.abs(want)).max())
    assert float(np.abs(g1.cpu().numpy() - want).max()) <= ulp
    # gscale 0 stores nothing (a -0.0 survives); the scalar is still computed
    g3 = _dev(P["g0"])
    g3[0, 0, 0] = -0.0
    before = g3.clone()
    l3 = _call(P, pd, 0.0, g3)
    assert torch.equal(_bits(g3), _bits(before)) and torch.equal(_bits(l3), _bits(loss))


@pytest.mark.parametrize("r", MC.RADII)
def test_single_pixel_is_exactly_zero(r):
    P = MC.inputs(f"1x1-r{r}-eps0.0001-random")
    g = torch.full((1, 1, 3), -0.0, device=DEV)
    before = g.clone()
    loss = _call(P, _dev(P["p"]), GSCALE, g)
    assert loss.item() == 0.0 and torch.equal(_bits(g), _bits(before))


def test_a_side_stream_gives_the_same_bits():
    from nn import _ops
    P = MC.inputs("42x63-r2-eps0.0001-random")
    pd, guide = _dev(P["p"]), _dev(P["I"])
    g1, g2 = _dev(P["g0"]), _dev(P["g0"])
    g1[0, 0, 0] = g2[0, 0, 0] = -0.0
    l1 = _call(P, pd, GSCALE, g1)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        stats = _ops.matting_prepare(guide, P["r"], P["eps"])
        l2 = torch.full((1,), -1.0, device=DEV)
        _ops.matting_fwd_bwd(pd, guide, stats, P["r"], GSCALE, g2, l2, ws=_ops.Workspaces())
    side.synchronize()
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(l1), _bits(l2))


@pytest.mark.parametrize("label", ["1x3-r4-eps0.0001-random", "17x33-r4-eps0.01-random", "48x64-r1-eps0.0001-random"])
def test_entries_stay_inside_their_declared_scratch_from_dirty_scratch(label):
    import _scratch_guard as SG
    from nn import _hip, _ops
    P = MC.inputs(label)
    h, w = P["h"], P["w"]
    guide, pd = _dev(P["I"]), _dev(P["p"])
    stats, guard = SG.guarded((9, h, w), torch.float32, float("nan"), DEV, "matting stats")
    assert 4 * stats.numel() == _hip.lib().strotss_matting_stats_bytes(h, w)
    _ops.matting_prepare(guide, P["r"], P["eps"], out=stats)
    torch.cuda.synchronize()
    guard.check()
    assert guard.untouched() == 0                      # every statistic written: nothing is read before it is made
    assert torch.equal(_bits(stats), _bits(_ops.matting_prepare(guide, P["r"], P["eps"])))
    ws = SG.GuardedWorkspaces()
    g1, gg = SG.guarded((h, w, 3), torch.float32, 0.0, DEV, "pixel gradient")
    l1 = _call(P, pd, GSCALE, g1, ws=ws, stats=stats).clone()
    first = ws.check()
    g2 = torch.zeros((h, w, 3), device=DEV)
    l2 = _call(P, pd, GSCALE, g2, ws=ws, stats=stats)             # the partials are dirty now, the ticket is back at 0
    gg.check()
    used = ws.check()
    (name, (declared, high)), = used.items()
    print(f"MEASURE scratch {label}: {name} declared {declared} high-water {high}")
    assert declared == _hip.lib().strotss_matting_workspace_bytes(h, w) and high < declared and used == first
    assert int(ws.zeroed("matting", (h, w), declared, DEV)[:4].view(torch.int32).item()) == 0
    assert torch.equal(_bits(g1), _bits(g2)) and torch.equal(_bits(l1), _bits(l2))


def test_refusals_reach_python_and_launch_nothing():
    from nn import _hip, _ops
    P = MC.inputs("9x12-r1-eps0.0001-random")
    guide, pd = _dev(P["I"]), _dev(P["p"])
    g = _dev(P["g0"])
    before = g.clone()
    stats = _ops.matting_prepare(guide, 1, 1e-4)
    loss = torch.full((1,), 7.0, device=DEV)
    for r, eps in ((0, 1e-2), (5, 1e-2), (1, 1e-5), (1, 2.0), (1, float("nan"))):
        with pytest.raises(_hip.StrotssHipError, match="ERANGE"):
            _ops.matting_prepare(guide, r, eps)
    with pytest.raises(_hip.StrotssHipError, match="ERANGE"):
        _ops.matting_fwd_bwd(pd, guide, stats, 5, 1.0, g, loss)
    with pytest.raises(ValueError):
        _ops.matting_prepare(torch.zeros(4, 4, 1, device=DEV), 1, 1e-2)
    torch.cuda.synchronize()
    assert torch.equal(_bits(g), _bits(before)) and loss.item() == 7.0
