"""ONE float64 restatement of the train step that takes every option StepEngine combines ("Combined
steps"): the transport of the style term (relaxed EMD, Sinkhorn, sliced), one style / a blend / several regions, a
content-weight map and 0..4 temporal targets.  It generalises five statements that each know one feature --
oracle.train_step / train_step_masked, _transport_ref.train_step, _sliced_ref.train_step and the _engine_case oracles of
tests/test_hip_content_weight.py, test_hip_temporal.py and test_hip_temporal_long.py -- and is built from their parts;
tests/test_step_cases_cpu.py shows it equal to each of them to 1e-12 with that one feature on.

    loss = mean_r (alpha * Lc_r + Ls_r) / loss_denom  +  sum_j lambda_j * L_j
    Lc_r   self_similarity of region r's samples; with a weight map, weighted_selfsim64 with the map at the samples
    Ls_r   sum_k w_k (moment + transport + palette / max(alpha, 1)) over the region's styles (one style: w = 1)
    L_j    (1 / (3 h w)) sum_p c_j(p) |img(p) - target_j(p)|^2: added once per step, not averaged over the regions
The sliced term's call number c (regions in order, within a region the styles of a blend in order) takes the directions of
draw t0 + c, as the engine's device counter does.

Bounds of a step (tests/test_hip_step_combos.py): the project's existing ones, _transport_ref.TOL_SCALAR on every scalar
relative to max(1, |ref|) and GRAD_TOL on every pyramid level's gradient in relative L2.  They stand for a case of
tests/_step_cases.py because this restatement's own float32 run on the CPU stays within a quarter of both
(tests/test_step_cases_cpu.py asserts it; STEP32 holds what it printed)."""
import torch

import _sliced_ref as SLR
import _transport_ref as TR
from oracle import strotss_oracle as O

TOL_SCALAR, GRAD_TOL = TR.TOL_SCALAR, TR.GRAD_TOL
TRANSPORT_KEY = {"remd": "l_remd", "sinkhorn": "l_sinkhorn", "sliced": "l_sliced"}

# float32-CPU distance from float64 per case of _step_cases.TABLE, as printed by tests/test_step_cases_cpu.py with one thread
# and with eight: (scalars relative to max(1, |ref|), worst level's gradient in relative L2), the larger of the two runs.
# Recorded, not asserted to the digit: the float32 run's sums depend on the machine and its thread count.
STEP32 = {
    "remd-one-map-t1-64x64": (3.5e-08, 1.9e-06),
    "remd-regions-map-t3-64x64": (3.0e-08, 1.5e-05),
    "remd-blend-nomap-t0-42x64": (2.2e-08, 5.0e-06),
    "sinkhorn-one-map-t0-64x64": (3.7e-08, 3.6e-06),
    "sinkhorn-one-nomap-t1-42x64": (2.4e-08, 2.3e-06),
    "sinkhorn-blend-map-t3-64x64": (2.4e-08, 2.2e-04),
    "sinkhorn-regions-map-t1-64x64": (4.7e-08, 1.9e-05),
    "sinkhorn-regions-nomap-t3-42x64": (2.6e-08, 1.8e-05),
    "sliced-one-map-t0-42x64": (4.4e-08, 1.3e-05),
    "sliced-one-nomap-t3-64x64": (3.0e-08, 2.6e-06),
    "sliced-blend-map-t1-64x64": (3.1e-08, 2.7e-04),
    "sliced-regions-map-t3-64x64": (4.7e-08, 1.5e-05),
    "sliced-regions-nomap-t0-64x64": (2.4e-08, 4.8e-05),
}


def weighted_selfsim64(x, y, c):
    from test_hip_content_weight import weighted_selfsim64 as f
    return f(x, y, c)


def style_terms(target, prediction, alpha, transport, signs=None):
    """(style loss, its transport term alone and detached) of one sample set"""
    kind = transport[0]
    if kind == "remd":
        total = O.style_loss(target, prediction, alpha)
    elif kind == "sinkhorn":
        total = TR.style_loss_sinkhorn(target, prediction, alpha, transport[1], transport[2])
    elif kind == "sliced":
        total = SLR.style_loss_sliced(target, prediction, alpha, signs)
    else:
        raise ValueError(transport)
    with torch.no_grad():
        if kind == "remd":
            term = O.relaxed_emd(target, prediction)
        elif kind == "sinkhorn":
            term = O.sinkhorn_knopp(target, prediction, "cosine", float(transport[1]), int(transport[2]))
        else:
            term = SLR.sliced_loss(target, prediction, signs)
    return total, term


def temporal_terms(img, temporal):
    """[L_j]: the unweighted terms of the (target, certainty, lambda) triples"""
    h, w = int(img.shape[1]), int(img.shape[2])
    return [(c.to(img.dtype)[None, :, :, None] * (img - tg.to(img.dtype)[None]) ** 2).sum() / (3 * h * w) for tg, c, _ in temporal]


def train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, *, transport=("remd",),
               weight_map=None, temporal=(), probe=None):
    """styles_per_region[r]: a sample set, or [(weight, sample set), ...] of a blend.  transport: ("remd",),
    ("sinkhorn", l, T) or ("sliced", n_proj, seed, t0).  weight_map: None or an (h, w) tensor.  temporal: 0..4
    (target (h, w, 3), certainty (h, w), lambda) triples.  probe: a list that receives (style rows, prediction rows, signs)
    of every (region, style) call, detached, for the conditioning checks.
    Returns loss, loss_c, loss_s (means over the regions; loss with the temporal sum), the transport term under
    TRANSPORT_KEY[kind] and under "l_transport", loss_t = sum_j L_j, loss_t_terms, and grads of EVERY pyramid level."""
    kind = transport[0]
    temporal = list(temporal)
    assert len(temporal) <= 4
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_a = ls_a = lt_a = 0.0
    r = len(indices_per_region)
    call = int(transport[3]) if kind == "sliced" else 0
    w64 = None if weight_map is None else weight_map.to(img.dtype)[None, :, :, None]
    for idx, style in zip(indices_per_region, styles_per_region):
        c_feat = O.sample_features(content_feat, idx, True)
        p_feat = O.sample_features(pred, idx, True)
        if w64 is None:
            lc = O.content_loss(c_feat, p_feat)
        else:
            lc = weighted_selfsim64(p_feat, c_feat, O.sample_features([w64], idx, True)[:, 0])
        blend = style if isinstance(style, list) else [(1.0, style)]
        ls = tr = 0.0
        for w, s in blend:
            signs = SLR.signs_of(transport[2], call, transport[1], p_feat.shape[1], p_feat.dtype) if kind == "sliced" else None
            total, term = style_terms(s, p_feat, alpha, transport, signs)
            if probe is not None:
                probe.append((s.detach(), p_feat.detach(), signs))
            ls, tr = ls + w * total, tr + w * term
            call += 1
        loss = loss + (alpha * lc + ls) / loss_denom
        lc_a, ls_a, lt_a = lc_a + lc, ls_a + ls, lt_a + tr
    loss = loss / r
    lts = temporal_terms(img, temporal)
    if lts:
        loss = loss + sum(lam * lt for (_, _, lam), lt in zip(temporal, lts))
    grads = torch.autograd.grad(loss, variables)
    term = (lt_a / r).detach()
    return {"loss": loss.detach(), "loss_c": (lc_a / r).detach(), "loss_s": (ls_a / r).detach(), TRANSPORT_KEY[kind]: term,
            "l_transport": term, "loss_t": sum(lt.detach() for lt in lts) if lts else torch.zeros((), dtype=img.dtype),
            "loss_t_terms": [lt.detach() for lt in lts], "grads": list(grads), "img": img.detach()}


def step_problem(h, w, n_samples, seed, masks=None, n_styles=1, weight_map=False, n_targets=0):
    """_transport_ref.step_problem (same images, same make_indices draws) with "wmap": the ramp_map of the weight-map test
    (a band of exact zeros) or None, and "temporal": n_targets (target, certainty, lambda) triples, the _long_targets and
    LAMS of the long-term test (the nearest frame blind on the left quarter)"""
    P = TR.step_problem(h, w, n_samples, seed, masks=masks, n_styles=n_styles)
    P["wmap"] = None
    if weight_map:
        from test_hip_content_weight import ramp_map
        P["wmap"] = ramp_map(h, w)
    P["temporal"] = []
    if n_targets:
        from test_hip_temporal_long import LAMS, _long_targets
        P["temporal"] = [(tg, c, lam) for (tg, c), lam in zip(_long_targets(h, w, n_targets), LAMS)]
        assert len(P["temporal"]) == n_targets
    return P


def reference_step(P, transport, dtype=torch.float64, blend_weights=None, vgg=None, step=None, probe=None):
    """train_step (or `step`, a function of its signature) of problem P in `dtype` on the CPU (vgg: a network to use in place
    of the plain one, float64 only)"""
    net = O.VGG(P["weights"], dtype=dtype) if vgg is None else vgg
    plain = O.VGG(P["weights"], dtype=dtype)
    c, styles = P["content"].to(dtype), [s.to(dtype) for s in P["styles"]]
    with torch.no_grad():
        cf = [c] + plain(c)
        sfs = [[s] + plain(s) for s in styles]
        per_region = []
        for sets in P["s_idx"]:
            samples = [O.sample_features(sf, si, False) for sf, si in zip(sfs, sets)]
            per_region.append(samples[0] if blend_weights is None else list(zip(blend_weights, samples)))
    init = O.make_laplacian(c) + styles[0].mean(dim=(1, 2), keepdim=True)
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]
    kw = {} if probe is None else dict(probe=probe)
    out = (step or train_step)(variables, net, cf, per_region, P["idx"], P["alpha"], P["denom"], transport=transport,
                               weight_map=P["wmap"], temporal=P["temporal"], **kw)
    out["init"] = init
    return out


def step_scalars(got, ref, kind):
    """{name: distance relative to max(1, |ref|)} of every scalar of a step: loss, loss_c, loss_s, the transport term under its
    own key, and with temporal targets loss_t and every entry of loss_t_terms (`got` must hold as many as `ref`; a one-target
    engine reports none, its loss_t is the term)"""
    def rel(a, b):
        return abs(float(a) - float(b)) / max(1.0, abs(float(b)))
    out = {k: rel(got[k], ref[k]) for k in ("loss", "loss_c", "loss_s", TRANSPORT_KEY[kind])}
    n = len(ref["loss_t_terms"])
    if n:
        out["loss_t"] = rel(got["loss_t"], ref["loss_t"])
        terms = got.get("loss_t_terms") or []
        if n > 1 or terms:
            assert len(terms) == n, (len(terms), n)
            for j, (a, b) in enumerate(zip(terms, ref["loss_t_terms"])):
                out[f"loss_t_terms[{j}]"] = rel(a, b)
    return out


def step_grads(got, ref):
    """[relative L2 distance] of every pyramid level's gradient"""
    assert len(got["grads"]) == len(ref["grads"])
    return [float((torch.as_tensor(a).double().cpu() - b.double()).norm() / b.double().norm())
            for a, b in zip(got["grads"], ref["grads"])]


def step_distance(got, ref, kind, levels=None):
    """_transport_ref.step_distance extended to the transport term, loss_t, its terms and (as there) all levels: (worst scalar
    distance, worst level's relative L2).  levels: compare these levels only (the planted-error test's level-0 comparison)."""
    sc, gr = TR.step_distance(got, ref)
    sc = max(sc, max(step_scalars(got, ref, kind).values()))
    per_level = step_grads(got, ref)
    if levels is not None:
        gr = max(per_level[k] for k in levels)
    return sc, gr


def within_bounds(got, ref, kind, levels=None):
    """the comparison of tests/test_hip_step_combos.py: (passes, worst scalar, worst gradient level) against TOL_SCALAR and
    GRAD_TOL; the planted errors of tests/test_step_cases_cpu.py go through this same function"""
    sc, gr = step_distance(got, ref, kind, levels)
    return bool(sc < TOL_SCALAR and gr < GRAD_TOL), sc, gr
