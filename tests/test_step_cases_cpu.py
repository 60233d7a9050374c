"""CPU checks of the combined steps ("Combined steps"): the table of tests/_step_cases.py covers what it
claims; the one restatement of tests/_step_ref.py equals each of the five statements it generalises with that statement's one
feature on; every case is conditioned (Sinkhorn's clamps inactive, the sliced sort gaps those of _sliced_cases' own step
problems) and its float32 run stays within a quarter of the bounds tests/test_hip_step_combos.py uses; and five planted
errors each miss those bounds through the comparison function that file calls."""
import functools
import itertools

import pytest
import torch

import _sinkhorn_cases as SKC
import _sinkhorn_ref as SKR
import _sliced_cases as SLC
import _sliced_ref as SLR
import _step_cases as C
import _step_ref as R
import _transport_cases as TC
import _transport_ref as TR
from oracle import strotss_oracle as O


# ------------------------------------------------------------------ the table
def test_table_holds_every_pair_of_factor_values():
    for (i, a), (j, b) in itertools.combinations(enumerate(C.FACTORS), 2):
        for va, vb in itertools.product(a, b):
            assert any(row[i] == va and row[j] == vb for row in C.TABLE), (va, vb)
    for row in C.TABLE:
        assert all(v in f for v, f in zip(row, C.FACTORS)), row


def test_table_holds_the_borrowing_path_on_every_style_side_and_three_targets_on_both_transports():
    for t in ("sinkhorn", "sliced"):
        for side in C.SIDES:
            assert any(row[:3] == (t, side, True) for row in C.TABLE), (t, side)
        assert any(row[0] == t and row[3] == 3 for row in C.TABLE), t
    assert sorted(C.LABELS[i] for i, row in enumerate(C.TABLE) if C.borrowing(row)) == sorted(
        lb for lb in C.LABELS if "-map-" in lb and not lb.startswith("remd"))
    assert 12 <= len(C.TABLE) <= 14 and C.REJECTED == []


def test_sample_counts_are_those_of_the_transport_steps():
    for lb, row in C.ROWS.items():
        P = C.problem(lb)
        if row[1] == "regions" and row[4] == (64, 64):
            assert [(len(i), len(s[0])) for i, s in zip(P["idx"], P["s_idx"])] == [(768, 600), (1024, 1024)]
        elif row[1] == "regions":          # 42 x 64: 504 pixels in the first content region
            assert [(len(i), len(s[0])) for i, s in zip(P["idx"], P["s_idx"])] == [(504, 600), (1024, 1024)]
        else:
            assert [len(i) for i in P["idx"]] == [C.n_samples(row)]
        assert (P["wmap"] is not None) == row[2] and len(P["temporal"]) == row[3]
        if row[2]:                         # some sampled weights are exactly 0
            for i in P["idx"]:
                cj = O.sample_features([P["wmap"].double()[None, :, :, None]], i, True)[:, 0]
                assert int((cj == 0).sum()) > 0 and float(cj.max()) > 0
    assert C.transport_of(C.TABLE[-1]) == ("sliced", SLC.STEP_PROJECTIONS, SLC.STEP_SEED, 0)
    assert tuple(r[1:5] for r in TC.STEPS) == ((64, 64, 384, 0), (42, 64, 300, 4), (64, 64, 1024, 5)) and TC.BLEND_STEP[1:5] == (64, 64, 256, 8)


# ------------------------------------------------------------------ the restatement is the five it generalises
EQ = 1e-12


def _small(masks=False, n_styles=1, weight_map=False, n_targets=0, n=256):
    return R.step_problem(64, 64, n, 1, masks=TC.step_masks(64, 64) if masks else None, n_styles=n_styles,
                          weight_map=weight_map, n_targets=n_targets)


def _equal(got, ref, keys=("loss", "loss_c", "loss_s")):
    for k in keys:
        assert abs(float(got[k]) - float(ref[k])) <= EQ * abs(float(ref[k])), (k, float(got[k]), float(ref[k]))
    assert len(got["grads"]) == len(ref["grads"]) == 6
    for k, (a, b) in enumerate(zip(got["grads"], ref["grads"])):
        assert float((a - b).norm()) <= EQ * float(b.norm()), k


def _oracle_inputs(P):
    """content features, the style sample sets per region and the variables of problem P, as reference_step makes them"""
    vgg = O.VGG(P["weights"], dtype=torch.float64)
    c, styles = P["content"].double(), [s.double() for s in P["styles"]]
    with torch.no_grad():
        cf = [c] + vgg(c)
        sfs = [[s] + vgg(s) for s in styles]
        samples = [[O.sample_features(sf, si, False) for sf, si in zip(sfs, sets)] for sets in P["s_idx"]]
    init = O.make_laplacian(c) + styles[0].mean(dim=(1, 2), keepdim=True)
    return vgg, cf, samples, [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(init)]


@pytest.mark.parametrize("masks", [False, True], ids=["train_step", "train_step_masked"])
def test_restatement_is_the_oracle_step(masks):
    P = _small(masks=masks)
    vgg, cf, samples, variables = _oracle_inputs(P)
    if masks:
        ref = O.train_step_masked(variables, vgg, cf, [s[0] for s in samples], P["idx"], P["alpha"], P["denom"])
    else:
        ref = O.train_step(variables, vgg, cf, samples[0][0], P["idx"][0], P["alpha"], P["denom"])
    got = R.reference_step(P, ("remd",))
    _equal(got, ref)
    assert float(got["loss_t"]) == 0.0 and got["loss_t_terms"] == [] and got["l_remd"] is got["l_transport"]


@pytest.mark.parametrize("side", ["regions", "blend"])
def test_restatement_is_the_sinkhorn_step(side):
    P = _small(masks=side == "regions", n_styles=2 if side == "blend" else 1)
    bw = TC.BLEND_WEIGHTS if side == "blend" else None
    _equal(R.reference_step(P, ("sinkhorn", 10.0, 30), blend_weights=bw), TR.reference_step(P, 10.0, 30, blend_weights=bw))


@pytest.mark.parametrize("side", ["regions", "blend"])
def test_restatement_is_the_sliced_step(side):
    """two regions and a blend: two calls each, the draw number advancing between them"""
    P = _small(masks=side == "regions", n_styles=2 if side == "blend" else 1)
    bw = SLC.BLEND_WEIGHTS if side == "blend" else None
    _equal(R.reference_step(P, ("sliced", 32, 3, 0), blend_weights=bw), SLR.reference_step(P, 32, 3, blend_weights=bw))


def _feature_oracle(P, blend_weights=None):
    """The oracle part of _engine_case in tests/test_hip_content_weight.py, test_hip_temporal.py and test_hip_temporal_long.py
    (those functions build a GPU engine first and cannot run here), transcribed: the weighted content term where P holds a
    map, lambda_j L_j added once per step.  tests/test_hip_step_combos.py compares the restatement with the functions
    themselves."""
    from test_hip_content_weight import weighted_selfsim64
    vgg, cf, samples, variables = _oracle_inputs(P)
    alpha, denom, idx, h, w = P["alpha"], P["denom"], P["idx"], P["h"], P["w"]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_sum = 0.0
    for r, ix in enumerate(idx):
        c_feat = O.sample_features(cf, ix, True)
        p_feat = O.sample_features(pred, ix, True)
        if P["wmap"] is not None:
            cj = O.sample_features([P["wmap"].double()[None, :, :, None]], ix, True)[:, 0]
            lc = weighted_selfsim64(p_feat, c_feat, cj)
        else:
            lc = O.self_similarity(p_feat, c_feat)
        ls = (sum(wk * O.style_loss(s, p_feat, alpha) for wk, s in zip(blend_weights, samples[r])) if blend_weights
              else O.style_loss(samples[r][0], p_feat, alpha))
        loss = loss + (alpha * lc + ls) / denom
        lc_sum = lc_sum + lc
    loss = loss / len(idx)
    lts = [(c.double()[None, :, :, None] * (img - tg.double()[None]) ** 2).sum() / (3 * h * w) for tg, c, _ in P["temporal"]]
    if len(lts) == 1:
        total = loss + P["temporal"][0][2] * lts[0]
    else:
        total = loss + sum(lam * lt for (_, _, lam), lt in zip(P["temporal"], lts))
    grads = torch.autograd.grad(total, variables)
    return dict(loss=float(total.detach()), loss_c=float(lc_sum.detach()) / len(idx),
                loss_t=float(sum(lt.detach() for lt in lts)), terms=[float(lt.detach()) for lt in lts],
                grads=grads)


@pytest.mark.parametrize("kw", [dict(weight_map=True), dict(weight_map=True, masks=True), dict(weight_map=True, n_styles=2),
                                dict(n_targets=1), dict(n_targets=3), dict(n_targets=3, masks=True)],
                         ids=["map", "map-regions", "map-blend", "one-target", "three-targets", "three-targets-regions"])
def test_restatement_is_the_weight_map_and_temporal_oracles(kw):
    P = _small(**kw)
    bw = (0.6, 0.4) if kw.get("n_styles") == 2 else None
    ref = _feature_oracle(P, bw)
    got = R.reference_step(P, ("remd",), blend_weights=bw)
    _equal(got, ref, keys=("loss", "loss_c") + (("loss_t",) if P["temporal"] else ()))
    assert len(got["loss_t_terms"]) == len(ref["terms"])
    for a, b in zip(got["loss_t_terms"], ref["terms"]):
        assert abs(float(a) - b) <= EQ * abs(b)


# ------------------------------------------------------------------ conditioning and the float32 yardstick
@functools.lru_cache(maxsize=None)
def ref64(lb):
    """(float64 step, its probes) of a case: computed once, shared, left unchanged"""
    row, probe = C.ROWS[lb], []
    return R.reference_step(C.problem(lb), C.transport_of(row), blend_weights=C.blend_of(row), probe=probe), probe


@functools.lru_cache(maxsize=None)
def _gap_asked():
    """What _sliced_cases asks of its step problems' sort gaps: nothing by value (they hold near-ties and are compared in
    norm) -- so the smallest gap that table's own problems hold, measured here the same way, is what a new case must reach."""
    worst = float("inf")
    for lb, h, w, n, seed, masked in SLC.STEPS + [SLC.BLEND_STEP]:
        bw = SLC.BLEND_WEIGHTS if lb == SLC.BLEND_STEP[0] else None
        P = R.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None, n_styles=2 if bw else 1)
        probe = []
        R.reference_step(P, ("sliced", SLC.STEP_PROJECTIONS, SLC.STEP_SEED, 0), blend_weights=bw, probe=probe)
        worst = min([worst] + [SLR.min_gap(s.numpy(), p.numpy(), g.numpy()) for s, p, g in probe])
    return worst


@pytest.mark.parametrize("lb", C.LABELS)
def test_case_is_conditioned(lb):
    row = C.ROWS[lb]
    ref, probe = ref64(lb)
    assert len(probe) == {"one": 1, "blend": 2, "regions": 2}[row[1]]
    if row[0] == "sinkhorn":
        for s, p, _ in probe:
            kv, ktu = SKR.clamp_arguments(s.numpy(), p.numpy(), "cosine", C.SINKHORN_L, C.SINKHORN_T)
            print(f"MEASURE clamp {lb} {min(kv.min(), ktu.min()):.3e}")
            assert min(kv.min(), ktu.min()) >= SKC.CLAMP_CLEAR
    if row[0] == "sliced":
        for s, p, g in probe:
            gap = SLR.min_gap(s.numpy(), p.numpy(), g.numpy())
            print(f"MEASURE gap {lb} {gap:.3e} asked {_gap_asked():.3e}")
            assert gap >= _gap_asked() > 0
    if row[3]:                             # the temporal part is a real share of the step, every term present
        share = sum(lam * float(lt) for (_, _, lam), lt in zip(C.problem(lb)["temporal"], ref["loss_t_terms"]))
        assert share > 0.05 * float(ref["loss"]) and min(float(lt) for lt in ref["loss_t_terms"]) > 0


@pytest.mark.parametrize("threads", [1, None], ids=["one_thread", "default_threads"])
def test_float32_step_stays_within_a_quarter_of_the_bounds(threads):
    """every case of the table, with one thread and with the machine's own count"""
    before = torch.get_num_threads()
    if threads is not None:
        torch.set_num_threads(threads)
    try:
        worst = {}
        for lb, row in C.ROWS.items():
            r32 = R.reference_step(C.problem(lb), C.transport_of(row), torch.float32, blend_weights=C.blend_of(row))
            worst[lb] = R.step_distance(r32, ref64(lb)[0], row[0])
            print(f"MEASURE step32 {lb} scalar {worst[lb][0]:.3e} grad {worst[lb][1]:.3e}")
    finally:
        torch.set_num_threads(before)
    assert sorted(R.STEP32) == sorted(C.LABELS)
    for lb, (sc, gr) in worst.items():
        assert sc <= R.TOL_SCALAR / 4 and gr <= R.GRAD_TOL / 4, (lb, sc, gr)
    assert (R.TOL_SCALAR, R.GRAD_TOL) == (5e-5, 5e-3)


# ------------------------------------------------------------------ planted errors
def planted_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, *, transport,
                 weight_map, temporal, plant=None):
    """A copy of _step_ref.train_step with one error planted (plant None: the copy itself, shown equal to the original):
      map_ignored_off_remd     the weight map ignored when the transport is not remd
      blend_transport_weight_1 the transport term of a blend taken with weight 1 instead of w_k
      temporal_over_regions    the temporal gradient divided by the region count
      second_region_draw_t0    the second region's sliced directions taken from draw t0 instead of t0 + 1
      temporal_after_fold      the temporal term added after the fold adjoint: level 0 correct, levels >= 1 without it"""
    kind = transport[0]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_a = ls_a = lt_a = 0.0
    r = len(indices_per_region)
    call = int(transport[3]) if kind == "sliced" else 0
    use_map = weight_map is not None and not (plant == "map_ignored_off_remd" and kind != "remd")
    for region, (idx, style) in enumerate(zip(indices_per_region, styles_per_region)):
        c_feat = O.sample_features(content_feat, idx, True)
        p_feat = O.sample_features(pred, idx, True)
        if use_map:
            cj = O.sample_features([weight_map.to(img.dtype)[None, :, :, None]], idx, True)[:, 0]
            lc = R.weighted_selfsim64(p_feat, c_feat, cj)
        else:
            lc = O.content_loss(c_feat, p_feat)
        ls = tr = 0.0
        for w, s in (style if isinstance(style, list) else [(1.0, style)]):
            draw = int(transport[3]) if plant == "second_region_draw_t0" and region == 1 else call
            signs = SLR.signs_of(transport[2], draw, transport[1], p_feat.shape[1], p_feat.dtype) if kind == "sliced" else None
            total, term = R.style_terms(s, p_feat, alpha, transport, signs)
            if plant == "blend_transport_weight_1":
                live = (O.sinkhorn_knopp(s, p_feat, "cosine", float(transport[1]), int(transport[2])) if kind == "sinkhorn"
                        else SLR.sliced_loss(s, p_feat, signs) if kind == "sliced" else O.relaxed_emd(s, p_feat))
                total, term = total + (1.0 - w) / w * live, term / w
            ls, tr = ls + w * total, tr + w * term
            call += 1
        loss = loss + (alpha * lc + ls) / loss_denom
        lc_a, ls_a, lt_a = lc_a + lc, ls_a + ls, lt_a + tr
    loss = loss / r
    lts = R.temporal_terms(img, temporal)
    t_sum = sum(lam * lt for (_, _, lam), lt in zip(temporal, lts)) if lts else None
    if plant == "temporal_over_regions":
        t_sum = t_sum / r + (t_sum - t_sum / r).detach()
    total = loss if t_sum is None else loss + t_sum
    if plant == "temporal_after_fold":
        grads = list(torch.autograd.grad(total, variables, retain_graph=True)[:1]) + list(torch.autograd.grad(loss, variables)[1:])
    else:
        grads = list(torch.autograd.grad(total, variables))
    term = (lt_a / r).detach()
    return {"loss": total.detach(), "loss_c": (lc_a / r).detach(), "loss_s": (ls_a / r).detach(), R.TRANSPORT_KEY[kind]: term,
            "l_transport": term, "loss_t": sum(lt.detach() for lt in lts) if lts else torch.zeros((), dtype=img.dtype),
            "loss_t_terms": [lt.detach() for lt in lts], "grads": grads, "img": img.detach()}


PLANTS = {
    "map_ignored_off_remd": "sinkhorn-one-map-t0-64x64",
    "blend_transport_weight_1": "sliced-blend-map-t1-64x64",
    "temporal_over_regions": "sinkhorn-regions-map-t1-64x64",
    "second_region_draw_t0": "sliced-regions-nomap-t0-64x64",
    "temporal_after_fold": "sliced-one-nomap-t3-64x64",
}


def _planted(lb, plant):
    row = C.ROWS[lb]
    return R.reference_step(C.problem(lb), C.transport_of(row), blend_weights=C.blend_of(row),
                            step=functools.partial(planted_step, plant=plant))


def test_the_copy_without_a_plant_is_the_restatement():
    lb = "sliced-blend-map-t1-64x64"
    got, ref = _planted(lb, None), ref64(lb)[0]
    ok, sc, gr = R.within_bounds(got, ref, "sliced")
    assert ok and sc <= EQ and gr <= EQ


@pytest.mark.parametrize("plant", list(PLANTS))
def test_planted_error_misses_the_bounds(plant):
    lb = PLANTS[plant]
    assert lb in C.ROWS
    kind = C.ROWS[lb][0]
    got, ref = _planted(lb, plant), ref64(lb)[0]
    ok, sc, gr = R.within_bounds(got, ref, kind)
    print(f"MEASURE plant {plant} on {lb}: scalar {sc:.3e} of {R.TOL_SCALAR:.0e}, grad {gr:.3e} of {R.GRAD_TOL:.0e}; "
          f"levels {['%.2e' % g for g in R.step_grads(got, ref)]}")
    assert not ok
    if plant == "temporal_after_fold":
        # level 0 alone -- what the weight-map and temporal step tests compare -- passes: the reason all levels are compared
        ok0, sc0, gr0 = R.within_bounds(got, ref, kind, levels=[0])
        assert ok0 and gr0 <= EQ and sc0 <= EQ
        assert min(R.step_grads(got, ref)[1:]) > R.GRAD_TOL
    if plant == "temporal_over_regions":       # no scalar tells: only the gradients do
        assert sc <= EQ and gr > R.GRAD_TOL
