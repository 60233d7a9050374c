"""One engine with all four pixel-space terms on (nn/pixel_terms.py), shared by tests/test_hip_pixel_prior.py and the engine row
of tests/test_hip_scratch_contracts.py: tests/_step_ref.py's problem at 42 x 64 with two temporal targets, the detail term at
pools (1, 4) with a cell map, TV and the photo term at radius 1, deterministic."""
import functools

import numpy as np
import torch

DEV = "cuda"
ALL_TERMS_HW = (42, 64)     # 2688 pixels: two full 1024-pixel blocks and a partial one; 42 = 10 * 4 + 2: partial cells at pool 4
PHOTO_WEIGHT = 40.0         # tests/_matting_step.py's for its 42 x 64 row


@functools.lru_cache(maxsize=None)
def all_terms_problem():
    """_step_ref.step_problem at ALL_TERMS_HW with a weight map (the detail term's cell map) and two temporal targets; cached,
    read-only"""
    import _step_ref as R
    return R.step_problem(*ALL_TERMS_HW, 300, 4, weight_map=True, n_targets=2)


def all_terms_indices(steps, seed=6):
    from oracle import strotss_oracle as O
    P, rng = all_terms_problem(), np.random.default_rng(seed)
    idx = [[torch.from_numpy(O.make_indices(P["h"], P["w"], True, P["n_samples"], rng)).to(DEV)] for _ in range(steps)]
    assert all(int(i[0].shape[0]) == P["n_samples"] for i in idx)       # every set has the count of the first: a graph replays
    return idx


def all_terms_engine():
    """a deterministic engine on all_terms_problem() with every pixel-space term on: two temporal targets, the detail term at
    pools (1, 4) with a cell map, TV, the photo term at radius 1"""
    import _matting_step as MS
    import _pixel_prior_step as PS
    from nn import _ops, engine
    from nn.model import VGGParams
    from oracle import strotss_oracle as O
    P = all_terms_problem()
    params = VGGParams(P["weights"], '16', None, DEV)
    content = P["content"].to(DEV)
    cfeat, sfeat = engine.extract_features(params, content), engine.extract_features(params, P["styles"][0].to(DEV))
    si = P["s_idx"][0][0]
    target = engine.StyleTarget.build(_ops.hypercol_gather(sfeat, torch.from_numpy(si).to(DEV), False), si.shape[0], 2179)
    init = O.make_laplacian(P["content"].double()) + P["styles"][0].double().mean(dim=(1, 2), keepdim=True)
    return engine.StepEngine(params, cfeat, [target], init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=True,
                             temporal=[engine.TemporalTarget(tg.to(DEV), c.to(DEV), lam) for tg, c, lam in P["temporal"]],
                             detail=engine.DetailTarget(content, (1, 4), PS.DETAIL_WEIGHT, P["wmap"]), tv_weight=PS.TV_WEIGHT,
                             photo=engine.PhotoTarget(content, 1, MS.EPS, PHOTO_WEIGHT))


def all_terms_state(eng):
    """variables, gradients, the regions' scalars and every pixel-space term's scalars"""
    return [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()] + \
        [t.loss.clone() for t in eng._pixel_terms]
