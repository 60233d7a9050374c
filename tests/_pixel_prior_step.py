"""Steps with the pixel-space priors (StepEngine(detail=, tv_weight=)): the float64 train step of
tests/_step_ref.py plus the two terms of tests/_pixel_prior_ref.py on the folded image,

    loss = (step of _step_ref)  +  DETAIL_WEIGHT * sum_p L_p  +  TV_WEIGHT * L_tv,

their pixel gradients taken through the fold's adjoint by torch autograd.  The rows are _pixel_prior_cases.STEP_TABLE in the
format of tests/_step_cases.py, so its helpers apply; with a content-weight map the cells weigh m_p = P_p(map).  The weights
are chosen so that each term is a real share of the loss at the first step, a third and a quarter of it:
tests/test_pixel_prior_cpu.py and tests/test_hip_pixel_prior.py assert that each is above 5 %.

Bounds: _step_ref.TOL_SCALAR on every scalar relative to max(1, |ref|) and GRAD_TOL on every pyramid level's gradient in
relative L2; tests/test_pixel_prior_cpu.py holds this restatement's own float32 run within a quarter of both."""
import functools

import numpy as np
import torch

import _pixel_prior_cases as PC
import _pixel_prior_ref as PR
import _step_cases as C
import _step_ref as R
from oracle import strotss_oracle as O

TOL_SCALAR, GRAD_TOL = R.TOL_SCALAR, R.GRAD_TOL
DETAIL_WEIGHT, TV_WEIGHT = 2.0, 0.5
POOLS = list(PC.STEP_POOLS)
LABELS = [C.label(r) for r in PC.STEP_TABLE]
ROWS = dict(zip(LABELS, PC.STEP_TABLE))
SCALARS = ("loss", "loss_c", "loss_s", "loss_detail", "loss_tv")


def train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, *, transport=("remd",),
               weight_map=None, temporal=(), probe=None, detail_weight=DETAIL_WEIGHT, tv_weight=TV_WEIGHT):
    out = R.train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom,
                       transport=transport, weight_map=weight_map, temporal=temporal)
    tdtype = out["img"].dtype
    dtype = np.float64 if tdtype == torch.float64 else np.float32
    x, c = out["img"][0].numpy(), content_feat[0][0].detach().numpy()
    h, w = x.shape[:2]
    weights = None
    if weight_map is not None:
        weights = [PR.pool(weight_map.numpy()[:, :, None], p, dtype)[:, :, 0] for p in POOLS]
    ld, gd = PR.detail(x, c, POOLS, weights, [detail_weight] * len(POOLS), dtype)
    lt, gt = PR.tv(x, PR.TV_EPS, tv_weight, dtype)
    img = O.fold_laplacian_pyramid(variables)
    extra = torch.autograd.grad(img, variables, grad_outputs=torch.from_numpy((gd + gt).astype(dtype))[None])
    out["grads"] = [a + b for a, b in zip(out["grads"], extra)]
    out["loss_detail_terms"] = [float(v) for v in ld]
    out["loss_detail"] = float(sum(float(v) for v in ld))
    out["loss_tv"] = float(lt)
    out["loss_base"] = float(out["loss"])
    out["loss"] = out["loss"] + detail_weight * out["loss_detail"] + tv_weight * out["loss_tv"]
    return out


@functools.lru_cache(maxsize=None)
def problem(lb):
    """the inputs of case `lb` (_step_ref.step_problem); cached, treat as read-only"""
    row = ROWS[lb]
    (h, w) = row[4]
    return R.step_problem(h, w, C.n_samples(row), row[5], masks=C.masks_of(row), n_styles=2 if row[1] == "blend" else 1,
                          weight_map=row[2], n_targets=row[3])


def reference_step(lb, dtype=torch.float64, vgg=None):
    row = ROWS[lb]
    return R.reference_step(problem(lb), C.transport_of(row), dtype=dtype, blend_weights=C.blend_of(row), vgg=vgg,
                            step=train_step)


def step_distance(got, ref):
    """(worst of SCALARS, loss_t included where the case has a target, relative to max(1, |ref|); worst pyramid level's
    gradient in relative L2)"""
    keys = SCALARS + (("loss_t",) if len(ref["loss_t_terms"]) else ())
    sc = max(abs(float(got[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in keys)
    return sc, max(R.step_grads(got, ref))
