"""Steps with the photorealism term (StepEngine(photo=)): the float64 step of tests/_pixel_prior_step.py
(the step of _step_ref.py, with or without the detail and TV terms) plus the term of tests/_matting_ref.py on the folded
image, the content as the guide,

    loss = (step of _pixel_prior_step)  +  photo_weight * L_photo,

its pixel gradient taken through the fold's adjoint by torch autograd.  The rows are _pixel_prior_cases.STEP_TABLE (64 x 64
and 42 x 64, one and two regions, a blend with a weight map, with and without a temporal target), each with the detail and
TV terms on or off.  The rows' losses differ by a factor of six, so each carries its own photo_weight, chosen so that the
term is 10..30 % of the loss at the first step: tests/test_matting_cpu.py asserts it.

Bounds: _step_ref.TOL_SCALAR on every scalar relative to max(1, |ref|) and GRAD_TOL on every pyramid level's gradient in
relative L2; tests/test_matting_cpu.py holds this restatement's own float32 run within a quarter of both."""
import functools

import numpy as np
import torch

import _matting_ref as MR
import _pixel_prior_step as PS
import _step_ref as R
from oracle import strotss_oracle as O

TOL_SCALAR, GRAD_TOL = R.TOL_SCALAR, R.GRAD_TOL
RADIUS, EPS = 1, 1e-4               # the command line's defaults
# (row of _pixel_prior_step, detail and TV terms on, photo_weight)
CASES = [(PS.LABELS[0], False, 6.0), (PS.LABELS[1], True, 40.0), (PS.LABELS[2], True, 15.0), (PS.LABELS[3], False, 30.0)]
LABELS = [f"{lb}-{'priors' if on else 'plain'}" for lb, on, _ in CASES]
BY_LABEL = dict(zip(LABELS, CASES))


def train_step(priors, photo_weight, variables, vgg, content_feat, *args, **kw):
    out = PS.train_step(variables, vgg, content_feat, *args, **kw,
                        **({} if priors else dict(detail_weight=0.0, tv_weight=0.0)))
    f32 = out["img"].dtype != torch.float64
    x, c = out["img"][0].numpy(), content_feat[0][0].detach().numpy()
    lp, gp = (MR.matting_float32 if f32 else MR.value_grad)(x, c, RADIUS, EPS)
    dtype = np.float32 if f32 else np.float64
    img = O.fold_laplacian_pyramid(variables)
    extra = torch.autograd.grad(img, variables, grad_outputs=torch.from_numpy((photo_weight * gp).astype(dtype))[None])
    out["grads"] = [a + b for a, b in zip(out["grads"], extra)]
    out["loss_photo"] = float(lp)
    out["loss"] = out["loss"] + photo_weight * out["loss_photo"]
    return out


def problem(lb):
    return PS.problem(BY_LABEL[lb][0])


def photo_share(lb, ref):
    """the weighted term's share of the step's loss"""
    return BY_LABEL[lb][2] * ref["loss_photo"] / float(ref["loss"])


@functools.lru_cache(maxsize=None)
def _reference_step(lb, f32):
    import _step_cases as C
    row_lb, priors, weight = BY_LABEL[lb]
    row = PS.ROWS[row_lb]
    return R.reference_step(PS.problem(row_lb), C.transport_of(row), dtype=torch.float32 if f32 else torch.float64,
                            blend_weights=C.blend_of(row), step=functools.partial(train_step, priors, weight))


def reference_step(lb, dtype=torch.float64, vgg=None):
    """the step of case `lb`; cached for the default float64 / float32 trunks, treat as read-only"""
    if vgg is None:
        return _reference_step(lb, dtype != torch.float64)
    import _step_cases as C
    row_lb, priors, weight = BY_LABEL[lb]
    row = PS.ROWS[row_lb]
    return R.reference_step(PS.problem(row_lb), C.transport_of(row), dtype=dtype, blend_weights=C.blend_of(row), vgg=vgg,
                            step=functools.partial(train_step, priors, weight))


def step_distance(lb, got, ref):
    """(worst scalar relative to max(1, |ref|): loss, loss_c, loss_s, loss_photo, with the priors loss_detail and loss_tv,
    with a target loss_t; worst pyramid level's gradient in relative L2)"""
    keys = ("loss", "loss_c", "loss_s", "loss_photo") + (("loss_detail", "loss_tv") if BY_LABEL[lb][1] else ()) + \
        (("loss_t",) if len(ref["loss_t_terms"]) else ())
    sc = max(abs(float(got[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in keys)
    return sc, max(R.step_grads(got, ref))
