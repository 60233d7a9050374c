"""Steps with the sliced palette term (StepEngine(palette_transport="sliced")): a table beside
tests/_step_cases.py in its row format -- (transport, side, map, targets, (h, w), seed), targets always 0 here -- so that its
helpers (label, n_samples, transport_of, blend_of, masks_of) apply, and the float64 restatement of such a step: the train
step of tests/_step_ref.py with the sliced 1-Wasserstein term in the palette slot, through torch autograd (the sort's
permutation is piecewise constant, |.| has the subgradient 0 at 0).

The table holds both sizes, style_transport remd and sliced, one and two regions, a two-style blend and a content-weight
map.  Seeds are those _transport_cases gives each size and style side (0, 4, 5, 8); tests/test_palette_sliced_cpu.py holds the
restatement's own float32 run at every row within a quarter of TOL_SCALAR and GRAD_TOL, the condition under which those two
bounds stand for the GPU."""
import functools
import math

import numpy as np
import torch

import _palette_sliced_ref as PR
import _sliced_ref as SLR
import _step_cases as C
import _step_ref as R
from oracle import strotss_oracle as O

TOL_SCALAR, GRAD_TOL = R.TOL_SCALAR, R.GRAD_TOL
PROJECTIONS = 64                          # the engine's default
SCALARS = ("loss", "loss_c", "loss_s", "l_palette_sliced")

# (style transport, side, map, targets, (h, w), seed)
TABLE = [
    ("remd", "one", False, 0, (64, 64), 0),
    ("remd", "regions", True, 0, (64, 64), 5),
    ("remd", "blend", True, 0, (42, 64), 8),
    ("sliced", "one", True, 0, (42, 64), 4),
    ("sliced", "blend", False, 0, (64, 64), 8),
    ("sliced", "regions", False, 0, (64, 64), 5),
]
LABELS = [C.label(r) for r in TABLE]
ROWS = dict(zip(LABELS, TABLE))
assert len(ROWS) == len(TABLE)


def directions(dtype=torch.float64):
    from nn import rand
    return torch.as_tensor(rand.palette_directions(PROJECTIONS), dtype=dtype)


def palette_sliced_loss(target, prediction, dirs):
    """the term of tests/_palette_sliced_ref.py on torch tensors of one dtype: target (ns, >= 3), prediction (n, >= 3)"""
    n, ns, P = prediction.shape[0], target.shape[0], dirs.shape[0]
    a = (O.convert_rgb_to_yuv(prediction) @ dirs.T).T.contiguous()
    b = (O.convert_rgb_to_yuv(target) @ dirs.T).T.contiguous()
    a_s, b_s = torch.sort(a, dim=1, stable=True)[0], torch.sort(b, dim=1, stable=True)[0]
    I, J, LEN = PR.overlaps(n, ns)
    wgt = torch.as_tensor(LEN.astype(np.float64) / (float(n) * float(ns)), dtype=a.dtype)
    w = (wgt[None, :] * (a_s[:, torch.as_tensor(I)] - b_s[:, torch.as_tensor(J)]).abs()).sum()
    return w * (2.0 / (math.sqrt(3.0) * P))


def train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, *, transport=("remd",),
               weight_map=None, temporal=(), probe=None):
    """_step_ref.train_step (no temporal targets) with palette_sliced_loss where the palette relaxed EMD stands; the result
    also holds l_palette_sliced, weighted over a blend and averaged over the regions as the engine's l_palette is"""
    assert not list(temporal)
    kind = transport[0]
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    inv_alpha = 1 / max(alpha, 1)
    dirs = directions(img.dtype)
    loss = lc_a = ls_a = lp_a = 0.0
    r = len(indices_per_region)
    call = int(transport[3]) if kind == "sliced" else 0
    w64 = None if weight_map is None else weight_map.to(img.dtype)[None, :, :, None]
    for idx, style in zip(indices_per_region, styles_per_region):
        c_feat = O.sample_features(content_feat, idx, True)
        p_feat = O.sample_features(pred, idx, True)
        if w64 is None:
            lc = O.content_loss(c_feat, p_feat)
        else:
            lc = R.weighted_selfsim64(p_feat, c_feat, O.sample_features([w64], idx, True)[:, 0])
        ls = lp = 0.0
        for w, s in (style if isinstance(style, list) else [(1.0, style)]):
            if kind == "sliced":
                term = SLR.sliced_loss(s, p_feat, SLR.signs_of(transport[2], call, transport[1], p_feat.shape[1], p_feat.dtype))
            else:
                assert kind == "remd"
                term = O.relaxed_emd(s, p_feat)
            pal = palette_sliced_loss(s, p_feat, dirs)
            if probe is not None:
                probe.append((s.detach(), p_feat.detach()))
            ls = ls + w * (O.moment_matching(s, p_feat) + term + inv_alpha * pal)
            lp = lp + w * pal.detach()
            call += 1
        loss = loss + (alpha * lc + ls) / loss_denom
        lc_a, ls_a, lp_a = lc_a + lc, ls_a + ls, lp_a + lp
    loss = loss / r
    grads = torch.autograd.grad(loss, variables)
    return {"loss": loss.detach(), "loss_c": (lc_a / r).detach(), "loss_s": (ls_a / r).detach(), "l_palette_sliced": lp_a / r,
            "grads": list(grads), "img": img.detach()}


@functools.lru_cache(maxsize=None)
def problem(lb):
    """the inputs of case `lb` (_step_ref.step_problem); cached, treat as read-only"""
    row = ROWS[lb]
    (h, w) = row[4]
    return R.step_problem(h, w, C.n_samples(row), row[5], masks=C.masks_of(row), n_styles=2 if row[1] == "blend" else 1,
                          weight_map=row[2], n_targets=0)


def reference_step(lb, dtype=torch.float64, vgg=None, probe=None):
    row = ROWS[lb]
    return R.reference_step(problem(lb), C.transport_of(row), dtype=dtype, blend_weights=C.blend_of(row), vgg=vgg,
                            step=train_step, probe=probe)


def step_distance(got, ref):
    """(worst of SCALARS relative to max(1, |ref|), worst pyramid level's gradient in relative L2)"""
    sc = max(abs(float(got[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in SCALARS)
    return sc, max(R.step_grads(got, ref))
