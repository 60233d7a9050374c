"""The cases of the photorealism term, the smallest shapes at which csrc/matting.hip can go wrong:
1 x 1, 1 x 3 and 5 x 7 (every window clipped, at r = 4 larger than the image), 9 x 12, one short of, equal to and one past
the 16 x 16 tile in each dimension (15 x 16, 16 x 16, 17 x 33: 2 x 3 tiles), 42 x 63 and 48 x 64; each at r = 1, 2, 4 and
eps = 1e-4, 1e-2, 1 on the images of _smooth_ref.test_images (values a little outside [0, 1]).  Two more kinds at 9 x 12: a
constant guide, and an image that is affine in the guide.  References are computed once and cached: treat them as read-only."""
import functools

import numpy as np

import _matting_ref as MR
import _smooth_ref as SR

TILE = 16
SHAPES = ((1, 1), (1, 3), (5, 7), (9, 12), (TILE - 1, TILE), (TILE, TILE), (TILE + 1, 2 * TILE + 1), (42, 63), (48, 64))
RADII = (1, 2, 4)
EPSS = (1e-4, 1e-2, 1.0)
CASES = [(h, w, r, eps, "random") for (h, w) in SHAPES for r in RADII for eps in EPSS] + \
        [(9, 12, r, eps, kind) for kind in ("constant_guide", "affine") for r in RADII for eps in (1e-4, 1.0)]


def label(case):
    h, w, r, eps, kind = case
    return f"{h}x{w}-r{r}-eps{eps:g}-{kind}"


LABELS = [label(c) for c in CASES]
BY_LABEL = dict(zip(LABELS, CASES))
assert len(BY_LABEL) == len(CASES)
DENSE_LABELS = [lb for lb, c in BY_LABEL.items() if c[0] * c[1] <= MR.DENSE_MAX_PIXELS]


@functools.lru_cache(maxsize=None)
def images(h, w, kind):
    """(p, I) float32, the same for every r and eps of a shape"""
    p, I = SR.test_images(h, w, 1000 * h + w)
    if kind == "constant_guide":
        I = np.broadcast_to(np.float32([0.25, 0.5, 0.75]), (h, w, 3)).copy()
    elif kind == "affine":                  # p = A I + c, in float32 (so affine up to its rounding)
        A = np.float32([[0.5, 0.2, -0.1], [0.1, 0.6, 0.2], [-0.2, 0.1, 0.7]])
        p = (I @ A.T + np.float32([0.3, -0.1, 0.2])).astype(np.float32)
    g0 = np.random.default_rng(h * w + 7).standard_normal((h, w, 3)).astype(np.float32)
    for a in (p, I, g0):
        a.setflags(write=False)
    return p, I, g0


@functools.lru_cache(maxsize=None)
def inputs(lb):
    """dict: h, w, r, eps, kind, p, I (float32), g0 (a pre-filled gradient), and the float64 reference: loss, grad, scale
    (the scalar's error scale), q"""
    h, w, r, eps, kind = BY_LABEL[lb]
    p, I, g0 = images(h, w, kind)
    q = SR.guided_direct(p, I, r, eps)
    loss, grad = MR.value_grad(p, I, r, eps, q)
    return dict(h=h, w=w, r=r, eps=eps, kind=kind, p=p, I=I, g0=g0, q=q, loss=loss, grad=grad,
                scale=MR.loss_scale(p, I, r, eps, q))


def float32_errors(lb):
    """(gradient error / max |gradient|, scalar error / scale) of _matting_ref.matting_float32 on the case"""
    P = inputs(lb)
    l32, g32 = MR.matting_float32(P["p"], P["I"], P["r"], P["eps"])
    gmax = float(np.abs(P["grad"]).max())
    return (float(np.abs(g32 - P["grad"]).max()) / gmax if gmax > 0 else float(np.abs(g32).max()),
            abs(l32 - P["loss"]) / P["scale"] if P["scale"] > 0 else abs(l32))
