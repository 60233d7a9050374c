"""Float64 restatement of the train step with the Sinkhorn style term (StepEngine(style_transport="sinkhorn"), DESIGN.md
section 20) and the bounds tests/test_hip_transport.py holds the engine to.

style_loss_sinkhorn is oracle.strotss_oracle.style_loss with sinkhorn_knopp(target, prediction, 'cosine', l, T) in place of
the first relaxed_emd; train_step is the body of oracle.train_step / train_step_masked with that loss, for any number of
regions, each region's style side one sample set or a weighted list of them (a blend: loss_s = sum_k w_k style_loss_k).

Bounds of a step: the relaxed-EMD step's (tests/test_hip_engine.py) -- TOL_SCALAR on loss, loss_c and loss_s, GRAD_TOL on
every pyramid level's gradient in relative L2.  They stand for this term because the restatement's own float32 run on the
CPU stays within a quarter of both (tests/test_transport_cpu.py asserts it; STEP32 holds what it printed)."""
import numpy as np
import torch

from oracle import strotss_oracle as O

TOL_SCALAR = 5e-5
GRAD_TOL = 5e-3
MARGIN = 8.0
# worst float32-CPU distance from float64 over _transport_cases.STEPS and the blend step, as printed by
# tests/test_transport_cpu.py: (scalars, relative to max(1, |ref|); gradients, relative L2).  Both below a quarter of the
# bounds above, so those hold unchanged; were one not, its bound would be MARGIN times the value here.
# (Recorded, not asserted: the float32 run's sums depend on the machine and its thread count -- the blend's gradients
# measured 2.9e-4 on one machine and 3.5e-5 on another.  _transport_cases.STEPS says how the problems were chosen.)
STEP32 = {"scalar": 3.7e-8, "grad": 2.9e-4}       # gradients: 5.1e-5 at most with one style, 2.9e-4 on the blend


def style_loss_sinkhorn(target, prediction, alpha, l, T):
    inv_alpha = 1 / max(alpha, 1)
    l_m = O.moment_matching(target, prediction)
    l_sk = O.sinkhorn_knopp(target, prediction, "cosine", float(l), int(T))
    l_pal = O.relaxed_emd(O.convert_rgb_to_yuv(target), O.convert_rgb_to_yuv(prediction), "both")
    return l_m + l_sk + inv_alpha * l_pal


def train_step(variables, vgg, content_feat, styles_per_region, indices_per_region, alpha, loss_denom, l, T):
    """styles_per_region[r]: a sample set, or [(weight, sample set), ...] of a blend.  Returns what oracle.train_step
    returns (loss_c and loss_s the means over the regions)."""
    img = O.fold_laplacian_pyramid(variables)
    pred = [img] + vgg(img)
    loss = lc_a = ls_a = 0.0
    r = len(indices_per_region)
    for idx, style in zip(indices_per_region, styles_per_region):
        c_feat = O.sample_features(content_feat, idx, True)
        p_feat = O.sample_features(pred, idx, True)
        lc = O.content_loss(c_feat, p_feat)
        blend = style if isinstance(style, list) else [(1.0, style)]
        ls = sum(w * style_loss_sinkhorn(s, p_feat, alpha, l, T) for w, s in blend)
        loss = loss + (alpha * lc + ls) / loss_denom
        lc_a, ls_a = lc_a + lc, ls_a + ls
    loss = loss / r
    grads = torch.autograd.grad(loss, variables)
    return {"loss": loss.detach(), "loss_c": (lc_a / r).detach(), "loss_s": (ls_a / r).detach(), "grads": list(grads),
            "img": img.detach()}


def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def step_problem(h, w, n_samples, seed, masks=None, n_styles=1):
    """The inputs of one step, as tests/test_hip_engine.py's _setup makes them (same images, index draws and constants):
    weights, content, styles (n_styles images), per region the style index sets (one per style) and the prediction index
    set, alpha, loss_denom."""
    from nn.model import synthetic_weights
    content = _img(h, w, 1 + seed)
    styles = [_img(h + 8, w - 4, 2 + seed + 10 * k) for k in range(n_styles)]
    rng = np.random.default_rng(seed)
    regions = masks if masks is not None else [(None, None)]
    s_idx, idx = [], []
    for cm, sm in regions:
        s_idx.append([O.make_indices(s.shape[1], s.shape[2], False, n_samples, rng, mask=sm) for s in styles])
        idx.append(O.make_indices(h, w, True, n_samples, rng, mask=cm))
    alpha = 8.0
    return dict(weights=synthetic_weights('16', 0), content=content, styles=styles, s_idx=s_idx, idx=idx, alpha=alpha,
                denom=2.0 + alpha + 1.0 / max(alpha, 1.0), h=h, w=w, n_samples=n_samples)


def reference_step(P, l, T, dtype=torch.float64, blend_weights=None, vgg=None):
    """train_step of problem P in `dtype` on the CPU (vgg: a network to use in place of the plain one, float64 only)"""
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
    out = train_step(variables, net, cf, per_region, P["idx"], P["alpha"], P["denom"], l, T)
    out["init"] = init
    return out


def step_distance(got, ref):
    """(worst scalar distance relative to max(1, |ref|), worst relative L2 over the pyramid levels) between two results
    of train_step (or an engine's read-outs shaped like one)"""
    sc = max(abs(float(got[k]) - float(ref[k])) / max(1.0, abs(float(ref[k]))) for k in ("loss", "loss_c", "loss_s"))
    gr = max(float((torch.as_tensor(a).double() - b.double()).norm() / b.double().norm())
             for a, b in zip(got["grads"], ref["grads"]))
    return sc, gr
