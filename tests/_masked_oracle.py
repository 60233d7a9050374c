"""The oracle's float64 VGG forward with the ReLU masks and max-pool selections of a float32 trunk's activations, every
disagreement with float64 checked (used by tests/test_hip_engine.py's step tests on trunks with Winograd layers;
tests/test_masked_oracle_cpu.py checks the check)."""
import torch

from oracle import strotss_oracle as O

# How far from zero a float64 pre-activation may be where the engine's ReLU mask disagrees with it, and how far below the
# float64 window maximum the value the engine's pool selection picks may lie: relative to the layer's max |pre|, 4x the
# worst single-layer F(4x4,3x3) error measured against float64 (2.3e-5, tests/test_hip_conv_routes.py).  A forward kernel
# that drops or zeroes outputs (a lost tail tile, a bad bounds check) disagrees far beyond it.
MASK_FLIP_TOL = 1e-4


def vgg_with_masks_of(vgg, x, acts, report=None):
    """O.VGG's forward in float64 with EVERY layer's ReLU mask and every max-pool selection taken from the float32
    activations `acts` (the engine's trunk, layer by layer): the linear map whose adjoint the engine's backward pass
    computes, so that a pre-activation within rounding of zero cannot flip a mask between the two sides.  Each
    disagreement is checked, not assumed: where (pre > 0) != (act > 0) the float64 pre-activation must lie within
    MASK_FLIP_TOL of zero, and the pooled value the engine's selection picks within MASK_FLIP_TOL of the float64 window
    maximum (both relative to the layer's max |pre|).  `report`: a list that receives (layer, mask flips, worst |pre| of a
    flip / max |pre|, pool selections that differ, worst shortfall / max |pre|) per layer."""
    F = torch.nn.functional
    h = vgg.preprocess(x.to(vgg.dtype)).permute(0, 3, 1, 2)
    outs, li, name = [], 0, None
    for item in O.VGG16_CFG:
        if item == "pool":
            _, sel = F.max_pool2d(acts[li - 1].permute(0, 3, 1, 2), 2, 2, return_indices=True)
            picked = h.flatten(2).gather(2, sel.flatten(2)).view(sel.shape)
            with torch.no_grad():
                short = F.max_pool2d(h, 2, 2) - picked
                scale = float(h.abs().max()) or 1.0
                worst = float(short.max()) / scale
                assert worst <= MASK_FLIP_TOL, ("pool after", name, worst, int((short > 0).sum()))
                if report is not None:
                    report[-1] += (int((short > 0).sum()), worst)
            h = picked
            continue
        name = item[0]
        w, b = vgg._oihw[li]
        pre = F.conv2d(h, w, b, padding=1)
        on = (acts[li] > 0).permute(0, 3, 1, 2)
        with torch.no_grad():
            flips = (pre > 0) != on
            n = int(flips.sum())
            worst = float(pre.abs()[flips].max()) / (float(pre.abs().max()) or 1.0) if n else 0.0
            assert worst <= MASK_FLIP_TOL, ("ReLU mask", name, n, worst)
            if report is not None:
                report.append((name, n, worst))
        h = pre * on
        li += 1
        if name in vgg.taps:
            outs.append(h.permute(0, 2, 3, 1))
    return outs


def mask_report(report):
    flips = sum(r[1] for r in report)
    sels = sum(r[3] for r in report if len(r) > 3)
    return ("%d ReLU mask flips (worst |pre| %.1e of the layer's max), %d pool selections off the float64 maximum "
            "(worst shortfall %.1e)" % (flips, max(r[2] for r in report), sels, max([r[4] for r in report if len(r) > 3] or [0])))
