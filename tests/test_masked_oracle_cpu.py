"""CPU: the mask-pinned float64 VGG of the GPU step tests (tests/_masked_oracle.py) reproduces the oracle's VGG when the
pinned activations are the oracle's own, and refuses activations whose masks disagree with float64 beyond rounding --
a forward kernel that zeroes a tile cannot hide behind the pinned masks."""
import pytest
import torch

from oracle import strotss_oracle as O

from _masked_oracle import vgg_with_masks_of

F = torch.nn.functional


def _setup():
    from nn.model import synthetic_weights
    vgg = O.VGG(synthetic_weights('16', 0))
    x = torch.rand(1, 37, 50, 3, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    h, acts, li = vgg.preprocess(x).permute(0, 3, 1, 2), [], 0
    for it in O.VGG16_CFG:
        if it == "pool":
            h = F.max_pool2d(h, 2, 2)
            continue
        w, b = vgg._oihw[li]
        li += 1
        h = F.relu(F.conv2d(h, w, b, padding=1))
        acts.append(h.permute(0, 2, 3, 1).float())          # what a float32 trunk would hold
    return vgg, x, acts


def test_pinned_masks_of_the_float64_activations_reproduce_the_oracle():
    vgg, x, acts = _setup()
    report = []
    got = vgg_with_masks_of(vgg, x, acts, report)
    for a, b in zip(vgg(x), got):
        assert (a - b).abs().max() <= 1e-13 * a.abs().max()
    assert len(report) == 13 and all(r[2] <= 1e-7 for r in report)


@pytest.mark.parametrize("layer", [1, 4, 9])
def test_a_zeroed_tile_fails_the_check(layer):
    vgg, x, acts = _setup()
    a = acts[layer].clone()
    assert float(a[0, :4, :4].amax()) > 0
    a[0, :4, :4] = 0.0                                       # a forward kernel that lost one 4 x 4 output tile
    acts[layer] = a
    with pytest.raises(AssertionError):
        vgg_with_masks_of(vgg, x, acts)
