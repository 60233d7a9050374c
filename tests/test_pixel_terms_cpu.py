"""CPU: the host side of the step's pixel-space terms (nn/pixel_terms.py) and the engine's one-GPU refusals.

1. Seven options of StepEngine run on one GPU only: each is refused with image strips and with region sharding, in the words
   below, and the refusal comes before the constructor touches a device (every tensor here lives on the CPU, and there need
   not be a library).
2. What each term's report() writes into the losses() dict and what it returns for out["loss"], on hand-set scalar tensors:
   the key sets, and the sums evaluated in the order losses() has always used (Python's left-to-right sum from 0 over the
   temporal targets, then detail, TV and photo, one addition each)."""
import pytest
import torch

from nn import engine, pixel_terms as PT

H, W = 8, 12
IMG = torch.zeros(1, H, W, 3)

# option -> (the constructor's keyword arguments, the refusal word for word)
ONE_GPU = {
    "sliced_palette": (dict(palette_transport="sliced"),
                       "the sliced palette term runs on one GPU: image strips and region sharding are not supported with it"),
    "sinkhorn": (dict(style_transport="sinkhorn"),
                 "the Sinkhorn style term runs on one GPU: image strips and region sharding are not supported with it"),
    "sliced_style": (dict(style_transport="sliced"),
                     "the sliced style term runs on one GPU: image strips and region sharding are not supported with it"),
    "content_weight": (dict(content_weight=torch.ones(H, W)),
                       "a content-weight map runs on one GPU: image strips and region sharding are not supported with it"),
    "temporal": (dict(temporal=engine.TemporalTarget(IMG[0], torch.ones(H, W), 1.0)),
                 "the temporal term runs on one GPU: image strips and region sharding are not supported with it"),
    "detail": (dict(detail=engine.DetailTarget(IMG[0], (1, 4), 1.0)),
               "the pixel-space priors (detail, tv_weight) run on one GPU: image strips and region sharding are not supported "
               "with them"),
    "tv": (dict(tv_weight=0.5),
           "the pixel-space priors (detail, tv_weight) run on one GPU: image strips and region sharding are not supported "
           "with them"),
    "photo": (dict(photo=engine.PhotoTarget(IMG[0], 1, 1e-4, 1.0)),
              "the photorealism term runs on one GPU: image strips and region sharding are not supported with it"),
}


@pytest.mark.parametrize("sharding", ["strips", "dist_group"])
@pytest.mark.parametrize("option", list(ONE_GPU))
def test_one_gpu_options_are_refused_before_any_device_call(option, sharding):
    kw, message = ONE_GPU[option]
    with pytest.raises(ValueError) as e:
        engine.StepEngine(None, [IMG], [object()], IMG, 8.0, 10.0, 2e-3, **{sharding: object()}, **kw)
    assert str(e.value) == message


def test_the_public_names_are_the_engines_too():
    for name in ("TemporalTarget", "DetailTarget", "PhotoTarget", "check_photo", "_check_prior_weight"):
        assert getattr(engine, name) is getattr(PT, name)


def _bare(cls, **fields):
    """a term with its reported fields set by hand: report() reads nothing else"""
    t = object.__new__(cls)
    for k, v in fields.items():
        setattr(t, k, v)
    return t


def _f32(*v):
    return torch.tensor(v, dtype=torch.float32)


def test_temporal_report_one_target_has_no_terms_list():
    t = _bare(PT.TemporalTerm, weights=[3.5], loss=_f32(0.1))
    out = {"loss": 2.0}
    share = t.report(out)
    l0 = float(_f32(0.1)[0])
    assert out == {"loss": 2.0, "loss_t": float(sum([l0]))}
    assert share == sum(lam * lt for lam, lt in zip([3.5], [l0]))


def test_temporal_report_three_targets_lists_three_terms():
    lams, vals = [3.5, 0.75, 12.0], _f32(0.1, 0.2, 0.7)
    t = _bare(PT.TemporalTerm, weights=lams, loss=vals.clone())
    out = {"loss": 2.0}
    share = t.report(out)
    terms = [float(v) for v in vals.tolist()]
    assert out == {"loss": 2.0, "loss_t": float(sum(terms)), "loss_t_terms": terms}
    assert share == sum(lam * lt for lam, lt in zip(lams, terms))       # left to right from 0, as written


def test_detail_report_always_lists_its_terms():
    for vals in (_f32(0.3), _f32(0.3, 0.01)):
        t = _bare(PT.DetailTerm, weight=2.0, loss=vals.clone())
        out = {"loss": 1.0}
        share = t.report(out)
        terms = [float(v) for v in vals.tolist()]
        assert out == {"loss": 1.0, "loss_detail": float(sum(terms)), "loss_detail_terms": terms}
        assert share == 2.0 * float(sum(terms))


def test_tv_and_photo_report_one_scalar_each():
    for cls, key in ((PT.TVTerm, "loss_tv"), (PT.PhotoTerm, "loss_photo")):
        t = _bare(cls, weight=0.3, loss=_f32(0.7))
        out = {"loss": 1.0}
        share = t.report(out)
        assert out == {"loss": 1.0, key: float(_f32(0.7)[0])}
        assert share == 0.3 * out[key]


def test_the_shares_are_added_in_the_order_temporal_detail_tv_photo():
    """losses() ends with `for t in terms: out["loss"] = out["loss"] + t.report(out)`: the value is the chain written out
    below, which is not the sum in another order (float addition does not associate)"""
    lams, tvals, dvals = [3.5, 0.75], _f32(0.1, 0.2), _f32(0.3, 0.01)
    terms = [_bare(PT.TemporalTerm, weights=lams, loss=tvals.clone()), _bare(PT.DetailTerm, weight=2.0, loss=dvals.clone()),
             _bare(PT.TVTerm, weight=0.5, loss=_f32(0.7)), _bare(PT.PhotoTerm, weight=40.0, loss=_f32(0.003))]
    base = 1.2345678901234567
    out = {"loss": base}
    for t in terms:
        out["loss"] = out["loss"] + t.report(out)
    lt = [float(v) for v in tvals.tolist()]
    want = base + sum(lam * l for lam, l in zip(lams, lt))
    want = want + 2.0 * float(sum(float(v) for v in dvals.tolist()))
    want = want + 0.5 * float(_f32(0.7)[0])
    want = want + 40.0 * float(_f32(0.003)[0])
    assert out["loss"] == want
    assert list(out) == ["loss", "loss_t", "loss_t_terms", "loss_detail", "loss_detail_terms", "loss_tv", "loss_photo"]
