"""GPU parity of the whole hot path: StepEngine.step() vs the float64 oracle's train_step +
rmsprop_update on identical weights, images and injected index sets; the reference-named operator
surface (nn.losses / nn.model / nn.strotss_utils) through autograd; the CLI driver end to end."""
import argparse
import os

import numpy as np
import pytest
import torch

from oracle import strotss_oracle as O

from _masked_oracle import mask_report, vgg_with_masks_of

pytestmark = pytest.mark.gpu

DEV = "cuda"
# One step's six variable gradients against the float64 oracle, relative L2.  What the linear backward chain itself
# contributes is measured by test_engine_backward_chain_without_sign_flips (<= 3e-4: Winograd F(4x4,3x3) rounding through 13
# layers); the losses add the rounding of their own gradients (L1 / hard-min terms: an entry of sign(a - b) or an arg-min
# flips where |a - b| is below float32 rounding, which changes one sample's row of dL/d(features), a 1e-3-relative event at
# 256-1024 samples).  Round 2 allowed 2e-2 everywhere; measured over all step tests of this file: 3.1e-3 at most.
GRAD_TOL = 5e-3


def _img(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(1, h, w, 3, generator=g, dtype=torch.float32)
    # low-pass once so the Laplacian pyramid is not pure noise
    return torch.nn.functional.avg_pool2d(x.permute(0, 3, 1, 2), 3, 1, 1).permute(0, 2, 3, 1).contiguous()


def _setup(h, w, n_samples, masks=None, seed=0, weights=None):
    from nn import _ops, engine
    from nn.model import VGGParams, synthetic_weights
    if weights is None:
        weights = synthetic_weights('16', 0)
    content, style = _img(h, w, 1 + seed), _img(h + 8, w - 4, 2 + seed)
    rng = np.random.default_rng(seed)
    alpha = 8.0
    denom = 2.0 + alpha + 1.0 / max(alpha, 1.0)
    vgg = O.VGG(weights, dtype=torch.float64)
    c64, s64 = content.double(), style.double()
    with torch.no_grad():
        cf = [c64] + vgg(c64)
        sf = [s64] + vgg(s64)
    init = (O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True))
    params = VGGParams(weights, '16', None, DEV)
    cfeat = engine.extract_features(params, content.to(DEV))
    sfeat = engine.extract_features(params, style.to(DEV))
    regions = masks if masks is not None else [(None, None)]
    s_samples, targets, idx_sets = [], [], []
    for cm, sm in regions:
        s_idx = O.make_indices(style.shape[1], style.shape[2], False, n_samples, rng, mask=sm)
        with torch.no_grad():
            s_samples.append(O.sample_features(sf, s_idx, False))
        feats = _ops.hypercol_gather(sfeat, torch.from_numpy(s_idx).to(DEV), False)
        targets.append(engine.StyleTarget.build(feats, s_idx.shape[0], 2179))
        idx_sets.append([O.make_indices(h, w, True, n_samples, rng, mask=cm) for _ in range(3)])
    eng = engine.StepEngine(params, cfeat, targets, init.float().to(DEV), alpha, denom, 2e-3, sample_size=n_samples)
    return dict(vgg=vgg, cf=cf, s_samples=s_samples, init=init, eng=eng, idx_sets=idx_sets, alpha=alpha, denom=denom)


class _EngineMaskedVGG:
    """The oracle's VGG with the ReLU masks and pool selections of the engine's last trunk forward (`vgg_with_masks_of`,
    which checks every disagreement against MASK_FLIP_TOL and records it in `report`)."""

    def __init__(self, vgg, eng):
        self.vgg, self.acts, self.report = vgg, [a.cpu() for a in eng.trunk.acts], []

    def __call__(self, x):
        self.report = []
        return vgg_with_masks_of(self.vgg, x, self.acts, self.report)


def _oracle_vgg(S, eng):
    """The float64 network a step is compared with.  Where a layer runs in Winograd form, its float32 rounding (~1e-5 of the
    output range) flips the ReLU mask of every pre-activation that close to zero -- measured 9 ... 50 per trunk at 341 x 512
    and 683 x 1024, each within 1e-6 of its layer's max |pre| -- and each flip moves a whole gradient entry: measured 4.6e-3 relative L2 on the pixel gradient of the linear probe at
    341 x 512 with the float64 network's own masks, 5.9e-6 with the engine's (test_engine_backward_chain_at_production_
    routing); the whole steps at 256 px and up then reach 5.2e-3, above GRAD_TOL.  So on any trunk with a Winograd layer
    the masks and pool selections of ALL layers (the first layer's and split-K direct layers' too: they inherit the
    Winograd layers' rounding) are taken from the engine's forward, and every place where they disagree with float64 is
    checked to lie within MASK_FLIP_TOL of zero (`vgg_with_masks_of`).  All-direct trunks keep the oracle's own masks."""
    return S["vgg"] if _trunk_routes(eng) <= {"direct", "direct_splitk"} else _EngineMaskedVGG(S["vgg"], eng)


def _check_step(S, masked):
    eng = S["eng"]
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(S["init"])]
    # the engine's variables are the fp32 kernels' pyramid of the same image
    for a, b in zip(eng.variables, variables):
        assert (a.cpu().double() - b.detach()).abs().max() < 2e-6
    rms = [torch.zeros_like(v) for v in variables]
    idx0 = [s[0] for s in S["idx_sets"]]
    eng.forward_backward([torch.from_numpy(i).to(DEV) for i in idx0])
    torch.cuda.synchronize()
    vgg = _oracle_vgg(S, eng)
    if masked:
        ref = O.train_step_masked(variables, vgg, S["cf"], S["s_samples"], idx0, S["alpha"], S["denom"])
    else:
        ref = O.train_step(variables, vgg, S["cf"], S["s_samples"][0], idx0[0], S["alpha"], S["denom"])
    if isinstance(vgg, _EngineMaskedVGG):
        print("step %dx%d: %s" % (eng.h, eng.w, mask_report(vgg.report)))
    got = eng.losses()
    for k in ("loss", "loss_c", "loss_s"):
        assert abs(got[k] - float(ref[k])) < 5e-5 * max(1.0, abs(float(ref[k]))), (k, got[k], float(ref[k]))
    # image and pixel gradient
    assert (eng.fold[0].cpu().double() - ref["img"]).abs().max() < 5e-6
    for k, (g, gr) in enumerate(zip(eng.gvars, ref["grads"])):
        rel = float((g.cpu().double() - gr).norm() / gr.norm())
        print("step %dx%d gradient level %d: rel L2 %.2e" % (eng.h, eng.w, k, rel))
        assert rel < GRAD_TOL, (k, rel)
    # one RMSprop update applied to the same gradients must agree tightly
    gsnap = [g.clone() for g in eng.gvars]
    eng.apply_gradients()
    with torch.no_grad():
        for v, r, g in zip(variables, rms, gsnap):
            O.rmsprop_update(v, r, g.cpu().double(), 2e-3)
    for a, b in zip(eng.variables, variables):
        assert (a.cpu().double() - b.detach()).abs().max() < 1e-5


def test_engine_step_matches_oracle_square():
    _check_step(_setup(64, 64, 384), masked=False)


def test_engine_step_matches_oracle_regime_weights():
    """the square step's problem and bounds on weights shaped like a pretrained trunk's (tests/_regime.py trunk_weights:
    dead channels, mostly-zero maps, channel scales spread over orders of magnitude and growing from block1 to block5)"""
    import _regime
    _check_step(_setup(64, 64, 256, weights=_regime.trunk_weights()), masked=False)


def test_engine_step_matches_oracle_nonsquare():
    # 42x64 is the reference image's first scale: exercises floor sizes and the W-axis divisor rule
    _check_step(_setup(42, 64, 300, seed=3), masked=False)


def test_engine_step_matches_oracle_masked():
    h, w = 64, 64
    cm1 = np.zeros((h, w, 1), np.float32); cm1[:, :30] = 1
    cm2 = 1 - cm1
    sm1 = np.zeros((h + 8, w - 4, 1), np.float32); sm1[:40] = 1
    sm2 = 1 - sm1
    _check_step(_setup(h, w, 256, masks=[(cm1, sm1), (cm2, sm2)], seed=5), masked=True)


def _trunk_routes(eng):
    """The convolution routes (forward and data-gradient) the engine's trunk takes on its generic layers."""
    from nn import model as M
    out = set()
    for L, a in zip(eng.trunk.p.layers, eng.trunk.acts):
        if L["cin"] != 3:
            h, w = int(a.shape[1]), int(a.shape[2])
            out.update(M.conv_route(h, w, L["cin"], L["cout"], dgrad=d) for d in (False, True))
    return out


# Default routing at the sizes the product runs (content_im.jpg's scales): the same tolerances as the
# small steps above, whose layers all take the split-K direct kernel.
PRODUCTION_STEPS = {
    (170, 256): {"F4_fused_f32", "F4_gemm_f32", "F2_gemm_f32", "direct_splitk"},
    (341, 512): {"F4_fused_f32", "F4_gemm_f32", "F2_gemm_f32"},
    (683, 1024): {"F4_fused_f32", "F4_gemm_f32", "F4_x3_gemm_128", "F4_x3_gemm_64"},
}


@pytest.mark.parametrize("hw", sorted(PRODUCTION_STEPS), ids=lambda hw: "%dx%d" % hw)
def test_engine_step_at_production_routing_vs_oracle(hw):
    h, w = hw
    S = _setup(h, w, 1024, seed=21)
    assert _trunk_routes(S["eng"]) == PRODUCTION_STEPS[hw], sorted(_trunk_routes(S["eng"]))
    _check_step(S, masked=False)


def test_engine_masked_step_at_production_routing_vs_oracle():
    h, w = 256, 256
    cm1 = np.zeros((h, w, 1), np.float32); cm1[:, :110] = 1
    sm1 = np.zeros((h + 8, w - 4, 1), np.float32); sm1[:150] = 1
    S = _setup(h, w, 1024, masks=[(cm1, sm1), (1 - cm1, 1 - sm1)], seed=22)
    assert _trunk_routes(S["eng"]) == {"F4_fused_f32", "F4_gemm_f32", "direct_splitk"}, sorted(_trunk_routes(S["eng"]))
    _check_step(S, masked=True)


def test_engine_backward_chain_at_production_routing():
    """test_engine_backward_chain_without_sign_flips at 341 x 512 (fused, F(4x4,3x3) f32 GEMMs and F(2x2,3x3) layers).
    At this size the float64 network's own ReLU masks are not enough: among 10^7 activations per layer a few lie within
    float32 rounding of zero (measured 16 flipped masks over the trunk), and each flipped mask moves a whole gradient
    entry (measured 1.6e-3 ... 4.6e-3 relative L2).  So the float64 side takes the engine's masks and pool selections,
    every disagreement checked to lie within rounding (`_masked_oracle.py`), and what is left is the linear chain's
    rounding alone."""
    eng, rels = _chain_probe(341, 512, 1024, 23, engine_masks=True)
    assert _trunk_routes(eng) == PRODUCTION_STEPS[(341, 512)], sorted(_trunk_routes(eng))
    print("341 x 512 backward chain, engine masks, rel L2 per level:", ["%.2e" % r for r in rels])
    for k, rel in enumerate(rels):
        assert rel < 3e-4, (k, rel)


def test_engine_multi_step_resynchronised():
    """Three consecutive steps (non-zero RMSprop slots, moved variables).  Before each step the
    oracle is re-synchronised to the engine's state so that fp32-vs-fp64 sign flips of near-zero
    gradient entries (RMSprop's first update is 10*lr*sign(g)) cannot compound: every step's losses,
    gradients and update are then held to the single-step tolerances."""
    S = _setup(64, 64, 384, seed=7)
    eng = S["eng"]
    for it in range(3):
        variables = [v.cpu().double().requires_grad_(True) for v in eng.variables]
        rms = [r.cpu().double() for r in eng.rms]
        idx = S["idx_sets"][0][it]
        eng.forward_backward([torch.from_numpy(idx).to(DEV)])
        ref = O.train_step(variables, _oracle_vgg(S, eng), S["cf"], S["s_samples"][0], idx, S["alpha"], S["denom"])
        got = eng.losses()
        for k in ("loss", "loss_c", "loss_s"):
            assert abs(got[k] - float(ref[k])) < 5e-5 * max(1.0, abs(float(ref[k]))), (it, k, got[k], float(ref[k]))
        for k, (g, gr) in enumerate(zip(eng.gvars, ref["grads"])):
            rel = float((g.cpu().double() - gr).norm() / gr.norm())
            assert rel < GRAD_TOL, (it, k, rel)
        gsnap = [g.cpu().double() for g in eng.gvars]
        eng.apply_gradients()
        with torch.no_grad():
            for v, r, g in zip(variables, rms, gsnap):
                O.rmsprop_update(v, r, g, 2e-3)
        for a, b in zip(eng.variables, variables):
            assert (a.cpu().double() - b.detach()).abs().max() < 1e-5
        for a, b in zip(eng.rms, rms):
            assert (a.cpu().double() - b).abs().max() < 1e-6 * max(1.0, float(b.abs().max()))


def test_engine_free_running_trajectory():
    """Free-running fp32 HIP vs fp64 oracle for a few steps with the same injected indices: the loss
    curves agree to 1%; pixels may differ by a few update quanta (10*lr = 0.02 per level and step)
    wherever a near-zero gradient entry changed sign -- bitwise agreement is unattainable even
    TF-vs-TF across devices (tolerances)."""
    S = _setup(64, 64, 384, seed=7)
    eng = S["eng"]
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(S["init"])]
    rms = [torch.zeros_like(v) for v in variables]
    for it in range(3):
        idx = S["idx_sets"][0][it]
        ref = O.train_step(variables, S["vgg"], S["cf"], S["s_samples"][0], idx, S["alpha"], S["denom"])
        with torch.no_grad():
            for v, r, g in zip(variables, rms, ref["grads"]):
                O.rmsprop_update(v, r, g, 2e-3)
        eng.step([torch.from_numpy(idx).to(DEV)])
        got = eng.losses()
        assert abs(got["loss"] - float(ref["loss"])) < 1e-2 * abs(float(ref["loss"])), (it, got, float(ref["loss"]))
    out = eng.stylized().cpu().double()
    ref_img = O.fold_laplacian_pyramid([v.detach() for v in variables])
    assert (out - ref_img).abs().mean() < 0.03


def test_graph_replay_equals_eager():
    """One hipGraph per step: replays must reproduce eager launches (same kernels, same order; only
    the scatter's fp32 atomics may reorder), and capture must not advance the optimisation."""
    Sa, Sb = _setup(64, 64, 384, seed=9), _setup(64, 64, 384, seed=9)
    ea, eb = Sa["eng"], Sb["eng"]
    idx = [torch.from_numpy(i).to(DEV) for i in Sa["idx_sets"][0]]
    before = [v.clone() for v in eb.variables]
    eb.capture_graph([idx[0]])
    for a, b in zip(before, eb.variables):
        assert torch.equal(a, b)
    assert float(sum(r.abs().sum() for r in eb.rms)) == 0.0
    for it in range(3):
        ea.step([idx[it]])
        eb.step([idx[it]])
        la, lb = ea.losses(), eb.losses()
        # step 0 starts from identical state: identical losses.  Later steps inherit the scatter's
        # atomic-order noise through sign(g) of near-zero gradient entries (10*lr quanta).
        assert abs(la["loss"] - lb["loss"]) < (1e-6 if it == 0 else 2e-2) * abs(la["loss"]), (it, la, lb)
    for a, b in zip(ea.variables, eb.variables):
        assert (a - b).abs().mean() < 5e-3


def _chain_probe(h, w, n, seed, engine_masks=False):
    """The engine's backward path driven by a fixed linear functional sum(W * p_feat) instead of the losses, against float64
    autograd of the same functional: the six variable gradients' relative L2 errors.  engine_masks: the float64 side takes
    its ReLU masks and pool selections from the engine's activations (`vgg_with_masks_of`)."""
    S = _setup(h, w, n, seed=seed)
    eng = S["eng"]
    idx = S["idx_sets"][0][0]
    ti = torch.from_numpy(idx).to(DEV)
    eng.trunk.forward(eng.fold_forward())
    torch.cuda.synchronize()
    variables = [v.clone().requires_grad_(True) for v in O.make_laplacian_pyramid(S["init"])]
    img = O.fold_laplacian_pyramid(variables)
    if engine_masks:
        report = []
        maps = vgg_with_masks_of(S["vgg"], img, [a.cpu() for a in eng.trunk.acts], report)
        print("%d x %d backward chain: %s" % (h, w, mask_report(report)))
    else:
        maps = S["vgg"](img)
    pf = O.sample_features([img] + maps, idx, True)
    W = torch.randn(pf.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    ref = torch.autograd.grad((pf * W).sum(), variables)
    eng._idx[0] = ti
    eng.gp[0].zero_()
    eng.gp[0][:len(idx), :2179] = W.float().to(DEV)
    if eng.deterministic:
        from nn import _ops
        _ops.hypercol_scatter_plan(eng._mt_pred, ti, eng._plans[0])
    eng.trunk.backward(eng._scatter)
    eng._fold_adjoint()
    torch.cuda.synchronize()
    return eng, [float((g.cpu().double() - gr).norm() / gr.norm()) for g, gr in zip(eng.gvars, ref)]


def test_engine_backward_chain_without_sign_flips():
    """How much of the 2e-2 gradient tolerance of `_check_step` is REAL error?  The losses are L1 / hard-min terms whose
    gradients flip sign on fp32 rounding noise; this probe replaces them by a fixed linear functional sum(W * p_feat)
    (dL/dp_feat = W, no flips) and sends it down the engine's own backward path -- tap scatter, 13 data-gradient layers
    (at these sizes all on the split-K direct kernel; test_engine_backward_chain_at_production_routing runs the Winograd
    forms), pooling, first-layer gradient, fold adjoint -- against float64 autograd of the same functional.  What is left
    is the linear chain's rounding (and ReLU masks of activations within rounding of zero)."""
    for (h, w, n) in ((64, 64, 384), (42, 64, 300)):
        _, rels = _chain_probe(h, w, n, 13)
        for k, rel in enumerate(rels):
            assert rel < 3e-4, (h, w, k, rel)            # measured: see DESIGN.md 6


def test_deterministic_mode_is_bitwise_reproducible():
    """StepEngine(deterministic=True) (STROTSS_DETERMINISTIC=1): the tap adjoint as a sorted scatter instead of float
    atomics -- two engines fed the same index stream hold bitwise identical variables after three steps, eagerly and
    through the captured graph, and the step still matches the default engine to rounding."""
    from nn import engine as E
    idx_np = None
    finals = []
    for graph in (False, True, False):
        S = _setup(64, 64, 384, seed=11)
        eng = S["eng"]
        det = E.StepEngine(eng.params, eng.content_feat, eng.style_targets, eng.stylized(), eng.alpha, eng.loss_denom,
                           eng.lr, sample_size=384, deterministic=True)
        idx = [torch.from_numpy(i).to(DEV) for i in S["idx_sets"][0]]
        if graph:
            det.capture_graph([idx[0]])
        for it in range(3):
            det.step([idx[it]])
        torch.cuda.synchronize()
        finals.append([v.clone() for v in det.variables] + [g.clone() for g in det.gvars])
    for a, b, c in zip(*finals):
        assert torch.equal(a, c), "eager vs eager"
        assert torch.equal(a, b), "eager vs graph replay"
    # against the atomic engine: one step from the same state
    S = _setup(64, 64, 384, seed=11)
    eng = S["eng"]
    det = E.StepEngine(eng.params, eng.content_feat, eng.style_targets, eng.stylized(), eng.alpha, eng.loss_denom, eng.lr,
                       sample_size=384, deterministic=True)
    i0 = torch.from_numpy(S["idx_sets"][0][0]).to(DEV)
    eng.forward_backward([i0]); det.forward_backward([i0])
    for a, b in zip(eng.gvars, det.gvars):
        assert float((a - b).norm() / a.norm()) < 1e-5


def test_prescatter_backward_equals_the_interleaved_one():
    """Small scales (nn/model.py VGGTrunk: every tapped layer's gradient comes from an accumulating producer): all maps'
    taps land in ONE scatter launch before the backward pass.  Same kernels and inputs otherwise -> the pixel gradient
    equals the interleaved form's to summation-order rounding; the deterministic engine (no atomics) must agree too."""
    if os.environ.get("STROTSS_PRESCATTER") == "0":
        pytest.skip("the switch under test is off in this run")
    S = _setup(64, 64, 384, seed=5)
    eng = S["eng"]
    assert eng.trunk.prescatter, "64 px: all tapped layers' producers are split-K direct dgrads or pool backwards"
    i0 = torch.from_numpy(S["idx_sets"][0][0]).to(DEV)
    eng.forward_backward([i0])
    pre = [g.clone() for g in eng.gvars]
    eng.trunk.prescatter = False
    eng.forward_backward([i0])
    for a, b in zip(pre, eng.gvars):
        assert float((a - b).norm() / b.norm()) < 1e-5
    eng.trunk.prescatter = True
    from nn import engine as E
    det = E.StepEngine(eng.params, eng.content_feat, eng.style_targets, eng.stylized(), eng.alpha, eng.loss_denom, eng.lr,
                       sample_size=384, deterministic=True)
    det.forward_backward([i0])
    for a, b in zip(pre, det.gvars):
        assert float((a - b).norm() / b.norm()) < 1e-5
    # 256 px: the tapped gradients come from F(4x4,3x3) data-gradients (fused kernel and three-kernel form), which can add to
    # their output since ABI 7; the policy keeps the interleaved scatter there (the fill of the tapped buffers costs what the
    # nine launches save: nn/model.py), STROTSS_PRESCATTER_MAX_PIXELS moves the border -- same gradient either way
    assert not _setup(256, 256, 256, seed=5)["eng"].trunk.prescatter
    os.environ["STROTSS_PRESCATTER_MAX_PIXELS"] = str(256 * 256)
    try:
        S = _setup(256, 256, 256, seed=5)
    finally:
        del os.environ["STROTSS_PRESCATTER_MAX_PIXELS"]
    eng = S["eng"]
    assert eng.trunk.prescatter
    i0 = torch.from_numpy(S["idx_sets"][0][0]).to(DEV)
    eng.forward_backward([i0])
    pre = [g.clone() for g in eng.gvars]
    eng.trunk.prescatter = False
    eng.forward_backward([i0])
    for a, b in zip(pre, eng.gvars):
        assert float((a - b).norm() / b.norm()) < 1e-5


_VARIANT1_CHILD = """
import sys; sys.path[:0] = %r
import torch, test_hip_engine as T
# 96 px: block1_conv2's data-gradient (64 -> 64 at 96 x 96) is a one-pass direct kernel and writes a tapped buffer
S = T._setup(96, 96, 384, seed=5); eng = S["eng"]
assert not eng.trunk.prescatter, "the library's one-pass kernel overwrites under this variant"
eng.forward_backward([torch.from_numpy(S["idx_sets"][0][0]).to(T.DEV)])
assert all(bool(torch.isfinite(g).all()) and float(g.norm()) > 0 for g in eng.gvars)
# 64 px: every tapped gradient comes from a split-K data-gradient or a pool backward, which add under every variant
S = T._setup(64, 64, 384, seed=5); eng = S["eng"]
assert eng.trunk.prescatter
i0 = torch.from_numpy(S["idx_sets"][0][0]).to(T.DEV)
eng.forward_backward([i0]); pre = [g.clone() for g in eng.gvars]
eng.trunk.prescatter = False
eng.forward_backward([i0])
for a, b in zip(pre, eng.gvars):
    assert float((a - b).norm() / b.norm()) < 1e-5
print("variant 1 ok")
"""


def test_prescatter_asks_the_library_whether_the_direct_data_gradient_adds():
    """STROTSS_CONV_VARIANT=1 (read once per process, hence a child): the one-pass direct kernel of that variant only
    overwrites, so strotss_conv3x3_dgrad refuses `accumulate` there.  The trunk asks the library before it pre-scatters
    (strotss_conv3x3_dgrad_can_accumulate): the step runs at a size with such a layer, interleaved, and where every
    producer still adds the pre-scattered backward equals the interleaved one as in the test above."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    paths = [os.path.join(root, "tests"), os.path.join(root, "strotss-tensorflow_amd"), root]
    env = {k: v for k, v in os.environ.items() if not k.startswith("STROTSS_")}
    out = subprocess.run([sys.executable, "-c", _VARIANT1_CHILD % (paths,)], env=dict(env, STROTSS_CONV_VARIANT="1"), cwd=root,
                         capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "variant 1 ok" in out.stdout, out.stdout[-2000:] + out.stderr[-3000:]


# ------------------------------------------------------------------ operator surface (autograd)
def test_losses_api_autograd():
    from nn import losses as L
    import run_strotss as RS
    rng = np.random.default_rng(0)
    n, ns, d = 96, 80, 131
    mk = lambda r, c: np.abs(rng.standard_normal((r, c))) + 0.01
    x, y, c = mk(ns, d), mk(n, d), mk(n, d)
    xt, ct = torch.from_numpy(x), torch.from_numpy(c)
    yt = torch.from_numpy(y).clone().requires_grad_(True)
    ref = 8.0 * O.content_loss(ct, yt) + O.style_loss(xt, yt, 8.0)
    gref, = torch.autograd.grad(ref, yt)
    yd = torch.from_numpy(y).float().to(DEV).requires_grad_(True)
    xd, cd = torch.from_numpy(x).float().to(DEV), torch.from_numpy(c).float().to(DEV)
    got = 8.0 * RS.ContentLoss()(cd, yd) + RS.StyleLoss(xd, 8.0)(yd)
    got.backward()
    assert abs(float(got) - float(ref)) < 1e-4 * abs(float(ref))
    rel = float((yd.grad.cpu().double() - gref).norm() / gref.norm())
    assert rel < 5e-3, rel
    # forward-only helpers
    assert (L.cosine_distance(xd, yd.detach()).cpu().double() - O.cosine_distance(xt, yt.detach())).abs().max() < 2e-6
    assert (L.l2_distance(xd[:, :3], yd.detach()[:, :3]).cpu().double()
            - O.l2_distance(xt[:, :3], yt.detach()[:, :3])).abs().max() < 1e-5
    with pytest.raises(KeyError):
        L.sinkhorn_knopp(xd, yd, distance='manhattan')
    with pytest.raises(NotImplementedError):            # its alternating scalings are not symmetric in the two sides
        L.sinkhorn_knopp(xd.clone().requires_grad_(True), yd)


@pytest.mark.parametrize("shape", [(96, 80, 131), (64, 100, 3), (70, 70, 35)])
def test_losses_differentiate_both_arguments_like_tf(shape):
    """TF's tape differentiates BOTH arguments of every loss and distance (reference losses.py:12-24, 39-80); run_strotss.py
    only ever asks for the prediction side.  The operator surface gives both: value and the two gradients of
    moment_matching, self_similarity (equal row counts), relaxed_emd under every metric, and of the matrices cosine_distance /
    l2_distance under a random upstream gradient, against the float64 autograd restatement."""
    from nn import losses as L
    n, ns, d = shape
    rng = np.random.default_rng(n + 3 * ns + d)
    mk = lambda r, c: np.abs(rng.standard_normal((r, c))) + 0.01
    x, y = mk(ns, d), mk(n, d)

    def both(fn_ref, fn_hip, a, b, tol, upstream=None):
        at, bt = torch.from_numpy(a).clone().requires_grad_(True), torch.from_numpy(b).clone().requires_grad_(True)
        ref = fn_ref(at, bt)
        ad = torch.from_numpy(a).float().to(DEV).requires_grad_(True)
        bd = torch.from_numpy(b).float().to(DEV).requires_grad_(True)
        got = fn_hip(ad, bd)
        if upstream is None:
            ga, gb = torch.autograd.grad(ref, (at, bt))
            got.backward()
            assert abs(float(got) - float(ref)) < 5e-5 * max(1.0, abs(float(ref))), (float(got), float(ref))
        else:
            ga, gb = torch.autograd.grad((ref * upstream).sum(), (at, bt))
            (got * upstream.float().to(DEV)).sum().backward()
            assert float((got.detach().cpu().double() - ref.detach()).abs().max()) < 1e-5
        for name, g, want in (("first", ad.grad, ga), ("second", bd.grad, gb)):
            rel = float((g.cpu().double() - want).norm() / max(1e-30, float(want.norm())))
            assert rel < tol, (name, rel)
        # one side alone gives the same gradient as asking for both
        ad2 = torch.from_numpy(a).float().to(DEV).requires_grad_(True)
        got2 = fn_hip(ad2, torch.from_numpy(b).float().to(DEV))
        (got2 if upstream is None else (got2 * upstream.float().to(DEV)).sum()).backward()
        assert torch.equal(ad2.grad, ad.grad)

    both(O.moment_matching, L.moment_matching, x, y, 5e-3)
    for metric in ("cosine", "l2", "both"):
        both(lambda a, b: O.relaxed_emd(a, b, metric), lambda a, b: L.relaxed_emd(a, b, metric), x, y, 5e-3)
    if n == ns:
        both(O.self_similarity, L.self_similarity, x, y, 5e-3)
    G = torch.from_numpy(rng.standard_normal((ns, n)))
    both(O.cosine_distance, L.cosine_distance, x, y, 2e-4, upstream=G)
    both(O.l2_distance, L.l2_distance, x, y, 2e-4, upstream=G)
    # dist_metrics['both'] composes the two differentiable matrices
    both(lambda a, b: O.cosine_distance(a, b) + O.l2_distance(a, b), L.dist_metrics['both'], x, y, 2e-4, upstream=G)


def test_relaxed_emd_target_side_gradient_keeps_tf_maximum_tie_rule():
    """x == y: R_X == R_Y bitwise and the two branches differ; tf.maximum sends the tie to its FIRST argument R_X (rows of
    x, minima over y).  The gradient w.r.t. x comes from the kernels with the roles exchanged (STROTSS_REMD_SWAPPED): it must
    still be the R_X branch's, i.e. equal the float64 restatement's, for every metric."""
    from nn import losses as L
    rng = np.random.default_rng(3)
    x = np.abs(rng.standard_normal((48, 19))) + 0.01
    x[5] = x[2]                                    # a duplicated row: the two branches' tie-splitting differs
    for metric in ("cosine", "l2", "both"):
        at, bt = torch.from_numpy(x).clone().requires_grad_(True), torch.from_numpy(x).clone().requires_grad_(True)
        ref = O.relaxed_emd(at, bt, metric)
        ga, gb = torch.autograd.grad(ref, (at, bt))
        ad = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
        bd = torch.from_numpy(x).float().to(DEV).requires_grad_(True)
        L.relaxed_emd(ad, bd, metric).backward()
        for name, g, want in (("first", ad.grad, ga), ("second", bd.grad, gb)):
            err = float((g.cpu().double() - want).abs().max())
            # ('l2' at x == y: every minimum sits on the clamped diagonal, the reference's gradient is exactly zero; in f32
            # |x|^2 + |y|^2 - 2 x.y of a row with itself is rounding noise around the 1e-6 clamp, worth ~1e-7 of gradient)
            assert err < 2e-3 * float(want.abs().max()) + 2e-6, (metric, name, err, float(want.abs().max()))


@pytest.mark.parametrize("distance", ["l2", "both", "cosine"])
@pytest.mark.parametrize("shape", [(96, 80, 131), (64, 100, 3), (200, 150, 35), (33, 257, 2179), (50, 40, 1)])
def test_relaxed_emd_every_metric_any_width(distance, shape):
    """relaxed_emd(x, y, distance) for every entry of dist_metrics at any width (reference losses.py:27-28, 69-80):
    value and d/dy against the float64 autograd restatement; a duplicated style row and a duplicated prediction row make
    ties that tf.reduce_min splits; a prediction row equal to a style row exercises the 1e-6 clamp of l2_distance."""
    from nn import losses as L
    n, ns, d = shape
    rng = np.random.default_rng(n * 7 + ns + d)
    mk = lambda r, c: np.abs(rng.standard_normal((r, c))) + 0.01
    x, y = mk(ns, d), mk(n, d)
    x[3] = x[1]                       # tie along the style axis
    y[5] = y[2]                       # tie along the prediction axis
    y[7] = x[4]                       # m = |x|^2 + |y|^2 - 2 x.y ~ 0: clamped, no l2 gradient
    xt = torch.from_numpy(x)
    yt = torch.from_numpy(y).clone().requires_grad_(True)
    ref = O.relaxed_emd(xt, yt, distance)
    gref, = torch.autograd.grad(ref, yt)
    yd = torch.from_numpy(y).float().to(DEV).requires_grad_(True)
    got = L.relaxed_emd(torch.from_numpy(x).float().to(DEV), yd, distance)
    got.backward()
    assert abs(float(got) - float(ref)) < 5e-5 * abs(float(ref)) + 1e-6, (float(got), float(ref))
    g = yd.grad.cpu().double()
    if d == 1 and distance == "cosine":          # every cosine distance is 0 at width 1: no gradient to compare
        assert float(g.norm()) < 1e-4
        return
    # the clamped pair: float32 rounding decides on which side of 1e-6 `m` falls, in the oracle (float64: exactly 0) it
    # is clamped -> compare all other rows, and require row 7's gradient to be finite
    keep = torch.ones(n, dtype=torch.bool); keep[7] = False
    rel = float((g[keep] - gref[keep]).norm() / gref[keep].norm())
    assert rel < 3e-3, rel
    assert torch.isfinite(g).all()
    with pytest.raises(KeyError):
        L.relaxed_emd(torch.from_numpy(x).float().to(DEV), yd, 'manhattan')


@pytest.mark.parametrize("cfg", [(96, 80, 131, 10, 30), (64, 100, 67, 5, 12), (200, 200, 35, 10, 30)])
@pytest.mark.parametrize("distance", ["cosine", "l2", "both"])
def test_sinkhorn_knopp_matches_float64_autograd(cfg, distance):
    """Build-defined Sinkhorn cost (losses.py:83-105 is dead code in the reference): value and the gradient through
    the iterations against the float64 autograd restatement, for every entry of dist_metrics (losses.py:27-28)."""
    from nn import losses as L
    n, ns, d, l, iters = cfg
    rng = np.random.default_rng(n + ns)
    mk = lambda r, c: np.abs(rng.standard_normal((r, c))) + 0.01
    x, y = mk(ns, d), mk(n, d)
    if distance != 'cosine':
        y[3] = x[5]                                   # an l2 entry under the 1e-6 clamp: no gradient through it
    xt = torch.from_numpy(x)
    yt = torch.from_numpy(y).clone().requires_grad_(True)
    ref = O.sinkhorn_knopp(xt, yt, distance, float(l), iters)
    gref, = torch.autograd.grad(ref, yt)
    yd = torch.from_numpy(y).float().to(DEV).requires_grad_(True)
    got = L.sinkhorn_knopp(torch.from_numpy(x).float().to(DEV), yd, distance, l, iters)
    got.backward()
    assert abs(float(got) - float(ref)) < 2e-4 * abs(float(ref)), (float(got), float(ref))
    g = yd.grad.cpu().double()
    keep = torch.ones(n, dtype=torch.bool)
    if distance != 'cosine':
        keep[3] = False          # the clamped pair: float32 rounding decides on which side of 1e-6 its m falls (as in the REMD test)
    rel = float((g[keep] - gref[keep]).norm() / gref[keep].norm())
    assert rel < 2e-3, rel
    assert torch.isfinite(g).all()
    with pytest.raises(ValueError):
        L.sinkhorn_knopp(torch.from_numpy(x).float().to(DEV), yd, distance, 0)


def test_vgg_and_pyramid_api_autograd():
    from nn import strotss_utils as SU
    from nn.model import VGG, synthetic_weights
    weights = synthetic_weights('16', 0)
    vgg = VGG(weights=weights, device=DEV)
    ov = O.VGG(weights, dtype=torch.float64)
    img = _img(48, 40, 4)
    taps = vgg(img.to(DEV))
    rtaps = ov(img.double())
    assert len(taps) == 9
    for a, b in zip(taps, rtaps):
        assert tuple(a.shape) == tuple(b.shape)
        assert (a.cpu().double() - b).abs().max() < 2e-5 * max(1.0, float(b.abs().max()))
    # differentiable composition: fold -> vgg -> bilinear sampling -> weighted sum
    pyr64 = [p.clone().requires_grad_(True) for p in O.make_laplacian_pyramid(img.double())]
    rng = np.random.default_rng(1)
    idx = O.make_indices(48, 40, True, 128, rng)
    i64 = O.fold_laplacian_pyramid(pyr64)
    f64 = O.sample_features([i64] + ov(i64), idx, True)
    wgt = torch.rand(f64.shape, generator=torch.Generator().manual_seed(0), dtype=torch.float64)
    gref = torch.autograd.grad((f64 * wgt).sum(), pyr64)
    pyr = [p.detach().float().to(DEV).requires_grad_(True) for p in pyr64]
    im = SU.fold_laplacian_pyramid(pyr)
    assert (im.detach().cpu().double() - i64.detach()).abs().max() < 5e-6
    feats = SU.Sampling(128).bilinear([im] + vgg(im), indices=torch.from_numpy(idx).to(DEV))
    assert (feats.detach().cpu().double() - f64.detach()).abs().max() < 5e-5 * float(f64.abs().max())
    (feats * wgt.float().to(DEV)).sum().backward()
    for p, g in zip(pyr, gref):
        rel = float((p.grad.cpu().double() - g).norm() / g.norm())
        assert rel < 1e-4, rel
    # pyramid helpers
    ps = SU.make_laplacian_pyramid(img.to(DEV))
    for a, b in zip(ps, O.make_laplacian_pyramid(img.double())):
        assert (a.cpu().double() - b).abs().max() < 2e-6
    yuv = SU.convert_rgb_to_yuv(feats.detach())
    assert (yuv.cpu().double() - O.convert_rgb_to_yuv(f64.detach())).abs().max() < 1e-5


def test_vgg19_and_keras_preprocess_variants():
    from nn.model import VGG, synthetic_weights, vgg_config
    w19 = synthetic_weights('19', 1)
    v = VGG(vgg_type='19', weights=w19, device=DEV)
    taps = v(_img(32, 32, 2).to(DEV))
    assert [t.shape[-1] for t in taps] == [64, 64, 128, 128, 256, 256, 256, 512, 512]
    # keras-style preprocessing == BGR flip + mean subtraction on x*255 (model.py:38)
    w16 = synthetic_weights('16', 2)
    vk = VGG(use_keras_weight=True, weights=w16, device=DEV, layers=['block1_conv1'])
    img = _img(16, 16, 3)
    x = (img.double() * 255)[..., [2, 1, 0]] - torch.tensor([103.939, 116.779, 123.68], dtype=torch.float64)
    wt, b = w16[0]
    ref = torch.relu(torch.nn.functional.conv2d(x.permute(0, 3, 1, 2), wt.double().permute(3, 2, 0, 1), b.double(),
                                                padding=1)).permute(0, 2, 3, 1)
    got = vk(img.to(DEV))[0].cpu().double()
    assert (got - ref).abs().max() < 1e-4 * float(ref.abs().max())


def test_cli_end_to_end(tmp_path):
    """run_strotss.run() on two small synthetic JPEGs: 2 scales x 3 steps, writes a JPEG."""
    from PIL import Image
    import run_strotss as RS
    rng = np.random.default_rng(0)
    for name, (h, w) in (("c.jpg", (90, 120)), ("s.jpg", (100, 80))):
        arr = (rng.random((h // 10, w // 10, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).resize((w, h), Image.BILINEAR).save(tmp_path / name, quality=95)
    out = tmp_path / "out.png"
    args = RS.build_parser().parse_args([str(tmp_path / "c.jpg"), str(tmp_path / "s.jpg"), "-o", str(out),
                                         "--level", "2", "--max_iter", "3"])
    final = RS.run(args)
    assert final.dtype == torch.uint8 and tuple(final.shape) == (96, 128, 3)     # long side 128 at scale 2
    assert os.path.exists(out)
    with Image.open(out) as im:
        assert im.format == "JPEG" and im.size == (128, 96)     # always a JPEG, as the reference writes
    with pytest.raises(ValueError):
        bad = argparse.Namespace(**vars(args)); bad.content_mask = "x.jpg"; bad.style_mask = None
        RS.run(bad)


def _write_pair(tmp_path, seed=3):
    from PIL import Image
    rng = np.random.default_rng(seed)
    for name, (h, w) in (("c.jpg", (200, 256)), ("s.jpg", (180, 150))):
        arr = (rng.random((h // 8, w // 8, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).resize((w, h), Image.BILINEAR).save(tmp_path / name, quality=95)
    return str(tmp_path / "c.jpg"), str(tmp_path / "s.jpg")


@pytest.mark.parametrize("start_level", [0, 1])
def test_run_schedule_matches_oracle_run_scales(tmp_path, start_level):
    """the multi-scale driver run() against the oracle's run_scales (run_strotss.py:65-96,154-155 of
    the reference) over 3 (2 with --start_level 1) scales x 2 steps at 64 -> 256 px with the same seed, i.e. the same
    index stream (style draw per scale, then one draw per step).  Per scale: size, lr (halved on the last), alpha,
    loss_denom, the initial image of each of the three branches (2e-6) and the first step's losses (5e-5).  The oracle
    is re-synchronised to the product's result at every scale boundary: free-running trajectories differ by whole
    RMSprop quanta wherever a near-zero gradient entry changes sign."""
    import run_strotss as RS
    from nn import utils
    from nn.model import synthetic_weights
    from nn.rand import PhiloxStream
    cpath, spath = _write_pair(tmp_path)
    args = RS.build_parser().parse_args([cpath, spath, "-o", str(tmp_path / "o.jpg"), "--level", "3", "--max_iter", "2",
                                         "--log_every", "1", "--start_level", str(start_level), "--seed", "5"])
    tr = []
    final = RS.run(args, trace=tr)
    n_scales = 3 - start_level
    assert len(tr) == n_scales and all(len(t["steps"]) == 2 for t in tr)
    content = utils.load_image(cpath).cpu().double()
    style = utils.load_image(spath).cpu().double()
    finals = {t["i"]: t["final"].cpu().double() for t in tr}
    otr, osteps = [], []
    O.run_scales(content, style, synthetic_weights('16', 5), level=3, start_level=start_level, max_iter=2, lr=2e-3,
                 alpha=1.0, seed=5, sample_size=1024, dtype=torch.float64, scale_trace=otr, trace=osteps,
                 previous_override=lambda i: finals.get(i - 1), rng=PhiloxStream(5))   # the product's stream: its host twin
    assert len(otr) == n_scales
    for t, o in zip(tr, otr):
        assert (t["i"], t["scl"]) == (o["i"], o["scl"])
        assert t["lr"] == o["lr"] and t["alpha"] == o["alpha"] and abs(t["loss_denom"] - o["loss_denom"]) < 1e-12
        assert tuple(t["init"].shape) == tuple(o["init"].shape)
        assert float((t["init"].cpu().double() - o["init"]).abs().max()) < 2e-6, t["i"]
        first = [s_ for s_ in osteps if s_[0] == t["i"] and s_[1] == 0][0]
        for k, ref in zip(("loss", "loss_c", "loss_s"), first[2:]):
            assert abs(t["steps"][0][k] - ref) < 5e-5 * max(1.0, abs(ref)), (t["i"], k, t["steps"][0][k], ref)
        second = [s_ for s_ in osteps if s_[0] == t["i"] and s_[1] == 1][0]
        # (free-running second step: a whole RMSprop quantum 10*lr wherever a near-zero gradient entry changed sign between f32
        # and f64 -- and the float atomics of the tap adjoint reorder last bits from run to run: 1 % was seen to fail once in
        # ~15 runs with the fused kernel forced; the 200-step trajectory test states the free-running tolerance)
        assert abs(t["steps"][1]["loss"] - second[2]) < 2e-2 * abs(second[2]), (t["i"], t["steps"][1]["loss"], second[2])
        # fresh RMSprop slots per scale: after 2 steps no pixel moved by more than 2 first-step quanta per level
        assert float((t["final"] - t["init"]).abs().max()) <= 6 * 2 * 10 * t["lr"] * 1.05
    assert [t["lr"] for t in tr][-1] == 1e-3 and all(t["lr"] == 2e-3 for t in tr[:-1])
    assert [t["alpha"] for t in tr] == [16.0 / 2 ** i for i in range(start_level, 3)]
    assert final.dtype == torch.uint8 and tuple(final.shape) == (200, 256, 3)


def test_cli_with_masks(tmp_path):
    """Region-guided run (run_strotss.py:52-59, 97-125): load_mask pairs the colour regions, every
    region draws its own samples, one trunk pass serves all regions."""
    from PIL import Image
    import run_strotss as RS
    from nn import strotss_utils as SU
    rng = np.random.default_rng(1)
    h, w = 128, 160
    for name in ("c.jpg", "s.jpg"):
        arr = (rng.random((h // 8, w // 8, 3)) * 255).astype(np.uint8)
        Image.fromarray(arr).resize((w, h), Image.BILINEAR).save(tmp_path / name, quality=95)
    cm = np.zeros((h, w, 3), np.uint8); cm[:, : w // 2] = 255      # white | black survive the JPEG round trip
    sm = np.zeros((h, w, 3), np.uint8); sm[: h // 2] = 255
    Image.fromarray(cm).save(tmp_path / "cm.jpg", quality=100, subsampling=0)
    Image.fromarray(sm).save(tmp_path / "sm.jpg", quality=100, subsampling=0)
    c_masks, s_masks = SU.load_mask(str(tmp_path / "cm.jpg"), str(tmp_path / "sm.jpg"), None, sample_threth=5000)
    assert len(c_masks) == 2 and len(s_masks) == 2
    tot = sum(float(m.sum()) for m in c_masks)
    assert abs(tot - h * w) < 0.02 * h * w                       # the two regions tile the image (JPEG edge pixels aside)
    with pytest.raises(Exception):
        SU.load_mask(str(tmp_path / "cm.jpg"), str(tmp_path / "sm.jpg"), None, sample_threth=10 ** 9)
    # the CLI default threshold (10000 px) also keeps both 10240-px regions
    out = tmp_path / "out.jpg"
    args = RS.build_parser().parse_args([str(tmp_path / "c.jpg"), str(tmp_path / "s.jpg"), "-o", str(out),
                                         "--content_mask", str(tmp_path / "cm.jpg"), "--style_mask",
                                         str(tmp_path / "sm.jpg"), "--level", "2", "--max_iter", "3"])
    final = RS.run(args)
    assert tuple(final.shape) == (102, 128, 3) and os.path.exists(out)


def test_cli_config1_reference_images(tmp_path):
    """BASELINE config 1 on the reference's own two images (data fixtures under tests/golden/):
    256 px, one scale, 50 RMSprop steps -> `--max_size 256 --start_level 2 --level 3 --max_iter 50`
    (SURVEY.md 8d mapping).  Checks the size arithmetic of the reference (321x481 -> 170x256), that the
    optimisation makes progress and that a JPEG comes out."""
    from PIL import Image
    import run_strotss as RS
    from nn import engine as E
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    out = tmp_path / "out.jpg"
    args = RS.build_parser().parse_args([os.path.join(g, "content_im.jpg"), os.path.join(g, "style_im.jpg"), "-o", str(out),
                                         "--max_size", "256", "--start_level", "2", "--level", "3", "--max_iter", "50",
                                         "--log_every", "50"])
    seen = []
    orig = E.StepEngine.losses

    def spy(self):
        r = orig(self); seen.append((self.steps_done, r["loss"])); return r
    E.StepEngine.losses = spy
    try:
        final = RS.run(args)
    finally:
        E.StepEngine.losses = orig
    assert tuple(final.shape) == (170, 256, 3) and final.dtype == torch.uint8
    assert seen and seen[-1][0] == 50 and np.isfinite(seen[-1][1])
    with Image.open(out) as im:
        assert im.format == "JPEG" and im.size == (256, 170)


def _routes_in_child(env, sizes):
    """The union of the trunk routes at the given image sizes under `env` (the library reads its switches once per process)."""
    import json, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = ("import json, sys; sys.path.insert(0, %r); import _route_cases as RC; "
            "print(json.dumps(sorted(set().union(*(RC.routes_at(h, w) for h, w in %r)))))" % (os.path.join(root, "tests"), sizes))
    out = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, **env), capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, out.stderr[-2000:]
    return set(json.loads(out.stdout.strip().splitlines()[-1]))


def test_step_parity_with_the_fused_winograd_kernel_forced():
    """The size policy keeps the Winograd forms away from the small images of the step-level oracle parity tests (64 x 64,
    42 x 64: every layer takes the split-K direct kernel).  Repeat those tests in child processes (the switches are read
    once per process) with STROTSS_DIRECT_MAX_TILES=0, which sends the layers to Winograd: once with the fused kernel
    forced (STROTSS_WINO_FUSED=2: F(2x2,3x3) + fused), once without it and with the bf16x3 GEMMs on from 100 tiles
    (F(2x2,3x3) + f32 GEMMs + bf16x3 GEMMs on 64 x 64 tiles).  Each child's routes are asserted first."""
    import subprocess, sys
    if os.environ.get("STROTSS_WINO_FUSED") == "2":
        pytest.skip("already inside the forced run")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    for env, want in (({"STROTSS_WINO_FUSED": "2", "STROTSS_DIRECT_MAX_TILES": "0"}, {"F4_fused_f32", "F2_gemm_f32"}),
                      ({"STROTSS_DIRECT_MAX_TILES": "0", "STROTSS_WINO_FUSED": "0", "STROTSS_X3_MIN_TILES": "100"},
                       {"F4_x3_gemm_64", "F4_gemm_f32", "F2_gemm_f32"})):
        routes = _routes_in_child(env, [(64, 64), (42, 64)])
        assert want <= routes, (env, sorted(routes))
        out = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", "test_hip_engine.py"), "-q", "-x", "-m",
                              "gpu", "-k", "matches_oracle or resynchronised"], env=dict(os.environ, **env), cwd=root,
                             capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, str(env) + out.stdout[-3000:] + out.stderr[-2000:]
        assert " passed" in out.stdout


def test_full_scale_winograd_vs_direct(tmp_path):
    """SURVEY.md 7's end-to-end criterion for the Winograd forms: a WHOLE scale of the schedule (256 px, 200 steps, the CLI's
    own loop and index stream) in child processes -- default convolution routing (at 256 px: the fused F(4x4,3x3) kernel,
    F(4x4,3x3) on f32 GEMMs and split-K direct; at 128 px it would be direct everywhere) against STROTSS_WINOGRAD=0 (the direct f32-MFMA form everywhere, 16x less rounding
    error).  The optimisation is chaotic at rounding level (RMSprop's first updates are sign-like, the losses are L1 /
    hard-min terms), so the yardstick is a CONTROL: the direct form once more with the learning rate changed by 1e-7
    relative.  The Winograd run must stay as close to the direct run as the control does (loss curves: median deviation
    within 3x the control's, never above 5 %; converged loss level within 3 %; output PSNR within 3 dB of the control's)."""
    import subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    from nn import utils
    for name, seed in (("c.jpg", 11), ("s.jpg", 12)):
        utils.write_image(_img(256, 256, seed) * 255.0, str(tmp_path / name))
    outs = {}
    for tag, env, lr in (("wino", {}, "2e-3"), ("direct", {"STROTSS_WINOGRAD": "0"}, "2e-3"),
                         ("control", {"STROTSS_WINOGRAD": "0"}, "2.0000002e-3")):
        r = subprocess.run([sys.executable, os.path.join(root, "tests", "_scale_worker.py"), str(tmp_path / tag),
                            str(tmp_path / "c.jpg"), str(tmp_path / "s.jpg"), lr, "256"], env=dict(os.environ, **env),
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr[-3000:]
        outs[tag] = np.load(str(tmp_path / tag) + ".npz")
    routes = {k: set(outs[k]["routes"].tolist()) for k in outs}
    assert routes["wino"] == {"F4_fused_f32", "F4_gemm_f32", "direct_splitk"}, routes     # the forms under test do run
    assert routes["direct"] == routes["control"] and routes["direct"] <= {"direct", "direct_splitk"}, routes
    lw, ld, lc = (outs[k]["losses"][:, 0] for k in ("wino", "direct", "control"))
    assert lw.shape == ld.shape == lc.shape == (200,)
    dev_w, dev_c = np.abs(lw - ld) / np.abs(ld), np.abs(lc - ld) / np.abs(ld)
    assert dev_w[0] < 1e-4, dev_w[0]                              # the same first step to rounding

    def psnr(a, b):
        return 10 * np.log10(1.0 / np.mean((np.clip(a.astype(np.float64), 0, 1) - np.clip(b.astype(np.float64), 0, 1)) ** 2))
    p_w, p_c = psnr(outs["wino"]["final"], outs["direct"]["final"]), psnr(outs["control"]["final"], outs["direct"]["final"])
    print(f"256 px, 200 steps, against the direct form: Winograd routing median loss deviation {np.median(dev_w):.2e} (worst "
          f"{dev_w.max():.2e}), PSNR {p_w:.1f} dB; control (lr x (1 + 1e-7)) {np.median(dev_c):.2e} (worst {dev_c.max():.2e}), "
          f"PSNR {p_c:.1f} dB; loss {ld[0]:.3f} -> {ld[-20:].mean():.3f} / {lw[-20:].mean():.3f}")
    assert np.median(dev_w) <= max(3 * np.median(dev_c), 1e-2) and np.median(dev_w) < 5e-2, (np.median(dev_w), np.median(dev_c))
    assert abs(lw[-20:].mean() - ld[-20:].mean()) < 3e-2 * ld[-20:].mean()
    assert ld[-20:].mean() < 0.8 * ld[0] and lw[-20:].mean() < 0.8 * lw[0]      # and it IS an optimisation
    assert p_w >= p_c - 3.0, (p_w, p_c)
