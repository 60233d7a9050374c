"""Style blending timings: the loss section at K = 1..4 styles, n = ns = 1024, D = 2179 -- the one blended call
(strotss_step_losses_blend_fwd_bwd) against the K-loop of separate entries the engine falls back to -- and a whole 64-px and
1024-px step (device draw, captured graph) with K = 2 against K = 1.  One JSON line per measurement; device events around
`iters` back-to-back calls after a warm-up."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import numpy as np
import torch

from nn import _ops as ops
from nn import engine

DEV = "cuda"
D = 2179


def _feat(n, seed):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, D)), 0) + 0.01 * rng.random((n, D))
    b = torch.zeros(ops.pad32(n), ops.pad32(D), dtype=torch.float32, device=DEV)
    b[:n, :D] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


def _time(fn, iters, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1000.0 / iters        # us per call


def loss_section(k, iters):
    n = 1024
    pred, content = _feat(n, 1), _feat(n, 2)
    targets = [engine.StyleTarget.build(_feat(n, 10 + i), n, D) for i in range(k)]
    weights = [1.0 / k] * k
    gp = torch.zeros_like(pred)
    sc = torch.zeros((4, 4), dtype=torch.float32, device=DEV)
    style_set = ops.make_style_set(targets, weights)

    def one_call():
        ops.step_losses_blend_fwd_bwd(pred, content, n, D, style_set, 8.0, 1.0, 1.0, 0.125, gp, sc[0], sc[1], sc[2], sc[3])

    def k_loop():
        ops.selfsim_fwd_bwd(pred, content, n, D, 8.0, gp, sc[0])
        for i, (t, w) in enumerate(zip(targets, weights)):
            ops.moment_fwd_bwd(t.mean, t.cov, pred, n, D, w, gp, sc[1, i:])
            ops.remd_cos_fwd_bwd_after_selfsim(t.feats, t.inv_norm, t.panels, t.ns, pred, n, D, w, gp, sc[2, i:])
            ops.palette_remd_fwd_bwd(t.feats, t.ns, pred, n, 0.125 * w, gp, sc[3, i:])

    return {"what": "loss_section", "K": k, "one_call_us": round(_time(one_call, iters), 1),
            "k_loop_us": round(_time(k_loop, iters), 1)}


def step(px, k, iters):
    from nn.model import VGGParams, synthetic_weights
    params = VGGParams(synthetic_weights('16', 0), '16', None, DEV)
    g = torch.Generator().manual_seed(0)
    h, w = px * 3 // 4, px
    content = torch.rand(1, h, w, 3, generator=g)
    styles = [torch.rand(1, h, w, 3, generator=g) for _ in range(k)]
    rng = np.random.default_rng(0)
    targets = []
    for s in styles:
        feats = engine.extract_features(params, s.to(DEV))
        idx = np.stack([rng.integers(0, h, 1024), rng.integers(0, w, 1024)], 1).astype(np.float32)
        rows = ops.hypercol_gather(feats, torch.from_numpy(idx).to(DEV), False)
        targets.append(engine.StyleTarget.build(rows, 1024, D))
    style = targets[0] if k == 1 else engine.StyleBlend(targets, [1.0] * k)
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [style], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024)
    if eng.enable_device_draw(0):
        eng.capture_graph()
        fn = eng.step
    else:                                              # a grid too large for the device draw: one injected index set
        from nn.strotss_utils import make_indices_np
        idx = [torch.from_numpy(make_indices_np(h, w, True, 1024, rng)).to(DEV)]
        eng.capture_graph(idx)
        fn = lambda: eng.step(idx)
    return {"what": "step", "px": px, "K": k, "step_us": round(_time(fn, iters), 1)}


def main():
    iters = int(os.environ.get("ITERS", "50"))
    for k in (1, 2, 3, 4):
        print(json.dumps(loss_section(k, iters)), flush=True)
    for px in (64, 1024):
        for k in (1, 2, 1, 2):                        # alternated: the spread shows in the repeats
            print(json.dumps(step(px, k, iters if px == 64 else max(10, iters // 5))), flush=True)


if __name__ == "__main__":
    main()
