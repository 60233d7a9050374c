"""Content-weight map timings.  One JSON line per measurement; device events around `iters` back-to-back calls
after a warm-up.
  - a whole step (device draw, captured graph) with and without a map, alternated, at 64 px and 1024 px;
  - the loss section alone, n = ns = 1024, D = 2179: the weighted grouped call (strotss_step_losses_cw_fwd_bwd) against the
    unweighted one, K = 1 and K = 2.
`--steps-only map|plain`: just 20 captured 64-px steps of one configuration -- the program to run under
`rocprofv3 --kernel-trace` for the launches per step (tools/step_trace.py TRACE_DIR counts them)."""
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
    style_set = ops.make_style_set(targets, [1.0 / k] * k)
    cw = torch.as_tensor(np.random.default_rng(3).random(n), dtype=torch.float32, device=DEV)
    gp = torch.zeros_like(pred)
    sc = torch.zeros((4, 4), dtype=torch.float32, device=DEV)

    def plain():
        ops.step_losses_blend_fwd_bwd(pred, content, n, D, style_set, 8.0, 1.0, 1.0, 0.125, gp, sc[0], sc[1], sc[2], sc[3])

    def weighted():
        ops.step_losses_cw_fwd_bwd(pred, content, n, D, cw, style_set, 8.0, 1.0, 1.0, 0.125, gp, sc[0], sc[1], sc[2], sc[3])

    out = {"what": "loss_section", "K": k}
    for rep in range(2):                              # alternated: the spread shows in the repeats
        out[f"plain_us_{rep}"] = round(_time(plain, iters), 1)
        out[f"weighted_us_{rep}"] = round(_time(weighted, iters), 1)
    return out


def make_engine(px, with_map):
    from nn.model import VGGParams, synthetic_weights
    params = VGGParams(synthetic_weights('16', 0), '16', None, DEV)
    g = torch.Generator().manual_seed(0)
    h, w = px * 3 // 4, px
    content = torch.rand(1, h, w, 3, generator=g)
    style = torch.rand(1, h, w, 3, generator=g)
    rng = np.random.default_rng(0)
    feats = engine.extract_features(params, style.to(DEV))
    idx = np.stack([rng.integers(0, h, 1024), rng.integers(0, w, 1024)], 1).astype(np.float32)
    target = engine.StyleTarget.build(ops.hypercol_gather(feats, torch.from_numpy(idx).to(DEV), False), 1024, D)
    cw = None
    if with_map:                                      # a ramp over the columns with a zero band
        m = np.tile(np.linspace(0.0, 1.0, w, dtype=np.float32), (h, 1))
        m[h // 3: h // 3 + h // 8] = 0.0
        cw = torch.from_numpy(m).to(DEV)
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [target], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024, content_weight=cw)
    if eng.enable_device_draw(0):
        eng.capture_graph()
        return eng.step
    from nn.strotss_utils import make_indices_np          # a grid too large for the device draw: one injected index set
    idx = [torch.from_numpy(make_indices_np(h, w, True, 1024, rng)).to(DEV)]
    eng.capture_graph(idx)
    return lambda: eng.step(idx)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--steps-only":
        fn = make_engine(64, sys.argv[2] == "map")
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    iters = int(os.environ.get("ITERS", "50"))
    for px in (64, 1024):
        steps = {m: make_engine(px, m) for m in (False, True)}
        it = iters if px == 64 else max(10, iters // 5)
        for rep in range(3):                          # alternated: map, no map
            for m in (False, True):
                print(json.dumps({"what": "step", "px": px, "map": m, "rep": rep,
                                  "step_us": round(_time(steps[m], it), 1)}), flush=True)
        del steps
        torch.cuda.empty_cache()
    for k in (1, 2):
        print(json.dumps(loss_section(k, iters)), flush=True)


if __name__ == "__main__":
    main()
