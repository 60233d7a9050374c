"""Long-term temporal term timings.  One JSON line per measurement; device events around `iters` back-to-back
calls after a warm-up, the configurations alternated within every repeat:
  - strotss_temporal_multi_fwd_bwd alone at 768 x 1024 for 1..4 targets (count 1 is strotss_temporal_fwd_bwd) and
    strotss_temporal_long_certainty (once per frame) for 2..4;
  - a whole step (device draw, captured graph) with 4 targets against 1, at 64 px and 1024 px.
`--steps-only COUNT`: just 20 captured 64-px steps with COUNT targets -- the program to run under
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


def make_engine(px, count):
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
    raw = (torch.rand(count, h, w, generator=g) > 0.2).float().to(DEV)
    cert = ops.temporal_long_certainty(raw)
    tts = [engine.TemporalTarget(torch.rand(h, w, 3, generator=g).to(DEV), cert[j], 1000.0) for j in range(count)]
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [target], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024, temporal=tts)
    if eng.enable_device_draw(0):
        eng.capture_graph()
        return eng.step
    from nn.strotss_utils import make_indices_np          # a grid too large for the device draw: one injected index set
    idx = [torch.from_numpy(make_indices_np(h, w, True, 1024, rng)).to(DEV)]
    eng.capture_graph(idx)
    return lambda: eng.step(idx)


def kernels(iters, repeats=3):
    h, w = 768, 1024
    g = torch.Generator().manual_seed(1)
    x, gimg = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(2))
    tgts = [torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(4)]
    raw = (torch.rand(4, h, w, generator=g) > 0.2).float().to(DEV)
    certs = list(ops.temporal_long_certainty(raw).unbind(0))
    loss = torch.zeros(4, device=DEV)
    comb = torch.empty_like(raw)
    for rep in range(repeats):
        out = {"what": "kernels", "h": h, "w": w, "rep": rep}
        for n in (1, 2, 3, 4):
            us = _time(lambda: ops.temporal_multi_fwd_bwd(x, tgts[:n], certs[:n], [1000.0] * n, gimg, loss), iters)
            out[f"multi_{n}_us"] = round(us, 2)
            out[f"multi_{n}_GBps"] = round(h * w * (3 * 3 * 4 + n * (3 * 4 + 4)) / us / 1e3, 1)    # x, gimg r/w
        for n in (2, 3, 4):
            st = raw[:n].contiguous()
            out[f"long_certainty_{n}_us"] = round(_time(lambda: ops.temporal_long_certainty(st, comb[:n]), iters), 2)
        print(json.dumps(out), flush=True)


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--steps-only":
        fn = make_engine(64, int(sys.argv[2]))
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    iters = int(os.environ.get("ITERS", "50"))
    kernels(iters)
    for px in (64, 1024):
        steps = {n: make_engine(px, n) for n in (1, 4)}
        it = iters if px == 64 else max(10, iters // 5)
        for rep in range(3):                          # alternated: 1 target, 4 targets
            for n in (1, 4):
                print(json.dumps({"what": "step", "px": px, "targets": n, "rep": rep,
                                  "step_us": round(_time(steps[n], it), 1)}), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
