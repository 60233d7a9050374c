"""Pixel-prior timings and the weight sweep.  One JSON line per measurement; device events around `iters`
back-to-back calls after a warm-up, configurations alternated, three repeats.
  - strotss_detail_fwd_bwd per pool size and for the default pools, strotss_tv_fwd_bwd and strotss_pool_mean alone at
    768 x 1024, next to strotss_temporal_fwd_bwd on the same box, with the bytes each must move and the rate that makes;
  - a whole captured step (device draw) without the terms, with each and with both, alternated, at 64 px and 1024 px.
`--sweep`: --detail_weight and --tv_weight over decades at --max_size 64 --level 1, 30 and 200 steps, deterministic, on
tests/golden's images: E_d (the mean squared D_4 of the written result against the content) and E_tv (L_tv of the written
result) per run -- what DESIGN §26's suggested starting values were read from."""
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tests")]
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


def make_engine(px, detail, tv):
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
    kw = {}
    if detail:
        kw["detail"] = engine.DetailTarget(content.to(DEV), (1, 4), 1.0)
    if tv:
        kw["tv_weight"] = 1.0
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [target], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024, **kw)
    if eng.enable_device_draw(0):
        eng.capture_graph()
        return eng.step
    from nn.strotss_utils import make_indices_np          # a grid too large for the device draw: one injected index set
    idx = [torch.from_numpy(make_indices_np(h, w, True, 1024, rng)).to(DEV)]
    eng.capture_graph(idx)
    return lambda: eng.step(idx)


def kernels(iters):
    h, w = 768, 1024
    g = torch.Generator().manual_seed(1)
    x, c, tgt, gimg = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(4))
    cert = (torch.rand(h, w, generator=g) > 0.2).float().to(DEV)
    loss = torch.zeros(4, device=DEV)
    px = h * w
    calls, nbytes = {}, {}
    for pools in ((1,), (2,), (4,), (8,), (16,), (1, 4)):
        contents = [ops.pool_mean(c, p) for p in pools]
        name = "detail_p" + "_".join(str(p) for p in pools)
        calls[name] = (lambda pools=pools, contents=contents: ops.detail_fwd_bwd(
            x, list(pools), contents, [None] * len(pools), [1.0] * len(pools), gimg, loss))
        # per pool size: gimg read and written (24 B / pixel); p = 1: x and c read once (24); p > 1: x read by the pooling
        # launch (12), the pooled planes written once and read twice (x's) or once (c's): 12 * 4 / p^2
        nbytes[name] = sum(px * (24 + (24 if p == 1 else 12 + 48 / (p * p))) for p in pools)
    calls["tv"] = lambda: ops.tv_fwd_bwd(x, 1.0, gimg, loss)
    nbytes["tv"] = px * 36                              # x read, gimg read and written
    pooled = ops.pool_mean(x, 4)
    calls["pool_mean_p4"] = lambda: ops.pool_mean(x, 4, pooled)
    nbytes["pool_mean_p4"] = px * (12 + 12 / 16)
    calls["temporal"] = lambda: ops.temporal_fwd_bwd(x, tgt, cert, 1000.0, gimg, loss)
    nbytes["temporal"] = px * (3 * 4 * 4 + 4)
    for rep in range(3):                                # alternated
        for name, fn in calls.items():
            us = _time(fn, iters)
            print(json.dumps({"what": "kernel", "name": name, "h": h, "w": w, "rep": rep, "us": round(us, 2),
                              "MB": round(nbytes[name] / 1e6, 2), "GBps": round(nbytes[name] / us / 1e3, 1)}), flush=True)


def sweep():
    import run_strotss as RS
    import _pixel_prior_ref as PR
    from PIL import Image
    os.environ["STROTSS_DETERMINISTIC"] = "1"
    tmp = tempfile.mkdtemp()
    golden = os.path.join(ROOT, "tests", "golden")
    out = os.path.join(tmp, "o.png")
    for iters in (30, 200):
        for flag, values in (("--detail_weight", (0.0, 0.1, 1.0, 10.0, 100.0, 1000.0, 10000.0)),
                             ("--tv_weight", (0.0, 0.01, 0.1, 1.0, 10.0, 100.0, 1000.0))):
            for v in values:
                args = RS.build_parser().parse_args([os.path.join(golden, "content_im.jpg"), os.path.join(golden, "style_im.jpg"),
                                                     "--max_size", "64", "--level", "1", "--max_iter", str(iters), "-o", out,
                                                     flag, str(v)])
                trace = []
                RS.run(args, trace)
                res = np.asarray(Image.open(out).convert("RGB"), dtype=np.float64) / 255.0
                content = RS._frame_at_result_size(RS._resolve(args), args.content_path).cpu().numpy().astype(np.float64)
                d4 = PR.laplacian(PR.pool(res, 4) - PR.pool(content, 4))
                d1 = PR.laplacian(res - content)
                last = trace[-1]["steps"][-1] if trace and trace[-1]["steps"] else {}
                print(json.dumps({"what": "sweep", "max_iter": iters, "flag": flag, "weight": v,
                                  "E_d": round(float((d4 * d4).mean()), 7), "E_d1": round(float((d1 * d1).mean()), 7),
                                  "E_tv": round(float(PR.tv(res)[0]), 6),
                                  "loss_c": round(float(last.get("loss_c", float("nan"))), 5),
                                  "loss_s": round(float(last.get("loss_s", float("nan"))), 5)}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--sweep":
        sweep()
        return
    iters = int(os.environ.get("ITERS", "50"))
    kernels(iters)
    for px in (64, 1024):
        steps = {m: make_engine(px, *m) for m in ((False, False), (True, False), (False, True), (True, True))}
        it = iters if px == 64 else max(10, iters // 5)
        for rep in range(3):                          # alternated
            for m, fn in steps.items():
                print(json.dumps({"what": "step", "px": px, "detail": m[0], "tv": m[1], "rep": rep,
                                  "step_us": round(_time(fn, it), 1)}), flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
