"""Photorealism-term timings and the weight sweep.  One JSON line per measurement; device events around `iters`
back-to-back calls after a warm-up, configurations alternated, three repeats.
  - strotss_matting_fwd_bwd at r = 1, 2, 4 next to strotss_guided_smooth at the same radius and strotss_temporal_fwd_bwd on
    the same box, and strotss_matting_prepare, at 768 x 1024 and 48 x 64, with the bytes each must move and the rate that makes;
  - a whole captured step (device draw) with and without the term, alternated, at 64 px and 1024 px.
`--sweep`: --photo_weight over decades at --max_size 64 --level 1, 30 and 200 steps, deterministic, on tests/golden's images:
E_m (L_photo of the written result against the content, from the float64 restatement of tests/_matting_ref.py), loss_c and
loss_s per run -- what DESIGN §33's suggested starting value was read from."""
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
EPS = 1e-4


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


def make_engine(px, photo):
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
    kw = dict(photo=engine.PhotoTarget(content.to(DEV), photo, EPS, 1.0)) if photo else {}
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [target], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024, **kw)
    if eng.enable_device_draw(0):
        eng.capture_graph()
        return eng.step
    from nn.strotss_utils import make_indices_np          # a grid too large for the device draw: one injected index set
    idx = [torch.from_numpy(make_indices_np(h, w, True, 1024, rng)).to(DEV)]
    eng.capture_graph(idx)
    return lambda: eng.step(idx)


def kernels(h, w, iters):
    g = torch.Generator().manual_seed(1)
    x, c, tgt, gimg, out = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(5))
    cert = (torch.rand(h, w, generator=g) > 0.2).float().to(DEV)
    loss = torch.zeros(4, device=DEV)
    px = h * w
    calls, nbytes = {}, {}
    for r in (1, 2, 4):
        stats = ops.matting_prepare(c, r, EPS)
        calls[f"matting_r{r}"] = lambda r=r, stats=stats: ops.matting_fwd_bwd(x, c, stats, r, 1.0, gimg, loss)
        # once per pixel: img, guide (12 each), the statistics (36), gimg read and written (24); the halo re-reads are the cache's
        nbytes[f"matting_r{r}"] = px * (24 + 36 + 24)
        calls[f"matting_prepare_r{r}"] = lambda r=r, stats=stats: ops.matting_prepare(c, r, EPS, out=stats)
        nbytes[f"matting_prepare_r{r}"] = px * (12 + 36)
        calls[f"guided_smooth_r{r}"] = lambda r=r: ops.guided_smooth(x, c, r, EPS, out=out)
        nbytes[f"guided_smooth_r{r}"] = px * (24 + 2 * 216 + 12)      # its 216 B / pixel workspace written and read
    calls["temporal"] = lambda: ops.temporal_fwd_bwd(x, tgt, cert, 1000.0, gimg, loss)
    nbytes["temporal"] = px * (3 * 4 * 4 + 4)
    for rep in range(3):                                # alternated
        for name, fn in calls.items():
            us = _time(fn, iters)
            print(json.dumps({"what": "kernel", "name": name, "h": h, "w": w, "rep": rep, "us": round(us, 2),
                              "MB": round(nbytes[name] / 1e6, 3), "GBps": round(nbytes[name] / us / 1e3, 1)}), flush=True)


def e_m(result, content, radius=1, eps=EPS):
    """L_photo of an (h, w, 3) result against the content, in float64"""
    import _matting_ref as MR
    return MR.value_grad(result, content, radius, eps)[0]


def sweep():
    import run_strotss as RS
    from PIL import Image
    os.environ["STROTSS_DETERMINISTIC"] = "1"
    tmp = tempfile.mkdtemp()
    golden = os.path.join(ROOT, "tests", "golden")
    out = os.path.join(tmp, "o.png")
    for iters in (30, 200):
        for v in (None, 0.0, 0.1, 1.0, 10.0, 100.0, 1000.0, 10000.0, 100000.0):
            args = RS.build_parser().parse_args([os.path.join(golden, "content_im.jpg"), os.path.join(golden, "style_im.jpg"),
                                                 "--max_size", "64", "--level", "1", "--max_iter", str(iters), "-o", out] +
                                                ([] if v is None else ["--photo_weight", str(v)]))
            trace = []
            RS.run(args, trace)
            res = np.asarray(Image.open(out).convert("RGB"), dtype=np.float64) / 255.0
            content = RS._frame_at_result_size(RS._resolve(args), args.content_path).cpu().numpy().astype(np.float64)
            last = trace[-1]["steps"][-1] if trace and trace[-1]["steps"] else {}
            print(json.dumps({"what": "sweep", "max_iter": iters, "weight": v, "E_m": round(e_m(res, content), 7),
                              "loss_c": round(float(last.get("loss_c", float("nan"))), 5),
                              "loss_s": round(float(last.get("loss_s", float("nan"))), 5),
                              "loss_photo": last.get("loss_photo")}), flush=True)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--sweep":
        sweep()
        return
    iters = int(os.environ.get("ITERS", "50"))
    kernels(768, 1024, iters)
    kernels(48, 64, iters)
    for px in (64, 1024):
        steps = {m: make_engine(px, m) for m in (0, 1, 4)}
        it = iters if px == 64 else max(10, iters // 5)
        for rep in range(3):                          # alternated
            for m, fn in steps.items():
                print(json.dumps({"what": "step", "px": px, "photo_radius": m, "rep": rep, "step_us": round(_time(fn, it), 1)}),
                      flush=True)
        del steps
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
