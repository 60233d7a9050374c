"""Temporal-term timings and the consistency sweep.  One JSON line per measurement; device events around `iters`
back-to-back calls after a warm-up.
  - a whole step (device draw, captured graph) with and without the temporal term, alternated, at 64 px and 1024 px;
  - strotss_temporal_fwd_bwd alone and strotss_flow_warp (once per frame) at 1024 x 768;
`--consistency`: the consistency error E = mean_{c=1} (out_t - warp(out_{t-1}))^2 of --video runs on a texture translated by
(3, 2) px per frame, for several lambdas (what the default was chosen from), and the per-frame wall clock of a sequence
run against independent single-image runs.
`--steps-only temporal|plain`: just 20 captured 64-px steps of one configuration -- the program to run under
`rocprofv3 --kernel-trace` for the launches per step (tools/step_trace.py TRACE_DIR counts them)."""
import json
import os
import sys
import tempfile
import time

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


def make_engine(px, with_term):
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
    tt = None
    if with_term:
        cert = (torch.rand(h, w, generator=g) > 0.2).float()
        tt = engine.TemporalTarget(torch.rand(h, w, 3, generator=g).to(DEV), cert.to(DEV), 1000.0)
    eng = engine.StepEngine(params, engine.extract_features(params, content.to(DEV)), [target], content.to(DEV), 8.0, 10.125,
                            2e-3, sample_size=1024, temporal=tt)
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
    x, tgt, gimg = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(3))
    cert = (torch.rand(h, w, generator=g) > 0.2).float().to(DEV)
    loss = torch.zeros(1, device=DEV)
    ys, xs = np.mgrid[0:h, 0:w].astype(np.float32)
    fb = torch.from_numpy(np.stack([3 * np.sin(xs / 40), 2 * np.cos(ys / 30)], -1).astype(np.float32)).to(DEV)
    ff = -fb
    prev = x[None].contiguous()
    warped, c_out = torch.empty_like(prev), torch.empty(h, w, device=DEV)
    out = {"what": "kernels", "h": h, "w": w}
    out["temporal_fwd_bwd_us"] = round(_time(lambda: ops.temporal_fwd_bwd(x, tgt, cert, 1000.0, gimg, loss), iters), 2)
    out["flow_warp_us"] = round(_time(lambda: ops.flow_warp(prev, fb, None, warped, c_out), iters), 2)
    out["flow_warp_fwd_check_us"] = round(_time(lambda: ops.flow_warp(prev, fb, ff, warped, c_out), iters), 2)
    nbytes = h * w * (3 * 4 * 4 + 4)                   # x, target, gimg read + gimg written, certainty
    out["temporal_fwd_bwd_GBps"] = round(nbytes / out["temporal_fwd_bwd_us"] / 1e3, 1)
    return out


def consistency(lams, configs):
    import run_strotss as RS
    import _temporal_ref as T
    from PIL import Image
    tmp = tempfile.mkdtemp()
    h, w, shift = 48, 64, (3, 2)
    frames, flows = os.path.join(tmp, "frames"), os.path.join(tmp, "flows")
    paths = T.translated_sequence(frames, flows, n_frames=3, h=h, w=w, shift=shift)
    style = os.path.join(tmp, "style.jpg")
    Image.fromarray((T.texture(56, 60, 7) * 255).astype(np.uint8)).save(style, quality=95)
    stems = [os.path.splitext(os.path.basename(p))[0] for p in paths]
    fb = np.broadcast_to(-np.float32(shift), (h, w, 2))
    ff = np.broadcast_to(np.float32(shift), (h, w, 2))
    for cfg in configs:
        for lam in lams:
            out = os.path.join(tmp, f"o_{lam}")
            RS.run(RS.build_parser().parse_args([frames, style, "--video", "--flow_dir", flows, "--temporal_weight", str(lam),
                                                 "-o", out] + cfg))
            imgs = [np.asarray(Image.open(os.path.join(out, s + ".jpg")).convert("RGB"), dtype=np.float64) / 255 for s in stems]
            print(json.dumps({"what": "consistency", "cfg": " ".join(cfg), "lambda": lam,
                              "E": round(T.consistency_error(imgs, fb, ff), 7)}), flush=True)


def wall_clock(px, level, iters, n_frames=3):
    """per-frame wall clock: a --video run of n_frames against n_frames single-image runs (each its own VGG build)"""
    import run_strotss as RS
    import _temporal_ref as T
    from PIL import Image
    tmp = tempfile.mkdtemp()
    h, w = px * 3 // 4, px
    frames, flows = os.path.join(tmp, "frames"), os.path.join(tmp, "flows")
    paths = T.translated_sequence(frames, flows, n_frames=n_frames, h=h, w=w, shift=(3, 2))
    style = os.path.join(tmp, "style.jpg")
    Image.fromarray((T.texture(h, w, 7) * 255).astype(np.uint8)).save(style, quality=95)
    cfg = ["--level", str(level), "--max_iter", str(iters)]
    res = {"what": "wall_clock", "px": px, "level": level, "max_iter": iters, "frames": n_frames}
    for rep in range(2):                               # the first round includes one-time set-up (code objects, allocator)
        t0 = time.perf_counter()
        RS.run(RS.build_parser().parse_args([frames, style, "--video", "--flow_dir", flows, "-o", os.path.join(tmp, "v")] + cfg))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        for p in paths:
            RS.run(RS.build_parser().parse_args([p, style, "-o", os.path.join(tmp, "single.jpg")] + cfg))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res[f"video_s_per_frame_{rep}"] = round((t1 - t0) / n_frames, 3)
        res[f"single_s_per_frame_{rep}"] = round((t2 - t1) / n_frames, 3)
    return res


def main():
    if len(sys.argv) > 2 and sys.argv[1] == "--steps-only":
        fn = make_engine(64, sys.argv[2] == "temporal")
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--consistency":
        consistency([0.0, 10.0, 100.0, 1000.0, 10000.0],
                    [["--max_size", "64", "--level", "1", "--max_iter", "30"],
                     ["--max_size", "64", "--level", "1", "--max_iter", "200"]])
        print(json.dumps(wall_clock(1024, 5, 200)), flush=True)
        return
    iters = int(os.environ.get("ITERS", "50"))
    for px in (64, 1024):
        steps = {m: make_engine(px, m) for m in (False, True)}
        it = iters if px == 64 else max(10, iters // 5)
        for rep in range(3):                          # alternated: no term, term
            for m in (False, True):
                print(json.dumps({"what": "step", "px": px, "temporal": m, "rep": rep,
                                  "step_us": round(_time(steps[m], it), 1)}), flush=True)
        del steps
        torch.cuda.empty_cache()
    print(json.dumps(kernels(iters)), flush=True)


if __name__ == "__main__":
    main()
