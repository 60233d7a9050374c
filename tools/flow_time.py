"""Optical-flow timings.  One JSON line per measurement; device events around `iters` back-to-back calls after
a warm-up, the two solver forms alternated, three repeats.
  - strotss_optical_flow at 48 x 64, 192 x 256 and 768 x 1024 with iters_per_launch 1 (one sweep per launch) and 8 (blocked);
`--wall`: per-frame wall clock of a three-frame 1024-px --video run with --compute_flow against the same run with
--flow_dir on the flows the first run saved.
`--trace-only K H W`: just five flows of one configuration -- the program to run under `rocprofv3 --kernel-trace` for the
launches per flow (tools/step_trace.py TRACE_DIR flow_pack_kernel counts them)."""
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

DEV = "cuda"


def _time(fn, iters, warm=3):
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


def _pair(h, w):
    import _flow_ref as R
    return (torch.from_numpy(x).to(DEV) for x in R.smooth_pair(h, w, 0))


def launches(h, w, k, p):
    """launches of one flow, counted from the parameters as strotss_optical_flow issues them"""
    import _flow_ref as R
    levels = len(R.level_sizes(h, w, p.min_side, p.max_levels))
    return 2 * levels + levels + levels * p.warps * (1 + p.iters // k) + 1


def flows(iters):
    for h, w in ((48, 64), (192, 256), (768, 1024)):
        a, b = _pair(h, w)
        out = torch.empty(h, w, 2, device=DEV)
        params = {k: ops.flow_params(iters_per_launch=k) for k in (1, 8)}
        assert torch.equal(ops.optical_flow(a, b, params[1]), ops.optical_flow(a, b, params[8]))
        for rep in range(3):                          # alternated: plain, blocked
            for k in (1, 8):
                us = _time(lambda: ops.optical_flow(a, b, params[k], out), iters)
                print(json.dumps({"what": "flow", "h": h, "w": w, "iters_per_launch": k, "rep": rep,
                                  "launches": launches(h, w, k, params[k]), "flow_us": round(us, 1)}), flush=True)


def wall_clock(px=1024, level=5, max_iter=200, n_frames=3):
    import run_strotss as RS
    import _temporal_ref as T
    from PIL import Image
    tmp = tempfile.mkdtemp()
    h, w = px * 3 // 4, px
    frames, saved = os.path.join(tmp, "frames"), os.path.join(tmp, "saved")
    T.translated_sequence(frames, os.path.join(tmp, "exact"), n_frames=n_frames, h=h, w=w, shift=(3, 2))
    style = os.path.join(tmp, "style.jpg")
    Image.fromarray((T.texture(h, w, 7) * 255).astype(np.uint8)).save(style, quality=95)
    cfg = [frames, style, "--video", "--level", str(level), "--max_iter", str(max_iter)]
    res = {"what": "wall_clock", "px": px, "level": level, "max_iter": max_iter, "frames": n_frames}
    for rep in range(2):                               # the first round includes one-time set-up (code objects, allocator)
        t0 = time.perf_counter()
        RS.run(RS.build_parser().parse_args(cfg + ["--compute_flow", "--save_flow", saved, "-o", os.path.join(tmp, "c")]))
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        RS.run(RS.build_parser().parse_args(cfg + ["--flow_dir", saved, "-o", os.path.join(tmp, "f")]))
        torch.cuda.synchronize()
        t2 = time.perf_counter()
        res[f"compute_flow_s_per_frame_{rep}"] = round((t1 - t0) / n_frames, 3)
        res[f"flow_dir_s_per_frame_{rep}"] = round((t2 - t1) / n_frames, 3)
    return res


def main():
    if len(sys.argv) > 4 and sys.argv[1] == "--trace-only":
        k, h, w = (int(v) for v in sys.argv[2:5])
        a, b = _pair(h, w)
        p = ops.flow_params(iters_per_launch=k)
        for _ in range(8):
            ops.optical_flow(a, b, p)
        torch.cuda.synchronize()
        return
    if len(sys.argv) > 1 and sys.argv[1] == "--wall":
        print(json.dumps(wall_clock()), flush=True)
        return
    flows(int(os.environ.get("ITERS", "10")))


if __name__ == "__main__":
    main()
