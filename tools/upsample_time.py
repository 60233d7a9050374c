"""Guided-upsampling kernel timings.  One JSON line per size pair, radius and mode: device events around `iters`
back-to-back calls of strotss_guided_upsample (five launches each) after a warm-up, at 768 x 1024 -> 3072 x 4096 and
384 x 512 -> 3072 x 4096 for r = 4 and 16, with the apply kernel's compulsory bytes (12 read and 12 written per output pixel,
one 64-byte record per low-resolution pixel).  The cases are run in two alternated rounds.
`--trace-only H W R MODE`: just twenty calls from (H, W) to 3072 x 4096 -- the program to run under
`rocprofv3 --kernel-trace --stats` for the time of each of the five kernels."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import torch

from nn import _ops as ops

DEV = "cuda"
TARGET = (3072, 4096)


def _time(fn, iters, warm=10):
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


def _inputs(h, w, seed):
    g = torch.Generator().manual_seed(seed)
    H, W = TARGET
    x, lo = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(2))
    hi = torch.rand(H, W, 3, generator=g).to(DEV)
    return x, lo, hi, torch.empty_like(hi)


def upsample(h, w, r, mode, iters, round_):
    x, lo, hi, out = _inputs(h, w, h + r)
    ops.guided_upsample(x, lo, hi, r, 1e-3, mode, out)        # the workspace of the size exists before anything is timed
    us = _time(lambda: ops.guided_upsample(x, lo, hi, r, 1e-3, mode, out), iters)
    us_lo = _time(lambda: ops.guided_smooth(x, lo, r, 1e-3), iters)      # the four launches of the same shape, for scale
    H, W = TARGET
    apply_bytes = 24 * H * W + 64 * h * w
    return {"what": "guided_upsample", "round": round_, "h": h, "w": w, "H": H, "W": W, "r": r, "mode": mode, "iters": iters,
            "us": round(us, 2), "us_guided_smooth_same_lo": round(us_lo, 2), "apply_MB": round(apply_bytes / 1e6, 2),
            "apply_GBps_if_rest_is_smooth": round(apply_bytes / max(us - us_lo, 1e-3) / 1e3, 1)}


def trace_only(h, w, r, mode, calls=20):
    x, lo, hi, out = _inputs(h, w, r)
    for _ in range(calls):
        ops.guided_upsample(x, lo, hi, r, 1e-3, mode, out)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) == 6 and sys.argv[1] == "--trace-only":
        return trace_only(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]), sys.argv[5])
    iters = int(os.environ.get("ITERS", "50"))
    for round_ in (1, 2):
        for h, w in ((768, 1024), (384, 512)):
            for r in (4, 16):
                for mode in ("residual", "guided"):
                    print(json.dumps(upsample(h, w, r, mode, iters, round_)), flush=True)


if __name__ == "__main__":
    main()
