"""Photo-smoothing kernel timings.  One JSON line per size and radius: device events around `iters`
back-to-back calls of strotss_guided_smooth (four launches each) after a warm-up, at 48 x 64 and 768 x 1024 for r = 4, 16 and
64, with the bytes a call moves to and from memory, the bandwidth that makes and the float64 additions of its window sums.
`--trace-only R`: just twenty calls at 768 x 1024 with radius R -- the program to run under `rocprofv3 --kernel-trace --stats`
for the time of each of the four kernels."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import torch

from nn import _ops as ops

DEV = "cuda"


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


def extent_sum(n, r):
    """sum over x of the length of [x - r, x + r] clipped to [0, n)"""
    return sum(min(x + r, n - 1) - max(x - r, 0) + 1 for x in range(n))


def smooth(h, w, r, iters):
    g = torch.Generator().manual_seed(h + r)
    x, guide, out = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(3))
    ops.guided_smooth(x, guide, r, 1e-2, out)          # the workspace of the size exists before anything is timed
    us = _time(lambda: ops.guided_smooth(x, guide, r, 1e-2, out), iters)
    npix = h * w
    # compulsory traffic of the four kernels: image + guide in, 21 float64 planes out | planes in, 12 float32 planes out |
    # those in, 12 float64 planes out | planes + guide in, image out (window re-reads are served by the caches / LDS)
    nbytes = npix * ((24 + 168) + (168 + 48) + (48 + 96) + (96 + 12 + 12))
    # float64 accumulations: a column pass and a row pass per stage, 21 and 12 sums each
    adds = (21 + 12) * (w * extent_sum(h, r) + h * extent_sum(w, r))
    return {"what": "guided_smooth", "h": h, "w": w, "r": r, "iters": iters, "us": round(us, 2),
            "MB_moved": round(nbytes / 1e6, 2), "GBps": round(nbytes / us / 1e3, 1), "f64_adds_M": round(adds / 1e6, 1),
            "f64_Gadds_per_s": round(adds / us / 1e3, 1)}


def trace_only(r, calls=20):
    g = torch.Generator().manual_seed(r)
    x, guide, out = (torch.rand(768, 1024, 3, generator=g).to(DEV) for _ in range(3))
    for _ in range(calls):
        ops.guided_smooth(x, guide, r, 1e-2, out)
    torch.cuda.synchronize()


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "--trace-only":
        return trace_only(int(sys.argv[2]))
    iters = int(os.environ.get("ITERS", "200"))
    for h, w in ((48, 64), (768, 1024)):
        for r in (4, 16, 64):
            print(json.dumps(smooth(h, w, r, iters)), flush=True)


if __name__ == "__main__":
    main()
