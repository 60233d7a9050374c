"""Colour-preservation kernel timings.  One JSON line per size: device events around `iters` back-to-back calls
after a warm-up of strotss_color_stats (with and without a weight plane), strotss_color_affine and strotss_luma_merge at
48 x 64 and 768 x 1024, with the bytes each moves and the bandwidth that makes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import numpy as np
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


def kernels(h, w, iters):
    g = torch.Generator().manual_seed(h)
    x, y, out = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(3))
    mask = (torch.rand(h, w, generator=g) > 0.5).float().to(DEV)
    A = np.eye(3) + 0.1 * np.random.default_rng(0).standard_normal((3, 3))
    b = np.array([0.1, -0.05, 0.02])
    ops.color_stats(x)                                 # the workspace of the size exists before anything is timed
    res = {"what": "color_kernels", "h": h, "w": w, "iters": iters}
    image, plane = 12 * h * w, 4 * h * w               # bytes of an image and of a weight plane
    for name, fn, nbytes in (("color_stats", lambda: ops.color_stats(x), image),
                             ("color_stats_masked", lambda: ops.color_stats(x, mask), image + plane),
                             ("color_affine", lambda: ops.color_affine(x, A, b, None, out), 2 * image),
                             ("color_affine_masked", lambda: ops.color_affine(x, A, b, mask, out), 2 * image + plane),
                             ("luma_merge", lambda: ops.luma_merge(x, y, out), 3 * image)):
        us = _time(fn, iters)
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_GBps"] = round(nbytes / us / 1e3, 1)
    return res


def main():
    iters = int(os.environ.get("ITERS", "200"))
    for h, w in ((48, 64), (768, 1024)):
        print(json.dumps(kernels(h, w, iters)), flush=True)


if __name__ == "__main__":
    main()
