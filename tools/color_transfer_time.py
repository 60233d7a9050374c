"""Colour-transfer kernel timings.  One JSON line per size: device events around `iters` back-to-back calls
after a warm-up of strotss_color_hist (10 bases and 1 basis), strotss_color_transfer_table, strotss_color_transfer_apply
(alone and with the next histogram fused) and a whole transfer_colour of T = 10 at 48 x 64 and 768 x 1024, with the bytes
each moves and the bandwidth that makes."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import torch

from nn import _hip
from nn import _ops as ops
from nn import strotss_utils as U

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


def kernels(h, w, iters, T=U.DEFAULT_TRANSFER_ITERS, bins=U.TRANSFER_BINS):
    g = torch.Generator().manual_seed(h)
    x, c, out = (torch.rand(h, w, 3, generator=g).to(DEV) for _ in range(3))
    mask = (torch.rand(h, w, generator=g) > 0.5).float().to(DEV)
    bases = U.transfer_bases(T)
    group = int(_hip.lib().strotss_color_hist_group(bins))
    target = ops.color_hist(c, bases, bins)
    hist = ops.color_hist(x, bases[:1], bins)[0].clone()
    nxt = torch.empty_like(hist)
    table = ops.color_transfer_table(hist, target[0], bases[0], bins)
    res = {"what": "color_transfer_kernels", "h": h, "w": w, "iters": iters, "T": T, "bins": bins, "hist_group": group}
    image, plane, counts = 12 * h * w, 4 * h * w, 12 * bins          # bytes of an image, a weight plane, a (3, bins) histogram
    reads = -(-T // group)                                           # the image is read once per group of bases
    for name, fn, nbytes in (
            ("color_hist_T", lambda: ops.color_hist(c, bases, bins, out=target), reads * image + 2 * T * counts),
            ("color_hist_1", lambda: ops.color_hist(x, bases[:1], bins, out=hist[None]), image + 2 * counts),
            ("color_hist_1_masked", lambda: ops.color_hist(x, bases[:1], bins, mask, out=hist[None]),
             image + plane + 2 * counts),
            ("table", lambda: ops.color_transfer_table(hist, target[0], bases[0], bins, out=table), 3 * counts + 12),
            ("apply", lambda: ops.color_transfer_apply(x, bases[0], table, bins, out=out), 2 * image),
            ("apply_next_hist", lambda: ops.color_transfer_apply(x, bases[0], table, bins, out=out, next_basis=bases[1],
                                                                 next_hist=nxt), 2 * image + 2 * counts),
            ("apply_next_hist_masked", lambda: ops.color_transfer_apply(x, bases[0], table, bins, mask, out=out,
                                                                        next_basis=bases[1], next_hist=nxt),
             2 * image + plane + 2 * counts)):
        us = _time(fn, iters)
        res[f"{name}_us"] = round(us, 2)
        res[f"{name}_GBps"] = round(nbytes / us / 1e3, 1)
    # the whole transfer, host checks and allocations included: 2 T + 2 kernel launches
    res["transfer_launches"] = 2 * T + 2
    res["transfer_us"] = round(_time(lambda: U.transfer_colour(x, c, iters=T, bins=bins), max(1, iters // 10), warm=3), 1)
    return res


def main():
    iters = int(os.environ.get("ITERS", "200"))
    for h, w in ((48, 64), (768, 1024)):
        print(json.dumps(kernels(h, w, iters)), flush=True)


if __name__ == "__main__":
    main()
