"""Timing of --refine_masks.

    python tools/refine_time.py CONTENT STYLE [--k 5] [--calls 50]
        device-event time of strotss_refine_labels (both launches) at 1024 x 683 with the content's own label grid from
        --auto_masks K, and at 1024 x 1024 with a 64 x 64 grid of random labels: microseconds per call, the compulsory
        16 bytes per pixel as a share of the HBM rate, float64 exponentials per second
    python tools/refine_time.py CONTENT STYLE --wall [--k 5]
        wall clock of run_strotss.run() at --max_size 1024 with --auto_masks K, alternating with and without --refine_masks
    python tools/refine_time.py --summarise DIR
        per-launch times of the two kernels from the *_kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

HBM_BYTES_PER_S = 8.0e12                 # MI355X: 8 TB/s


def summarise(src: str) -> None:
    hits = sorted(glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *_kernel_trace.csv under {src}")
    groups = {}
    with open(hits[0]) as f:
        for r in csv.DictReader(f):
            if "refine_" not in r["Kernel_Name"]:
                continue
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            groups.setdefault((name, int(r["Grid_Size_X"])), []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# kernel  grid_threads  calls  median_us  min_us  max_us")
    for (name, grid), us in sorted(groups.items()):
        print(f"{name} {grid} {len(us)} {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}")


def window_cells(n: int, g: int, radius: int) -> int:
    """sum over the n pixel rows (columns) of the number of grid rows (columns) in the pixel's clipped window"""
    total = 0
    for y in range(n):
        i = min(y * g // n, g - 1)
        total += min(g - 1, i + radius) - max(0, i - radius) + 1
    return total


def time_entry(torch, _ops, U, image, grid, k, calls, what):
    h, w = int(image.shape[0]), int(image.shape[1])
    gh, gw = int(grid.shape[0]), int(grid.shape[1])
    args = (image, grid, k, U.REFINE_RADIUS, U.REFINE_SIGMA_S, U.REFINE_SIGMA_R)
    for _ in range(5):
        _ops.refine_labels(*args)
    torch.cuda.synchronize()
    times = []
    for _ in range(calls):
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        _ops.refine_labels(*args)
        stop.record()
        stop.synchronize()
        times.append(1e3 * start.elapsed_time(stop))
    us = statistics.median(times)
    exps = window_cells(h, gh, U.REFINE_RADIUS) * window_cells(w, gw, U.REFINE_RADIUS)
    rate = 16.0 * h * w / (us * 1e-6)
    print(f"{what}: {h} x {w}, grid {gh} x {gw}, k {k}: median {us:.1f} us per call (min {min(times):.1f}, both launches, "
          f"{calls} calls); 16 B/pixel = {rate / 1e9:.0f} GB/s = {100 * rate / HBM_BYTES_PER_S:.1f} % of HBM; "
          f"{exps / (h * w):.1f} float64 exp per pixel = {exps / (us * 1e-6) / 1e9:.0f} G exp/s")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--wall", action="store_true")
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import torch
    import run_strotss as RS
    from nn import _ops, utils
    from nn import strotss_utils as U
    from nn.model import VGG
    content_path, style_path = a.paths
    if a.wall:
        out = os.path.join(tempfile.mkdtemp(), "refine_time.jpg")
        base = [content_path, style_path, "--max_size", "1024", "-o", out, "--auto_masks", str(a.k)]
        for extra in ([], ["--refine_masks"]) * 3:
            t0 = time.perf_counter()
            RS.run(RS.build_parser().parse_args(base + extra))
            print(f"run() --auto_masks {a.k} {' '.join(extra) or '(nearest neighbour)'}: {time.perf_counter() - t0:.3f} s")
        return
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    content, style = (utils.load_image(p, max_size=1024) for p in (content_path, style_path))
    found = U.auto_mask_regions(vgg.params, content, style, a.k)
    if not found["kept"]:
        raise SystemExit(f"--auto_masks {a.k} found fewer than two regions on this pair")
    time_entry(torch, _ops, U, content[0].contiguous(), found["content_grid"].contiguous(), found["kept"], a.calls,
               "the content's own grid")
    gen = torch.Generator(device="cpu").manual_seed(0)
    image = torch.rand((1024, 1024, 3), generator=gen).to(content.device)
    grid = torch.randint(0, a.k, (64, 64), generator=gen, dtype=torch.int32).to(content.device)
    time_entry(torch, _ops, U, image, grid, a.k, a.calls, "uniform noise, random labels")


if __name__ == "__main__":
    main()
