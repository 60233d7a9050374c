"""Timing of --auto_masks.

    python tools/cluster_time.py CONTENT STYLE [--max_size 1024] [--k 5]
        wall clock of the auto-mask stage alone (two trunks, two gathers, the k-means loop; three calls, the first warms up)
        and of run_strotss.run() with and without --auto_masks K
    python tools/cluster_time.py --summarise DIR
        per-launch times of the k-means kernels from the *_kernel_trace.csv of a `rocprofv3 --kernel-trace --stats` run
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


def summarise(src: str) -> None:
    hits = sorted(glob.glob(os.path.join(src, "**", "*_kernel_trace.csv"), recursive=True))
    if not hits:
        raise SystemExit(f"no *_kernel_trace.csv under {src}")
    groups = {}
    with open(hits[0]) as f:
        for r in csv.DictReader(f):
            if "kmeans" not in r["Kernel_Name"]:
                continue
            name = r["Kernel_Name"].replace("(anonymous namespace)::", "").replace("void ", "").split("(")[0]
            key = (name, int(r["Grid_Size_X"]) * int(r.get("Grid_Size_Y", 1) or 1))
            groups.setdefault(key, []).append((int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)
    print("# kernel  grid_threads  calls  median_us  min_us  max_us")
    for (name, grid), us in sorted(groups.items()):
        print(f"{name} {grid} {len(us)} {statistics.median(us):.1f} {min(us):.1f} {max(us):.1f}")


def main() -> None:
    ap = argparse.ArgumentParser()
    ap.add_argument("paths", nargs="*")
    ap.add_argument("--max_size", type=int, default=1024)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--summarise", default=None)
    a = ap.parse_args()
    if a.summarise:
        return summarise(a.summarise)
    import torch
    import run_strotss as RS
    from nn import strotss_utils as U
    from nn import utils
    from nn.model import VGG
    content_path, style_path = a.paths
    vgg = VGG(use_keras_weight=False, weights=None, seed=0, device=utils.device())
    content, style = (utils.load_image(p, max_size=a.max_size) for p in (content_path, style_path))
    for call in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        found = U.auto_mask_regions(vgg.params, content, style, a.k)
        torch.cuda.synchronize()
        print(f"auto-mask stage, call {call}: {1e3 * (time.perf_counter() - t0):.1f} ms, {found['kept']} regions of K = {a.k}, "
              f"counts {found['counts'].tolist()}")
    out = os.path.join(tempfile.mkdtemp(), "cluster_time.jpg")
    for extra in ([], ["--auto_masks", str(a.k)], [], ["--auto_masks", str(a.k)]):
        args = RS.build_parser().parse_args([content_path, style_path, "--max_size", str(a.max_size), "-o", out] + extra)
        t0 = time.perf_counter()
        RS.run(args)
        print(f"run() {' '.join(extra) or 'plain'}: {time.perf_counter() - t0:.2f} s")


if __name__ == "__main__":
    main()
