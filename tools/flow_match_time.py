"""Timings of the optical flow's patch-matching stage, by tools/flow_time.py's method: one JSON line per
measurement; device events around `iters` back-to-back calls after a warm-up, match_radius 0 and 2 alternated, three
repeats, at 48 x 64, 192 x 256 and 768 x 1024 with the default parameters (params = None: the solver form the library
picks at the size)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tests")]
import torch

from nn import _ops as ops
from flow_time import DEV, _pair, _time


def main():
    iters = int(os.environ.get("ITERS", "10"))
    import _flow_ref as R
    for h, w in ((48, 64), (192, 256), (768, 1024)):
        a, b = _pair(h, w)
        out = torch.empty(h, w, 2, device=DEV)
        levels = len(R.level_sizes(h, w))
        for rep in range(3):                          # alternated: without, with
            for r in (0, 2):
                us = _time(lambda: ops.optical_flow(a, b, None, out, match_radius=r), iters)
                print(json.dumps({"what": "flow_match", "h": h, "w": w, "match_radius": r, "rep": rep, "levels": levels,
                                  "stage_launches": levels if r else 0, "flow_us": round(us, 1)}), flush=True)


if __name__ == "__main__":
    main()
