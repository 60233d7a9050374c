"""Timings of the robust optical flow, by tools/flow_match_time.py's method: one JSON line per measurement;
device events around `iters` back-to-back calls after a warm-up, robust off and on alternated, three repeats, at 48 x 64,
192 x 256 and 768 x 1024 with the default parameters (params = None: the solver form the library picks at the size).  Per
size also the launches of one flow's solver: sweeps, and weight updates when robust."""
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
    p = ops.flow_params()
    for h, w in ((48, 64), (192, 256), (768, 1024)):
        a, b = _pair(h, w)
        out = torch.empty(h, w, 2, device=DEV)
        levels = len(R.level_sizes(h, w))
        per_launch = p.iters_per_launch if h * w <= 4096 else 1
        for rep in range(3):                          # alternated: without, with
            for robust in (None, {}):
                us = _time(lambda: ops.optical_flow(a, b, None, out, robust=robust), iters)
                outer = ops.flow_robust_params({}).outer
                print(json.dumps({"what": "flow_robust", "h": h, "w": w, "robust": robust is not None, "rep": rep,
                                  "levels": levels, "sweeps_per_launch": per_launch,
                                  "sweep_launches": levels * p.warps * p.iters // per_launch,
                                  "weight_launches": levels * p.warps * outer if robust is not None else 0,
                                  "flow_us": round(us, 1)}), flush=True)


if __name__ == "__main__":
    main()
