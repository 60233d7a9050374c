#!/usr/bin/env python3
"""HIP-event time of strotss_detail_map (--sample_map auto): the minimum of 7 windows of 100 replays
of one captured call, and of 100 eager calls, against the time 40 bytes per pixel take at the HBM's peak.
usage: python tools/detail_map_time.py [H W R]..."""
import json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
    sys.path.insert(0, p)
import torch
from nn import _ops

HBM_PEAK = 8.0e12            # bytes per second, MI355X
BYTES_PER_PIXEL = 12 + 8 + 8 + 4 + 4 + 4     # img read, plane written, plane read, s written, s read, out written


def windows(fn, n=7, reps=100):
    best = float("inf")
    for _ in range(n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize(); e0.record()
        for _ in range(reps):
            fn()
        e1.record(); torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) / reps * 1e3)
    return best


args = [int(a) for a in sys.argv[1:]]
cases = [tuple(args[i:i + 3]) for i in range(0, len(args), 3)] or [(1024, 1024, 16), (1024, 1024, 4), (1024, 1024, 64), (512, 384, 8)]
for h, w, r in cases:
    img = torch.rand((h, w, 3), device="cuda")
    for _ in range(3):
        _ops.detail_map(img, r)
    eager = windows(lambda: _ops.detail_map(img, r))
    side = torch.cuda.Stream()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.stream(side):
        _ops.detail_map(img, r)
        side.synchronize()
        with torch.cuda.graph(graph, stream=side):
            out = _ops.detail_map(img, r)
    torch.cuda.synchronize()
    replay = windows(graph.replay)
    assert torch.equal(out, _ops.detail_map(img, r))
    bound = BYTES_PER_PIXEL * h * w / HBM_PEAK * 1e6
    print(json.dumps({"what": "detail_map", "h": h, "w": w, "r": r, "windows": 7, "replays": 100, "us_replay_min": round(replay, 2),
                      "us_eager_min": round(eager, 2), "MB_moved": round(BYTES_PER_PIXEL * h * w / 1e6, 2),
                      "us_hbm_bound": round(bound, 2), "ratio_to_bound": round(replay / bound, 1)}), flush=True)
