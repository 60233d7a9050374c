"""Child process of test_full_scale_winograd_vs_direct: ONE whole scale of the CLI's schedule (200 RMSprop steps at the
given size, 128 px by default, through `run_strotss.run`, hipGraph replay, per-step host index draws from seed 0) under the
convolution form the environment selects (STROTSS_WINOGRAD is read once per process); writes the per-step losses, the
output image and the convolution routes the trunk's layers took."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np
import torch

import _route_cases as RC

if __name__ == "__main__":
    out_path, content, style = sys.argv[1], sys.argv[2], sys.argv[3]
    lr = sys.argv[4] if len(sys.argv) > 4 else "2e-3"
    size = sys.argv[5] if len(sys.argv) > 5 else "128"
    k = {"128": 1, "256": 2}[size]                  # the schedule's scale k has a long side of 64 * 2^k
    import run_strotss
    args = run_strotss.build_parser().parse_args([content, style, "-o", out_path + ".jpg", "--max_size", size,
                                                  "--start_level", str(k), "--level", str(k + 1), "--max_iter", "200", "--log_every", "200", "--lr", lr])
    trace = []
    final = run_strotss.run(args, trace=trace)
    rec = trace[0]
    losses = np.array([[s["loss"], s["loss_c"], s["loss_s"]] for s in rec["steps"]], np.float64)
    h, w = rec["hw"]
    np.savez(out_path + ".npz", losses=losses, final=rec["final"].cpu().numpy(), u8=final.cpu().numpy(),
             routes=np.array(sorted(RC.routes_at(h, w))))
