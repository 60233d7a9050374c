"""Child process of tests/test_hip_launch_caps.py: center_kernel, which the moment term reaches only in its f32 GEMM form
(STROTSS_X3_MOMENT=0; the library reads the switch once per process).  strotss_moment_stats and strotss_moment_fwd_bwd on the
step case of tests/_loss_cases.py (1024 rows of 2208 floats: 565248 float4 against 2048 workgroups of 256), with the harness
of tests/_loss_harness.py (NaN-filled workspaces, a seeded base).  Prints one JSON line: {"stats": [figures, failures],
"fwd_bwd": [figures, failures]}."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.dirname(os.path.abspath(__file__))):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np

import _launch_cap_cases as L
import _loss_cases as LC
import _loss_ref as LR
from _loss_harness import fbuf, poison, run_entry

if __name__ == "__main__":
    assert all(os.environ.get(k) == v for k, v in L.CENTER_ENV.items()), "run with STROTSS_X3_MOMENT=0"
    from nn import _ops as ops
    c = LC.make_case(L.CENTER_LABEL)
    assert (c.ns, c.d) == L.CENTER_SHAPE and (c.n, c.d) == L.CENTER_SHAPE
    bx, by = fbuf(c.x), fbuf(c.y)
    ops.moment_stats(bx, c.ns, c.d)                         # the workspace takes its size
    poison(ops)
    mean, cov = ops.moment_stats(bx, c.ns, c.d)
    stats = L.center_stats_judge(mean[:c.d].double().cpu().numpy(), cov[:c.d, :c.d].double().cpu().numpy(), c.x)
    l, g, b, _ = LR.moment(c.x, c.y)
    gs = 1.5
    got, loss, _ = run_entry(ops, lambda gp, lo: ops.moment_fwd_bwd(mean, cov, by, c.n, c.d, gs, gp, lo[0]), c.n, c.d,
                             np.abs(g).max() * gs, 2)
    print(json.dumps({"stats": stats, "fwd_bwd": L.center_grad_judge(float(loss[0, 0]), got / gs, c.x, c.y)}))
