"""Sliced Wasserstein style term timings.  One JSON line per measurement; device events around `iters` back-to-back
calls after a warm-up, the forms alternated, three repeats.
  - the operator at n = ns = 1024, D = 2179: strotss_sliced_cos_fwd_bwd with 64, 256 and 1024 directions beside the relaxed EMD
    (strotss_remd_cos_fwd_bwd_panels) and the Sinkhorn step entry at its defaults, each after the content loss's prologue;
    the prologue is timed on its own and is not counted (the step pays it for the content term anyway);
  - a whole 1024-px step (device draw, captured graph, built as bench.py builds its engine): remd, sinkhorn and sliced.
ITERS sets the calls per measurement (default 50; the steps take a fifth of it)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tools")]
import torch

from nn import _ops as ops
from nn import engine
from transport_time import D, DEV, N, _feat, _time

PROJECTIONS = (64, 256, 1024)
LAUNCHES = 7        # directions 1, projections 2, sort/match 1, row dots 1, backward GEMM 1, finish 1


def operator(iters):
    pred, content, style = _feat(N, 1), _feat(N, 2), _feat(N, 3)
    st = engine.StyleTarget.build(style, N, D)
    gp, gtmp = torch.zeros_like(pred), torch.zeros_like(pred)
    lo = torch.zeros(4, dtype=torch.float32, device=DEV)
    counter = torch.zeros(1, dtype=torch.int32, device=DEV)

    def prologue():
        ops.selfsim_fwd_bwd(pred, content, N, D, 1.0, gtmp, lo[1:])

    def remd():
        prologue()
        ops.remd_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, N, pred, N, D, 1.0, gp, lo)

    def sinkhorn():
        prologue()
        ops.sinkhorn_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, N, pred, N, D, engine.DEFAULT_SINKHORN_L,
                                               engine.DEFAULT_SINKHORN_ITERS, 1.0, gp, lo)

    def sliced(p):
        def fn():
            prologue()
            ops.sliced_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, N, pred, N, D, p, 0, counter, 1.0, gp, lo)
        return fn

    forms = [("remd", remd), ("sinkhorn", sinkhorn)] + [(f"sliced_p{p}", sliced(p)) for p in PROJECTIONS]
    for rep in range(3):
        out = {"what": "operator", "n": N, "ns": N, "d": D, "rep": rep}
        for name, fn in forms:
            out[name + "_us"] = _time(fn, iters)
        pro = _time(prologue, iters)
        out = {k: (round(v - pro, 1) if k.endswith("_us") else v) for k, v in out.items()}
        out.update(prologue_us=round(pro, 1), sliced_launches=LAUNCHES)
        print(json.dumps(out), flush=True)


def main():
    from transport_time import make_step
    iters = int(os.environ.get("ITERS", "50"))
    operator(iters)
    transports = ("remd", "sinkhorn", "sliced")
    steps = {t: make_step(1024, t) for t in transports}
    for rep in range(3):
        for t in transports:
            print(json.dumps({"what": "step", "px": 1024, "transport": t, "rep": rep,
                              "projections": engine.DEFAULT_SLICED_PROJECTIONS if t == "sliced" else None,
                              "step_us": round(_time(steps[t], max(10, iters // 5)), 1)}), flush=True)


if __name__ == "__main__":
    main()
