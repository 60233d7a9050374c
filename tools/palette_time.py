"""Sliced palette term timings.  One JSON line per measurement; device events around `iters` back-to-back calls
after a warm-up, the forms alternated, three repeats.
  - the operator at n = ns = 1024, D = 2179: strotss_palette_sliced_fwd_bwd with 16, 64 and 256 directions beside the palette
    relaxed EMD (strotss_palette_remd_fwd_bwd);
  - a whole 1024-px step (device draw, captured graph, built as bench.py builds its engine): palette_transport remd and sliced
    under style_transport remd and sliced.  With palette_transport sliced and style_transport remd the step leaves the grouped
    13-launch loss call for the 21 separate launches: run the tool again under STROTSS_GROUPED_LOSSES=0 (read once per
    process) to time the remd / remd step on the separate launches too; every step line says which form ran ("grouped").
ITERS sets the calls per measurement (default 50; the steps take a fifth of it)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tools")]
import torch

from nn import _ops as ops
from nn import engine, rand
from transport_time import D, DEV, N, _feat, _time, make_step

PROJECTIONS = (16, 64, 256)
LAUNCHES = 2        # sort/match 1, finish 1
REMD_LAUNCHES = 4   # prepare 1, minima 1, select 1, backward 1


def operator(iters):
    pred, style = _feat(N, 1), _feat(N, 3)
    gp = torch.zeros_like(pred)
    lo = torch.zeros(4, dtype=torch.float32, device=DEV)
    dirs = {p: torch.from_numpy(rand.palette_directions(p)).to(DEV) for p in PROJECTIONS}

    def remd():
        ops.palette_remd_fwd_bwd(style, N, pred, N, 1.0, gp, lo)

    def sliced(p):
        return lambda: ops.palette_sliced_fwd_bwd(style, N, pred, N, dirs[p], 1.0, gp, lo)

    forms = [("remd", remd)] + [(f"sliced_p{p}", sliced(p)) for p in PROJECTIONS]
    for rep in range(3):
        out = {"what": "operator", "n": N, "ns": N, "d": D, "rep": rep}
        for name, fn in forms:
            out[name + "_us"] = round(_time(fn, iters), 1)
        out.update(sliced_launches=LAUNCHES, remd_launches=REMD_LAUNCHES)
        print(json.dumps(out), flush=True)


def main():
    iters = int(os.environ.get("ITERS", "50"))
    operator(iters)
    grouped = bool(ops.step_losses_available())
    forms = [(t, p) for t in ("remd", "sliced") for p in ("remd", "sliced")]
    steps = {(t, p): make_step(1024, t, palette_transport=p) for t, p in forms}
    for rep in range(3):
        for t, p in forms:
            print(json.dumps({"what": "step", "px": 1024, "style_transport": t, "palette_transport": p, "rep": rep,
                              "projections": engine.DEFAULT_PALETTE_PROJECTIONS if p == "sliced" else None,
                              "grouped": grouped and t == "remd" and p == "remd",
                              "step_us": round(_time(steps[(t, p)], max(10, iters // 5)), 1)}), flush=True)


if __name__ == "__main__":
    main()
