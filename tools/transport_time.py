"""Sinkhorn style term timings.  One JSON line per measurement; device events around `iters` back-to-back calls
after a warm-up, the two forms alternated, three repeats.
  - the operator at n = ns = 1024, D = 2179, T = 30 and T = 10: the plain entry (strotss_sinkhorn_cos_fwd_bwd) against the
    step's (strotss_sinkhorn_cos_fwd_bwd_panels after the content loss's prologue; the prologue is timed on its own and is
    not counted, the step pays it for the content term anyway), with each entry's launch count.  This is the pair a fused
    one-launch-per-scaling form of the iteration was measured with (2436 us against 685 us at T = 30, so it is
    not in the library); a new form of the iteration is timed by putting it behind the step's entry;
  - a whole 1024-px step (device draw, captured graph, built as bench.py builds its engine): remd against sinkhorn.
ITERS sets the calls per measurement (default 50; the steps take a fifth of it).
With --log every operator line also times the log-domain entry (strotss_sinkhorn_log_cos_fwd_bwd_panels) beside
the linear step entry, at L = 10 and at L = 100, and the steps add sinkhorn with sinkhorn_log at L = 100."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd")]
import numpy as np
import torch

from nn import _ops as ops
from nn import engine

DEV = "cuda"
D = 2179
N = 1024


def _feat(n, seed):
    rng = np.random.default_rng(seed)
    x = np.maximum(rng.standard_normal((n, D)), 0) + 0.01 * rng.random((n, D))
    b = torch.zeros(ops.pad32(n), ops.pad32(D), dtype=torch.float32, device=DEV)
    b[:n, :D] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


def _time(fn, iters, warm=5):
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


def launches(T):
    """(plain, step): kernel launches of one call, from the host code of csrc/losses.hip.
    plain: norms 1, cost matrix 1, exp 1, fill 1, 3 T forward, cost 2, 3 T - 1 reverse, assembly 1, backward GEMM 1.
    step:  the same without the norms."""
    return 6 * T + 7, 6 * T + 6


def launches_log(T):
    """the log-domain entry, from the host code of csrc/sinkhorn_log.hip: cost matrix 1, psi_0 memset 1, 3 T forward, cost 2,
    3 T - 1 reverse, assembly 1, backward GEMM 1"""
    return 6 * T + 5


def operator(T, iters, log=False):
    pred, content, style = _feat(N, 1), _feat(N, 2), _feat(N, 3)
    st = engine.StyleTarget.build(style, N, D)
    gp, gtmp = torch.zeros_like(pred), torch.zeros_like(pred)
    lo = torch.zeros(4, dtype=torch.float32, device=DEV)

    def prologue():
        ops.selfsim_fwd_bwd(pred, content, N, D, 1.0, gtmp, lo[1:])

    def plain():
        ops.sinkhorn_cos_fwd_bwd(st.feats, st.inv_norm, N, pred, N, D, 10.0, T, 1.0, gp, lo)

    def step_entry_with_prologue():
        prologue()
        ops.sinkhorn_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, N, pred, N, D, 10.0, T, 1.0, gp, lo)

    def log_entry_with_prologue(L):
        def fn():
            prologue()
            ops.sinkhorn_log_cos_fwd_bwd_after_selfsim(st.feats, st.inv_norm, st.panels, N, pred, N, D, L, T, 1.0, gp, lo)
        return fn

    n_old, n_new = launches(T)
    for rep in range(3):
        old = _time(plain, iters)
        both = _time(step_entry_with_prologue, iters)
        logs = {L: _time(log_entry_with_prologue(L), iters) for L in (10.0, 100.0)} if log else {}
        pro = _time(prologue, iters)
        rec = {"what": "operator", "n": N, "ns": N, "d": D, "T": T, "rep": rep, "plain_us": round(old, 1),
               "plain_launches": n_old, "step_entry_us": round(both - pro, 1), "step_entry_launches": n_new,
               "prologue_us": round(pro, 1)}
        for L, t in logs.items():
            rec[f"log_entry_L{L:g}_us"] = round(t - pro, 1)
        if log:
            rec["log_entry_launches"] = launches_log(T)
        print(json.dumps(rec), flush=True)


def make_step(px, transport, **kw):
    sys.path.insert(0, ROOT)
    import bench
    from nn.model import VGGParams, synthetic_weights
    from nn import strotss_utils as SU
    params = VGGParams(synthetic_weights('16', 0), '16', None, DEV)
    dev = torch.device(DEV, torch.cuda.current_device())
    content, style = bench.synth_image(px, px, 100).to(dev), bench.synth_image(px, px, 200).to(dev)
    rng = np.random.default_rng(0)
    s_idx = torch.from_numpy(SU.make_indices_np(px, px, False, N, rng, None)).to(dev)
    target = engine.StyleTarget.build(ops.hypercol_gather(engine.extract_features(params, style), s_idx, False),
                                      int(s_idx.shape[0]), D)
    init = SU.make_laplacian(content) + style.mean(dim=(1, 2), keepdim=True)
    eng = engine.StepEngine(params, engine.extract_features(params, content), [target], init, 1.0, 4.0, 1e-3, sample_size=N,
                            style_transport=transport, **kw)
    if eng.enable_device_draw(0, 1000, None):
        eng.capture_graph()
        return eng.step
    idx = [torch.from_numpy(SU.make_indices_np(px, px, True, N, rng)).to(dev)]
    eng.capture_graph(idx)
    return lambda: eng.step(idx)


def main():
    iters = int(os.environ.get("ITERS", "50"))
    log = "--log" in sys.argv[1:]
    for T in (30, 10):
        operator(T, iters, log)
    steps = {t: make_step(1024, t) for t in ("remd", "sinkhorn")}
    if log:
        steps["sinkhorn_log_L100"] = make_step(1024, "sinkhorn", sinkhorn_l=100.0, sinkhorn_log=True)
    for rep in range(3):
        for t in steps:
            print(json.dumps({"what": "step", "px": 1024, "transport": t, "rep": rep,
                              "step_us": round(_time(steps[t], max(10, iters // 5)), 1)}), flush=True)


if __name__ == "__main__":
    main()
