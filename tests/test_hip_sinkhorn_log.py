"""The log-domain Sinkhorn term on the GPU: strotss_sinkhorn_log_cos_fwd_bwd_panels element by element
against float64 autograd of the restatement in tests/_sinkhorn_log_ref.py at every case of tests/_sinkhorn_log_cases.py,
against the linear entry where that engages no clamp, its determinism, refusals and workspace size; then
StepEngine(style_transport="sinkhorn", sinkhorn_log=True) against the float64 restatement of the step, the bits of the
engines the switch does not concern, graph capture, and the command line.

The operator is called the way the step calls it: the content loss first (its workspace then holds the prediction rows'
reciprocal norms and x3 panels), then nn._ops.sinkhorn_log_cos_fwd_bwd_after_selfsim.  Run as a script with the argument
"x3_off" (a child process under STROTSS_X3=0, where no panels exist and the cost matrix runs on the f32 MFMA) this file
makes the operator comparisons again and prints one JSON line."""
import ctypes as C
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if __name__ == "__main__":
    sys.path[:0] = [ROOT, os.path.join(ROOT, "strotss-tensorflow_amd"), os.path.join(ROOT, "tests")]

import _sinkhorn_log_cases as LC
import _sinkhorn_log_ref as LR
import _sinkhorn_ref as SR
import _transport_cases as TC
import _transport_ref as TR
from _loss_harness import DEV, LC_pad, SENTINEL, fbuf, report, run_entry
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

EINVAL, EALIGN, ERANGE = -1, -2, -3
GSCALES = (1.0, 0.37)


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@functools.lru_cache(maxsize=None)
def ref64(label):
    c = LC.make_case(label)
    return LR.run(c.x, c.y, c.l, c.T)


def entry(ops, c, l, T, gs, log=True):
    """fn(gpred, loss4): the content loss on the prediction rows (gradient and loss to scratch), then the step's Sinkhorn
    term (log: the log-domain entry) borrowing from its workspace"""
    bx, by = fbuf(c.x), fbuf(c.y)
    rs, xs = ops.row_inv_norm(bx, c.ns), ops.row_inv_norm_x3(bx, c.ns)[1]
    content = by.clone()
    gtmp, ltmp = torch.zeros_like(by), torch.zeros(4, dtype=torch.float32, device=DEV)
    term = ops.sinkhorn_log_cos_fwd_bwd_after_selfsim if log else ops.sinkhorn_cos_fwd_bwd_after_selfsim

    def fn(gp, lo):
        ops.selfsim_fwd_bwd(by, content, c.n, c.d, 1.0, gtmp, ltmp)
        term(bx, rs, xs, c.ns, by, c.n, c.d, l, T, gs, gp, lo[0])
    return fn


def check_case(ops, c, ref_l, ref_g):
    """the comparisons of one case at both gscales, into a seeded gpred and a zeroed one; returns the zero-base gradient"""
    tol = LR.TOL_SK[LR.family(c)]
    losses, zero_base = [], []
    for k, gs in enumerate(GSCALES):
        got, loss, g0 = run_entry(ops, entry(ops, c, c.l, c.T, gs), c.n, c.d, np.abs(ref_g).max() * gs, 70 + k)
        what = f"sinkhorn_log:g{gs}"
        rel = abs(loss[0, 0] - ref_l) / abs(ref_l)
        report(f"scalar:{what}", c.label, f"{rel:.3e}")
        for name, g in ((what, got / gs), (what + ":zero_base", g0.astype(np.float64) / gs)):
            err = LR.err_over_max(g, ref_g)
            report(f"grad:{name}", c.label, f"max {err:.3e} of tol {tol:.3e}")
            assert np.isfinite(g).all() and (np.abs(g - ref_g) <= tol * np.abs(ref_g).max()).all(), (name, err, tol)
        assert rel <= LR.TOL_SCALAR, (what, loss[0, 0], ref_l)
        assert not loss.flatten()[1:].any()
        losses.append(loss[0, 0])
        zero_base.append(g0)
    assert losses[0] == losses[1], "the loss depends on gscale"
    return zero_base[0]


@pytest.mark.parametrize("label", LC.LABELS)
def test_log_entry_matches_float64(ops, label):
    check_case(ops, LC.make_case(label), *ref64(label))


def test_cases_without_x3_panels_in_a_child_process():
    """STROTSS_X3=0 is read once per process: a fresh child makes the comparisons of test_log_entry_matches_float64"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "x3_off"], env=dict(os.environ, STROTSS_X3="0"),
                         capture_output=True, text=True, timeout=600)
    print(out.stdout[-8000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    assert res["cases"] == len(LC.LABELS) and res["panels"] is False


@pytest.mark.parametrize("c", LC.conditioned_linear_cases(), ids=lambda c: c.label)
def test_log_entry_agrees_with_the_linear_entry_where_no_clamp_acts(ops, c):
    """L = 10, the case's own T (at which tests/test_sinkhorn_cases_cpu.py asserts the conditioning): both entries lie within
    their tolerance of the same float64 function, so within the sum of the two of each other"""
    out = []
    for log in (False, True):
        g = torch.zeros((LC_pad(c.n), LC_pad(c.d)), dtype=torch.float32, device=DEV)
        lo = torch.zeros(4, 4, dtype=torch.float32, device=DEV)
        entry(ops, c, 10.0, c.T, 1.0, log)(g, lo)
        torch.cuda.synchronize()
        out.append((g[:c.n, :c.d].double().cpu().numpy(), float(lo[0, 0])))
    (g_lin, l_lin), (g_log, l_log) = out
    tol = SR.TOL_SK["cosine"] + LR.TOL_SK["l10"]
    if c.d == 1:                                          # every cosine distance is 0: so are both losses and gradients
        assert max(abs(l_lin), abs(l_log), np.abs(g_lin).max(), np.abs(g_log).max()) <= 2e-6
        return
    scale = np.abs(g_lin).max()
    report("grad:log_vs_linear", c.label, f"{np.abs(g_log - g_lin).max() / scale:.3e} of tol {tol:.3e}")
    assert (np.abs(g_log - g_lin) <= tol * scale).all() and abs(l_log - l_lin) <= 2.0 * LR.TOL_SCALAR * abs(l_lin)


def test_two_calls_and_two_streams_give_the_same_bits(ops):
    c = LC.make_case("ns600_n768_d2179_L100")
    fn = entry(ops, c, c.l, c.T, 1.0)
    out = []
    for stream in (torch.cuda.current_stream(), torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()):
        g = torch.zeros((LC_pad(c.n), LC_pad(c.d)), dtype=torch.float32, device=DEV)
        lo = torch.zeros(4, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            fn(g, lo)
        torch.cuda.synchronize()
        out.append((g, lo))
    for g, lo in out[1:]:
        assert torch.equal(g, out[0][0]) and torch.equal(lo, out[0][1])
    assert bool(out[0][0].any())


def test_refusals_leave_outputs_and_workspace_untouched_and_the_size_is_exact(ops):
    from nn import _hip
    lib = _hip.lib()
    c = LC.make_case("ns65_n63")                          # d = 35: a row stride of 48 holds the rows and is no multiple of 32
    bx, by = fbuf(c.x), fbuf(c.y)
    rs, xs = ops.row_inv_norm_x3(bx, c.ns)
    rp, xp = ops.row_inv_norm_x3(by, c.n)
    by48 = torch.zeros((LC_pad(c.n), 48), dtype=torch.float32, device=DEV)
    by48[:c.n, :c.d] = by[:c.n, :c.d]
    g = torch.full((LC_pad(c.n), LC_pad(c.d)), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    bytes_ = lib.strotss_sinkhorn_log_step_workspace_bytes
    nb = bytes_(c.ns, c.n, c.T)
    assert nb > 0 and bytes_(0, 1, 1) == 0 and bytes_(1, 0, 1) == 0 and bytes_(1, 1, 0) == 0 and bytes_(1, 1, 65) == 0
    assert bytes_(-3, 5, 5) == 0 and bytes_(1, 1, 64) > 0
    # no K matrix: one n x ns matrix less than the linear entry's workspace
    assert nb < lib.strotss_sinkhorn_step_workspace_bytes(c.ns, c.n, c.T)
    ws = torch.full((nb + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    p, f = _hip.ptr, C.c_float

    def call(style=bx, rs_=rs, xs_=xs, ns=c.ns, pred=by, rp_=rp, xp_=xp, n=c.n, ld=by.shape[1], l=10.0, T=c.T, nbytes=nb,
             gp=g, lo=loss, w=ws):
        return lib.strotss_sinkhorn_log_cos_fwd_bwd_panels(p(style), p(rs_), p(xs_), ns, p(pred), p(rp_), p(xp_), n, c.d, ld, f(l),
                                                           T, f(1.0), p(gp), p(lo), p(w), nbytes, _hip.stream_ptr())
    assert call(T=0) == ERANGE and call(T=65) == ERANGE and call(T=-1) == ERANGE
    assert call(l=0.0) == ERANGE and call(l=-1.0) == ERANGE and call(l=float("inf")) == ERANGE and call(l=float("nan")) == ERANGE
    assert call(l=1000.5) == ERANGE and call(l=float(np.nextafter(np.float32(1000.0), np.float32(2000.0)))) == ERANGE
    assert call(pred=by48, ld=48) == EALIGN
    assert call(ns=0) == EINVAL and call(n=0) == EINVAL and call(nbytes=nb - 1) == EINVAL and call(nbytes=0) == EINVAL
    assert call(style=None) == EINVAL and call(rs_=None) == EINVAL and call(pred=None) == EINVAL and call(rp_=None) == EINVAL
    assert call(gp=None) == EINVAL and call(lo=None) == EINVAL and call(w=None) == EINVAL
    assert call(xs_=None) == EINVAL and call(xp_=None) == EINVAL              # the panels come as a pair
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((loss == SENTINEL).all()) and bool((ws == 0x5A).all())
    # the same arguments unspoiled are accepted, at exactly the size the bytes entry gives: nothing past it is written
    assert call() == 0 and call(xs_=None, xp_=None) == 0 and call(l=1000.0) == 0
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool((loss[1:] == SENTINEL).all()) and float(loss[0]) != SENTINEL
    assert bool((ws[nb:] == 0x5A).all()) and not bool((ws[:nb] == 0x5A).all())


# ------------------------------------------------------------------ the step
def _engine(P, blend_weights=None, deterministic=None, **kw):
    from nn import _ops, engine
    from nn.model import VGGParams
    params = VGGParams(P["weights"], '16', None, DEV)
    cfeat = engine.extract_features(params, P["content"].to(DEV))
    sfeats = [engine.extract_features(params, s.to(DEV)) for s in P["styles"]]
    targets = []
    for sets in P["s_idx"]:
        ts = [engine.StyleTarget.build(_ops.hypercol_gather(sf, torch.from_numpy(si).to(DEV), False), si.shape[0], 2179)
              for sf, si in zip(sfeats, sets)]
        targets.append(ts[0] if blend_weights is None else engine.StyleBlend(ts, list(blend_weights)))
    c64, s64 = P["content"].double(), P["styles"][0].double()
    init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic, **kw)


def _check_step(P, L, blend_weights=None):
    import test_hip_engine as THE
    eng = _engine(P, blend_weights, style_transport="sinkhorn", sinkhorn_l=L, sinkhorn_iters=30, sinkhorn_log=True)
    eng.forward_backward([torch.from_numpy(i).to(DEV) for i in P["idx"]])
    torch.cuda.synchronize()
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(P["weights"], dtype=torch.float64)), eng)
    ref = LR.reference_step(P, L, 30, blend_weights=blend_weights, vgg=vgg)
    got = eng.losses()
    tol_s, tol_g = LR.step_bounds(L)
    assert got["l_sinkhorn"] == got["l_remd"] > 0
    for k in ("loss", "loss_c", "loss_s"):
        rel = abs(got[k] - float(ref[k])) / max(1.0, abs(float(ref[k])))
        report(f"step:{k}", f"{eng.h}x{eng.w}:L{L:g}", f"{rel:.3e}")
        assert rel < tol_s, (k, got[k], float(ref[k]))
    for k, (g, gr) in enumerate(zip(eng.gvars, ref["grads"])):
        rel = float((g.cpu().double() - gr).norm() / gr.norm())
        report(f"step:grad_level{k}", f"{eng.h}x{eng.w}:L{L:g}", f"{rel:.3e}")
        assert rel < tol_g, (k, rel)


@pytest.mark.parametrize("L", [10.0, 100.0])
@pytest.mark.parametrize("spec", TC.STEPS, ids=[s[0] for s in TC.STEPS])
def test_log_step_matches_the_float64_restatement(spec, L):
    _, h, w, n, seed, masked = spec
    _check_step(TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None), L)


@pytest.mark.parametrize("L", [10.0, 100.0])
def test_log_blend_step_matches_the_float64_restatement(L):
    _check_step(TR.step_problem(*TC.BLEND_STEP[1:5], n_styles=2), L, blend_weights=TC.BLEND_WEIGHTS)


def test_engine_refuses_what_the_switch_does_not_run_with():
    P = TR.step_problem(64, 64, 128, 1)
    for kw in (dict(sinkhorn_log=True), dict(style_transport="remd", sinkhorn_log=True),
               dict(style_transport="sliced", sinkhorn_log=True),
               dict(style_transport="sinkhorn", sinkhorn_log=True, sinkhorn_l=1000.5),
               dict(style_transport="sinkhorn", sinkhorn_log=True, sinkhorn_iters=65)):
        with pytest.raises(ValueError):
            _engine(P, **kw)


def _run_steps(P, idx, **kw):
    eng = _engine(P, deterministic=True, **kw)
    scalars = []
    for i in idx:
        eng.step(i)
        scalars.append(eng.scalars.clone())
    torch.cuda.synchronize()
    return [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + scalars


def test_the_other_engines_keep_their_bits():
    """sinkhorn_log=False is the omitted argument bit for bit and differs from True; "remd" and "sliced" engines give the
    same bits before and after log-domain steps have run in the process"""
    P = TR.step_problem(64, 64, 256, 9)
    rng = np.random.default_rng(4)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng)).to(DEV)] for _ in range(3)]
    sk = dict(style_transport="sinkhorn", sinkhorn_l=10.0, sinkhorn_iters=30)
    before = {t: _run_steps(P, idx, style_transport=t) for t in ("remd", "sliced")}
    omitted, false = _run_steps(P, idx, **sk), _run_steps(P, idx, sinkhorn_log=False, **sk)
    true = _run_steps(P, idx, sinkhorn_log=True, **sk)
    for a, b in zip(omitted, false):
        assert torch.equal(a, b)
    assert not all(torch.equal(a, b) for a, b in zip(omitted, true))
    for t in ("remd", "sliced"):
        for a, b in zip(before[t], _run_steps(P, idx, style_transport=t)):
            assert torch.equal(a, b), t


def test_captured_log_steps_equal_eager_ones_and_read_nothing_back():
    P = TR.step_problem(64, 64, 256, 11, masks=TC.step_masks(64, 64))
    rng = np.random.default_rng(5)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng, mask=cm)).to(DEV) for cm, _ in TC.step_masks(64, 64)]
           for _ in range(3)]
    kw = dict(style_transport="sinkhorn", sinkhorn_l=100.0, sinkhorn_iters=30, sinkhorn_log=True, deterministic=True)
    finals = []
    for graph in (False, True):
        eng = _engine(P, **kw)
        if graph:
            eng.capture_graph(idx[0])
        else:
            eng.step(idx[0])                  # workspaces take their size: the guarded steps below allocate nothing
            eng = _engine(P, **kw)
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode("error")       # a device-to-host read inside a step raises
        try:
            for i in idx:
                eng.step(i)
        finally:
            torch.cuda.set_sync_debug_mode("default")
        torch.cuda.synchronize()
        finals.append([v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()])
    for a, b in zip(*finals):
        assert torch.equal(a, b), "eager vs graph replay"


# ------------------------------------------------------------------ the command line
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_cli_sinkhorn_log_run(tmp_path, monkeypatch):
    import run_strotss
    from PIL import Image
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    logged = []

    class Bar(run_strotss.tqdm):                      # the progress bar's log line, as it is set
        def set_postfix(self, ordered_dict=None, **kw):
            logged.append(dict(ordered_dict or {}))
            super().set_postfix(ordered_dict, **kw)
    monkeypatch.setattr(run_strotss, "tqdm", Bar)
    out, trace = tmp_path / "log.jpg", []
    run_strotss.run(run_strotss.build_parser().parse_args(
        [os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg"), "-o", str(out), "--max_size", "64",
         "--level", "1", "--max_iter", "30", "--log_every", "30", "--style_transport", "sinkhorn", "--sinkhorn_log",
         "--sinkhorn_reg", "100"]), trace=trace)
    img = np.asarray(Image.open(out), np.float64)
    assert open(out, "rb").read()[:2] == b"\xff\xd8" and np.isfinite(img).all() and img.std() > 0
    steps = trace[0]["steps"]
    assert len(steps) == 30 and all(np.isfinite(s["l_sinkhorn"]) and s["l_sinkhorn"] > 0 for s in steps)
    assert np.isfinite(trace[0]["final"].cpu().numpy()).all()
    assert logged and all(np.isfinite(float(d["sinkhorn"])) for d in logged)          # the log line names the term


def test_cli_sinkhorn_log_video(tmp_path):
    import run_strotss
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three synthetic 48 x 64 frames of the colour test
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    run_strotss.run(run_strotss.build_parser().parse_args(
        [frames, style, "--video", "--compute_flow", "-o", str(tmp_path / "out"), "--max_size", "64", "--level", "1",
         "--max_iter", "30", "--style_transport", "sinkhorn", "--sinkhorn_log", "--sinkhorn_reg", "100"]))
    stems = [os.path.splitext(os.path.basename(q))[0] for q in paths]
    assert len(stems) == 3 and sorted(os.listdir(tmp_path / "out")) == sorted(t + ".jpg" for t in stems)
    for t in stems:
        img = np.asarray(Image.open(tmp_path / "out" / (t + ".jpg")), np.float64)
        assert np.isfinite(img).all() and img.std() > 0


# ------------------------------------------------------------------ the child process
def _child():
    from nn import _hip, _ops
    for label in LC.LABELS:
        c = LC.make_case(label)
        check_case(_ops, c, *LR.run(c.x, c.y, c.l, c.T))
    # what the library hands out in this process: no panels
    c = LC.make_case(LC.LABELS[0])
    by = fbuf(c.y)
    nb = _hip.lib().strotss_selfsim_workspace_bytes(c.n, by.shape[1])
    ws = _ops.workspaces.get("selfsim", nb, by.device)
    rp, xp = C.c_void_p(), C.c_void_p()
    _hip.check(_hip.lib().strotss_selfsim_pred_panels(_hip.ptr(ws), nb, c.n, by.shape[1], C.byref(rp), C.byref(xp)), "panels")
    print(json.dumps({"cases": len(LC.LABELS), "panels": bool(xp.value)}))


if __name__ == "__main__":
    assert sys.argv[1:] == ["x3_off"]
    _child()
