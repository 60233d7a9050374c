"""The Sinkhorn style term on the GPU: strotss_sinkhorn_cos_fwd_bwd_panels element by element against
float64 autograd of oracle.sinkhorn_knopp at every cosine case of tests/_sinkhorn_cases.py and at the further sizes of
tests/_transport_cases.py, with the bounds of tests/_sinkhorn_ref.py; then StepEngine(style_transport=
"sinkhorn") against the float64 restatement of the step (tests/_transport_ref.py), the default path's bits, graph capture,
and the command line.

The operator is called the way the step calls it: the content loss first (its workspace then holds the prediction rows'
reciprocal norms and x3 panels), then nn._ops.sinkhorn_cos_fwd_bwd_after_selfsim.  Run as a script with the argument
"x3_off" (a child process under STROTSS_X3=0, where no panels exist and the cost matrix runs on the f32 MFMA) this file
makes the same comparisons and prints one JSON line."""
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

import _sinkhorn_cases as SC
import _sinkhorn_ref as SR
import _transport_cases as TC
import _transport_ref as TR
from _loss_harness import DEV, LC_pad, SENTINEL, fbuf, report, run_entry
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

EINVAL, EALIGN, ERANGE = -1, -2, -3
GSCALES = (1.0, 0.37)
CASES = TC.all_cosine()
IDS = [c.label for c, _ in CASES]
ZERO = "n50_ns40_d1"            # one column: every cosine distance is 0, so are the loss and the gradient


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@functools.lru_cache(maxsize=None)
def ref64(label):
    c, l = [(c, l) for c, l in CASES if c.label == label][0]
    return SR.sinkhorn(c.x, c.y, "cosine", l, c.T)


def entry(ops, c, l, gs):
    """fn(gpred, loss4): the content loss on the prediction rows (gradient and loss to scratch), then the step's Sinkhorn
    term borrowing from its workspace"""
    bx, by = fbuf(c.x), fbuf(c.y)
    rs, xs = ops.row_inv_norm(bx, c.ns), ops.row_inv_norm_x3(bx, c.ns)[1]
    content = by.clone()
    gtmp, ltmp = torch.zeros_like(by), torch.zeros(4, dtype=torch.float32, device=DEV)

    def fn(gp, lo):
        ops.selfsim_fwd_bwd(by, content, c.n, c.d, 1.0, gtmp, ltmp)
        ops.sinkhorn_cos_fwd_bwd_after_selfsim(bx, rs, xs, c.ns, by, c.n, c.d, l, c.T, gs, gp, lo[0])
    return fn


def check_case(ops, c, l, ref_l, ref_g):
    """the comparisons of one case at both gscales, on a zeroed and on a pre-filled gpred; returns the zero-base gradients"""
    tol = SR.TOL_SK[SR.family(c, "cosine")]
    zero = c.label == ZERO
    scale = max(np.abs(ref_g).max(), 1e-3 if zero else 0.0)
    losses, zero_base = [], []
    for k, gs in enumerate(GSCALES):
        got, loss, g0 = run_entry(ops, entry(ops, c, l, gs), c.n, c.d, scale * gs, 50 + k)
        what = f"sinkhorn_step:g{gs}"
        if zero:
            report(f"grad:{what}", c.label, f"max|g| {np.abs(got).max():.3e}")
            assert abs(loss[0, 0]) <= 1e-6 and np.abs(got).max() <= 1e-6 and np.abs(g0).max() <= 1e-6
        else:
            rel = abs(loss[0, 0] - ref_l) / abs(ref_l)
            report(f"scalar:{what}", c.label, f"{rel:.3e}")
            assert rel <= SR.loss_tolerance(c, l), (what, loss[0, 0], ref_l)
            for name, g in ((what, got / gs), (what + ":zero_base", g0.astype(np.float64) / gs)):
                err = SR.err_over_max(g, ref_g)
                report(f"grad:{name}", c.label, f"max {err:.3e} of tol {tol:.3e}")
                assert np.isfinite(g).all() and (np.abs(g - ref_g) <= tol * np.abs(ref_g).max()).all(), (name, err, tol)
        assert not loss.flatten()[1:].any()
        if c.kind == "dup":
            assert np.array_equal(g0[SC.DUP_ROWS[0]], g0[SC.DUP_ROWS[1]]), "duplicate prediction rows differ"
        losses.append(loss[0, 0])
        zero_base.append(g0)
    assert losses[0] == losses[1], "the loss depends on gscale"
    return zero_base


@pytest.mark.parametrize("c,l", CASES, ids=IDS)
def test_fused_entry_matches_float64(ops, c, l):
    ref_l, ref_g = ref64(c.label)
    zero_base = check_case(ops, c, l, ref_l, ref_g)
    # the plain entry on the same case (its own norms, the cost matrix on the f32 MFMA): both lie within TOL_SK of float64, so within twice that of each other
    bx, by = fbuf(c.x), fbuf(c.y)
    rs = ops.row_inv_norm(bx, c.ns)
    g = torch.zeros((LC_pad(c.n), LC_pad(c.d)), dtype=torch.float32, device=DEV)
    lo = torch.zeros(4, dtype=torch.float32, device=DEV)
    ops.sinkhorn_cos_fwd_bwd(bx, rs, c.ns, by, c.n, c.d, l, c.T, 1.0, g, lo)
    torch.cuda.synchronize()
    old = g[:c.n, :c.d].double().cpu().numpy()
    scale = max(np.abs(ref_g).max(), 1e-30)
    diff = float(np.abs(old - zero_base[0]).max())
    report("grad:fused_vs_existing", c.label, f"{diff / scale:.3e}")
    if c.label == ZERO:
        assert diff <= 2e-6
    else:
        assert diff <= 2.0 * SR.TOL_SK[SR.family(c, "cosine")] * scale


def test_two_streams_give_the_same_bits(ops):
    c, l = [(c, l) for c, l in CASES if c.label == "t_n1024_ns1024_T30"][0]
    fn = entry(ops, c, l, 1.0)
    out = []
    for stream in (torch.cuda.current_stream(), torch.cuda.Stream(), torch.cuda.Stream()):
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


def test_refusals_leave_outputs_and_workspace_untouched(ops):
    from nn import _hip
    lib = _hip.lib()
    c = SC.make_case("n65_ns31_T2")                       # d = 35: a row stride of 48 holds the rows and is no multiple of 32
    bx, by = fbuf(c.x), fbuf(c.y)
    rs, xs = ops.row_inv_norm_x3(bx, c.ns)
    rp, xp = ops.row_inv_norm_x3(by, c.n)
    by48 = torch.zeros((LC_pad(c.n), 48), dtype=torch.float32, device=DEV)
    by48[:c.n, :c.d] = by[:c.n, :c.d]
    g = torch.full((LC_pad(c.n), LC_pad(c.d)), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    nb = lib.strotss_sinkhorn_step_workspace_bytes(c.ns, c.n, c.T)
    assert nb >= lib.strotss_sinkhorn_workspace_bytes(c.ns, c.n, c.T) and lib.strotss_sinkhorn_step_workspace_bytes(0, 1, 1) == 0
    ws = torch.full((nb + 64,), 0x5A, dtype=torch.uint8, device=DEV)
    p, f = _hip.ptr, C.c_float

    def call(style=bx, rs_=rs, xs_=xs, ns=c.ns, pred=by, rp_=rp, xp_=xp, n=c.n, ld=by.shape[1], l=10.0, T=c.T, nbytes=nb,
             gp=g, lo=loss, w=ws):
        return lib.strotss_sinkhorn_cos_fwd_bwd_panels(p(style), p(rs_), p(xs_), ns, p(pred), p(rp_), p(xp_), n, c.d, ld, f(l), T,
                                                       f(1.0), p(gp), p(lo), p(w), nbytes, _hip.stream_ptr())
    assert call(T=0) == ERANGE and call(T=65) == ERANGE
    assert call(l=0.0) == ERANGE and call(l=-1.0) == ERANGE and call(l=float("inf")) == ERANGE and call(l=float("nan")) == ERANGE
    assert call(pred=by48, ld=48) == EALIGN
    assert call(ns=0) == EINVAL and call(n=0) == EINVAL and call(nbytes=nb - 1) == EINVAL
    assert call(style=None) == EINVAL and call(rs_=None) == EINVAL and call(rp_=None) == EINVAL and call(gp=None) == EINVAL
    assert call(lo=None) == EINVAL and call(w=None) == EINVAL
    assert call(xs_=None) == EINVAL and call(xp_=None) == EINVAL              # the panels come as a pair
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((loss == SENTINEL).all()) and bool((ws == 0x5A).all())
    assert call() == 0 and call(xs_=None, xp_=None) == 0                      # ... and the same arguments unspoiled are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool((loss[1:] == SENTINEL).all()) and float(loss[0]) != SENTINEL


def test_cases_without_x3_panels_in_a_child_process():
    """STROTSS_X3=0 is read once per process: a fresh child makes the comparisons of test_fused_entry_matches_float64"""
    out = subprocess.run([sys.executable, os.path.abspath(__file__), "x3_off"], env=dict(os.environ, STROTSS_X3="0"),
                         capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    res = json.loads(out.stdout.strip().splitlines()[-1])
    print(out.stdout[-6000:])
    assert res["cases"] == len(CASES) and res["panels"] is False


# ------------------------------------------------------------------ the step
def _engine(P, transport="sinkhorn", l=10.0, T=30, blend_weights=None, deterministic=None, init=None):
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
    if init is None:
        c64, s64 = P["content"].double(), P["styles"][0].double()
        init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    kw = {} if transport is None else dict(style_transport=transport, sinkhorn_l=l, sinkhorn_iters=T)
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic, **kw)


def _check_step(P, blend_weights=None):
    import test_hip_engine as THE
    eng = _engine(P, blend_weights=blend_weights)
    eng.forward_backward([torch.from_numpy(i).to(DEV) for i in P["idx"]])
    torch.cuda.synchronize()
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(P["weights"], dtype=torch.float64)), eng)
    ref = TR.reference_step(P, 10.0, 30, blend_weights=blend_weights, vgg=vgg)
    got = eng.losses()
    assert got["l_sinkhorn"] == got["l_remd"] > 0
    for k in ("loss", "loss_c", "loss_s"):
        rel = abs(got[k] - float(ref[k])) / max(1.0, abs(float(ref[k])))
        report(f"step:{k}", f"{eng.h}x{eng.w}", f"{rel:.3e}")
        assert rel < TR.TOL_SCALAR, (k, got[k], float(ref[k]))
    for k, (g, gr) in enumerate(zip(eng.gvars, ref["grads"])):
        rel = float((g.cpu().double() - gr).norm() / gr.norm())
        report(f"step:grad_level{k}", f"{eng.h}x{eng.w}", f"{rel:.3e}")
        assert rel < TR.GRAD_TOL, (k, rel)


@pytest.mark.parametrize("spec", TC.STEPS, ids=[s[0] for s in TC.STEPS])
def test_sinkhorn_step_matches_the_float64_restatement(spec):
    _, h, w, n, seed, masked = spec
    _check_step(TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None))


def test_sinkhorn_blend_step_matches_the_float64_restatement():
    _check_step(TR.step_problem(*TC.BLEND_STEP[1:5], n_styles=2), blend_weights=TC.BLEND_WEIGHTS)


def test_engine_refuses_what_the_term_does_not_run_with():
    P = TR.step_problem(64, 64, 128, 1)
    for kw in (dict(transport="emd"), dict(l=0.0), dict(l=float("nan")), dict(l=float("inf")), dict(T=0), dict(T=65), dict(T=2.5)):
        with pytest.raises(ValueError):
            _engine(P, **kw)


def test_remd_transport_is_the_default_engine_bit_for_bit():
    P = TR.step_problem(64, 64, 256, 9)
    rng = np.random.default_rng(4)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng)).to(DEV)] for _ in range(3)]
    finals = []
    for transport in (None, "remd"):
        eng = _engine(P, transport=transport, deterministic=True)
        scalars = []
        for i in idx:
            eng.step(i)
            scalars.append(eng.scalars.clone())
        torch.cuda.synchronize()
        finals.append([v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + scalars)
        assert "l_sinkhorn" not in eng.losses()
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_captured_sinkhorn_steps_equal_eager_ones_and_read_nothing_back():
    P = TR.step_problem(64, 64, 256, 11, masks=TC.step_masks(64, 64))
    rng = np.random.default_rng(5)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng, mask=cm)).to(DEV) for cm, _ in TC.step_masks(64, 64)]
           for _ in range(3)]
    finals = []
    for graph in (False, True):
        eng = _engine(P, deterministic=True)
        if graph:
            eng.capture_graph(idx[0])
        else:
            eng.step(idx[0])                  # workspaces take their size: the guarded steps below allocate nothing
            eng = _engine(P, deterministic=True)
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


def _cli_args(out, *extra):
    import run_strotss
    return run_strotss.build_parser().parse_args(
        [os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg"), "-o", str(out), "--max_size", "64",
         "--level", "1", "--max_iter", "30", "--log_every", "30"] + list(extra))


def test_cli_sinkhorn_run(tmp_path, monkeypatch):
    import run_strotss
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    outs, traces = {}, {}
    for tag, extra in (("remd", ()), ("sk_a", ("--style_transport", "sinkhorn")), ("sk_b", ("--style_transport", "sinkhorn"))):
        traces[tag] = []
        run_strotss.run(_cli_args(tmp_path / f"{tag}.jpg", *extra), trace=traces[tag])
        outs[tag] = open(tmp_path / f"{tag}.jpg", "rb").read()
        assert outs[tag][:2] == b"\xff\xd8"
    assert outs["sk_a"] == outs["sk_b"] and outs["sk_a"] != outs["remd"]
    steps = traces["sk_a"][0]["steps"]
    assert len(steps) == 30 and "l_sinkhorn" not in traces["remd"][0]["steps"][0]
    first, last = steps[0]["l_sinkhorn"], float(np.mean([s["l_sinkhorn"] for s in steps[-5:]]))
    report("cli:sinkhorn_first_last5", "64px", f"{first:.5f} {last:.5f}")
    assert last < first


def test_cli_sinkhorn_video(tmp_path):
    import run_strotss
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three synthetic frames of the colour test
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    run_strotss.run(run_strotss.build_parser().parse_args(
        [frames, style, "--video", "--compute_flow", "-o", str(tmp_path / "out"), "--max_size", "64", "--level", "1",
         "--max_iter", "10", "--style_transport", "sinkhorn", "--sinkhorn_iters", "10"]))
    stems = [os.path.splitext(os.path.basename(q))[0] for q in paths]
    assert len(stems) == 3 and sorted(os.listdir(tmp_path / "out")) == sorted(t + ".jpg" for t in stems)


# ------------------------------------------------------------------ the child process
def _child():
    from nn import _hip, _ops
    for c, l in CASES:
        ref_l, ref_g = SR.sinkhorn(c.x, c.y, "cosine", l, c.T)
        check_case(_ops, c, l, ref_l, ref_g)
    # what the library hands out in this process: no panels
    c = CASES[0][0]
    by = fbuf(c.y)
    nb = _hip.lib().strotss_selfsim_workspace_bytes(c.n, by.shape[1])
    ws = _ops.workspaces.get("selfsim", nb, by.device)
    rp, xp = C.c_void_p(), C.c_void_p()
    _hip.check(_hip.lib().strotss_selfsim_pred_panels(_hip.ptr(ws), nb, c.n, by.shape[1], C.byref(rp), C.byref(xp)), "panels")
    print(json.dumps({"cases": len(CASES), "panels": bool(xp.value)}))


if __name__ == "__main__":
    assert sys.argv[1:] == ["x3_off"]
    _child()
