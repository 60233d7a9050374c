"""The sliced Wasserstein style term on the GPU: strotss_sliced_cos_fwd_bwd against float64 autograd of
tests/_sliced_ref.py -- element by element at the tie-free, duplicate and sign cases of tests/_sliced_cases.py (searched at sort
widths 64 .. 256, constructed at 512 and 1024, where the same bits are also asked of three calls), in norm at the
full-shape cases, with x3 panels and with both panels NULL -- its output contract, counter, determinism and refusals; then
StepEngine(style_transport="sliced") against the float64 restatement of the step, the other transports' bits, graph capture
and the command line."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _sliced_cases as SC
import _sliced_ref as SR
import _transport_cases as TC
import _transport_ref as TR
from _loss_harness import DEV, LC_pad, SENTINEL, fbuf, report, run_entry
from _sinkhorn_ref import loss_tolerance
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EINVAL, EALIGN, ERANGE = -1, -2, -3
GSCALES = (1.0, 0.37)


@pytest.fixture(scope="module")
def ops():
    from nn import _ops
    return _ops


@functools.lru_cache(maxsize=None)
def ref64(label):
    c = SC.make_full(label) if label in SC.FULL_LABELS else SC.make_case(label)
    return SR.sliced(c.x, c.y, c.signs)


class Call:
    """the entry on one case: device rows, norms, panels, a workspace and a counter of its own"""

    def __init__(self, ops, c, panels=True):
        from nn import _hip
        self.lib, self.hip, self.c = _hip.lib(), _hip, c
        self.bx, self.by = fbuf(c.x), fbuf(c.y)
        self.rs, self.xs = ops.row_inv_norm_x3(self.bx, c.ns)
        self.rp, self.xp = ops.row_inv_norm_x3(self.by, c.n)
        if not panels:
            self.xs = self.xp = None
        self.ld = self.by.shape[1]
        self.nb = self.lib.strotss_sliced_workspace_bytes(c.ns, c.n, self.ld, c.n_proj)
        assert self.nb > 0
        self.ws = torch.full((self.nb,), 0xFF, dtype=torch.uint8, device=DEV)        # NaN bytes: a read before a write shows
        self.counter = torch.tensor([c.t], dtype=torch.int32, device=DEV)

    def __call__(self, gp, lo, gs=1.0, t=None, **kw):
        p = self.hip.ptr
        if t is not None:
            self.counter.fill_(t)
        a = dict(style=self.bx, rs=self.rs, xs=self.xs, ns=self.c.ns, pred=self.by, rp=self.rp, xp=self.xp, n=self.c.n,
                 d=self.c.d, ld=self.ld, n_proj=self.c.n_proj, counter=self.counter, gp=gp, lo=lo, ws=self.ws, nbytes=self.nb)
        a.update(kw)
        seed = self.c.seed & 0xFFFFFFFFFFFFFFFF
        return self.lib.strotss_sliced_cos_fwd_bwd(
            p(a["style"]), p(a["rs"]), p(a["xs"]), a["ns"], p(a["pred"]), p(a["rp"]), p(a["xp"]), a["n"], a["d"], a["ld"],
            a["n_proj"], seed & 0xFFFFFFFF, seed >> 32, p(a["counter"]), C.c_float(gs), p(a["gp"]), p(a["lo"]), p(a["ws"]),
            a["nbytes"], self.hip.stream_ptr())


def _run(ops, c, panels, gs, k):
    """run_entry's protocol (zero base, then a seeded base with sentinel padding) on a fresh counter value each call"""
    call = Call(ops, c, panels)

    def fn(gp, lo):
        assert call(gp, lo[0], gs, t=c.t) == 0
    ref_g = ref64(c.label)[1]
    got, loss, g0 = run_entry(ops, fn, c.n, c.d, max(np.abs(ref_g).max(), 1e-3) * gs, 70 + k)
    assert int(call.counter.item()) == c.t + 1, "the counter reads t + 1 after a call"
    assert not loss.flatten()[1:].any()
    return got, loss[0, 0], g0


@pytest.mark.parametrize("panels", (True, False), ids=("x3", "f32"))
@pytest.mark.parametrize("label", SC.ELEMENTWISE)
def test_entry_matches_float64_element_by_element(ops, label, panels):
    c = SC.make_case(label)
    ref_l, ref_g = ref64(label)
    tol = SR.TOL_GRAD[SR.family(c)]
    losses = []
    for k, gs in enumerate(GSCALES):
        got, loss, g0 = _run(ops, c, panels, gs, k)
        rel = abs(loss - ref_l) / abs(ref_l)
        report(f"scalar:sliced:g{gs}", label, f"{rel:.3e}")
        assert rel <= loss_tolerance(c, 0.0), (loss, ref_l)
        for name, g in ((f"sliced:g{gs}", got / gs), (f"sliced:g{gs}:zero_base", g0.astype(np.float64) / gs)):
            err = SR.err_over_max(g, ref_g)
            report(f"grad:{name}", label, f"max {err:.3e} of tol {tol:.3e}")
            assert np.isfinite(g).all() and (np.abs(g - ref_g) <= tol * np.abs(ref_g).max()).all(), (name, err, tol)
        losses.append(loss)
    assert losses[0] == losses[1], "the loss depends on gscale"


@pytest.mark.parametrize("panels", (True, False), ids=("x3", "f32"))
@pytest.mark.parametrize("label", SC.FULL_LABELS)
def test_entry_matches_float64_in_norm_at_full_shapes(ops, label, panels):
    c = SC.make_full(label)
    ref_l, ref_g = ref64(label)
    got, loss, g0 = _run(ops, c, panels, 1.0, 0)
    rel = abs(loss - ref_l) / abs(ref_l)
    report("scalar:sliced", label, f"{rel:.3e}")
    assert rel <= loss_tolerance(c, 0.0), (loss, ref_l)
    for name, g in (("sliced", got), ("sliced:zero_base", g0.astype(np.float64))):
        err = SR.rel_fro(g, ref_g)
        report(f"grad_fro:{name}", label, f"{err:.3e} of tol {SR.TOL_FRO[label]:.3e}")
        assert np.isfinite(g).all() and err <= SR.TOL_FRO[label], (name, err)


def _zero_out(c):
    return (torch.zeros((LC_pad(c.n), LC_pad(c.d)), dtype=torch.float32, device=DEV),
            torch.zeros(4, dtype=torch.float32, device=DEV))


@pytest.mark.parametrize("panels", (True, False), ids=("x3", "f32"))
@pytest.mark.parametrize("label", SC.CONSTRUCTED)
def test_wide_sorts_give_the_same_bits_three_times(ops, label, panels):
    """widths 512 and 1024 (six and ten cross-wave stages on two alternating LDS buffers): twice from fresh NaN-byte
    workspaces and once more on the workspace the second call left.  A buffer reused a stage early or a missing barrier shows as
    a changed bit before it shows as a wrong rank"""
    c = SC.make_case(label)
    assert SC.width(c.n, c.ns) in (512, 1024)
    outs, call = [], None
    for fresh in (True, True, False):
        if fresh:
            call = Call(ops, c, panels)
        g, lo = _zero_out(c)
        assert call(g, lo, t=c.t) == 0
        torch.cuda.synchronize()
        outs.append((g, lo))
    g0, l0 = outs[0]
    assert bool(torch.isfinite(g0).all()) and bool(g0[:c.n, :c.d].any()) and float(l0[0]) > 0
    for g, lo in outs[1:]:
        assert torch.equal(g, g0) and torch.equal(lo, l0)


def test_contract_accumulation_padding_counter_and_bits(ops):
    c = SC.make_case("n65_ns40_p4")                        # ld = 64 holds d = 35: 29 pad columns; rows 65 .. 95 past the end
    call = Call(ops, c)
    g0, l0 = _zero_out(c)
    assert call(g0, l0) == 0
    torch.cuda.synchronize()
    assert int(call.counter.item()) == c.t + 1
    assert not bool(g0[c.n:].any()) and bool(g0[:c.n, :c.d].any())
    pad = g0[:c.n, c.d:]
    assert not bool(pad.any()) and not bool(torch.signbit(pad).any()), "pad columns of rows < n receive +0"
    # the same counter value: the same bits, again and on a second stream; accumulation is one rounding of base + gradient
    base = torch.full_like(g0, SENTINEL)
    base[:c.n, :c.d] = torch.as_tensor(np.random.default_rng(3).standard_normal((c.n, c.d)), dtype=torch.float32, device=DEV)
    g1, l1 = base.clone(), torch.zeros_like(l0)
    assert call(g1, l1, t=c.t) == 0
    g2, l2 = _zero_out(c)
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert call(g2, l2, t=c.t) == 0
    torch.cuda.synchronize()
    assert torch.equal(g2, g0) and torch.equal(l2, l0)
    assert torch.equal(g1[:c.n, :c.d], (base + g0)[:c.n, :c.d]) and torch.equal(l1, l0)
    assert torch.equal(g1[c.n:], base[c.n:]) and torch.equal(g1[:c.n, c.d:], base[:c.n, c.d:] + 0.0)
    # another counter value: other directions, another loss -- the one the host twin's directions give
    g3, l3 = _zero_out(c)
    assert call(g3, l3, t=c.t + 1) == 0
    torch.cuda.synchronize()
    assert int(call.counter.item()) == c.t + 2 and float(l3[0]) != float(l0[0])
    from nn import rand
    ref_l, ref_g = SR.sliced(c.x, c.y, rand.sliced_signs(c.seed, c.t + 1, c.n_proj, c.d))
    assert abs(float(l3[0]) - ref_l) <= 5e-5 * abs(ref_l)
    assert SR.err_over_max(g3[:c.n, :c.d].double().cpu().numpy(), ref_g) <= SR.TOL_GRAD["wide"]


def test_the_device_draws_the_host_twins_signs(ops):
    """d = 3, n = ns = 1: with x = (1, 2, 4) / sqrt(21) and the style row (1, 0, 0), a = <eps, x> takes eight distinct values
    up to sign and b = eps_0, so the loss (a - b)^2 / 2 tells the three signs of every draw (up to their common sign, under
    which the term is invariant)"""
    from nn import rand
    x, y = np.array([[1.0, 0.0, 0.0]]), np.array([[1.0, 2.0, 4.0]])
    c = SC.Case("signs", 1, 1, 3, 1, "plain", 0x1234567890, x, y, 0)
    call = Call(ops, c)
    g, lo = _zero_out(c)
    for t in range(12):
        assert call(g, lo, t=t) == 0
        torch.cuda.synchronize()
        e = rand.sliced_signs(c.seed, t, 1, 3)[0].astype(np.float64)
        want = 0.5 * (float(e @ y[0]) / np.sqrt(21.0) - e[0]) ** 2
        assert abs(float(lo[0]) - want) <= 1e-5 * max(want, 1e-3), (t, float(lo[0]), want, e)
    assert len({tuple(rand.sliced_signs(c.seed, t, 1, 3)[0]) for t in range(12)}) > 2


def test_refusals_leave_outputs_workspace_and_counter_untouched(ops):
    c = SC.make_case("n65_ns40_p4")
    call = Call(ops, c)
    lib = call.lib
    g = torch.full((LC_pad(c.n), LC_pad(c.d)), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    call.ws.fill_(0x5A)
    by48 = torch.zeros((LC_pad(c.n), 48), dtype=torch.float32, device=DEV)
    q = lib.strotss_sliced_workspace_bytes
    assert q(0, 1, 64, 1) == 0 and q(1, 1025, 64, 1) == 0 and q(1, 1, 48, 1) == 0 and q(1, 1, 64, 1025) == 0 and q(1, 1, 64, 0) == 0
    r = lambda gp=g, lo=loss, **kw: call(gp, lo, **kw)
    assert r(style=None) == EINVAL and r(rs=None) == EINVAL and r(pred=None) == EINVAL and r(rp=None) == EINVAL
    assert r(counter=None) == EINVAL and r(gp=None) == EINVAL and r(lo=None) == EINVAL and r(ws=None) == EINVAL
    assert r(ns=0) == EINVAL and r(n=0) == EINVAL and r(d=0) == EINVAL and r(n_proj=0) == EINVAL and r(n=-3) == EINVAL
    assert r(d=call.ld + 1) == EINVAL and r(nbytes=call.nb - 1) == EINVAL
    assert r(xs=None) == EINVAL and r(xp=None) == EINVAL                      # the panels come as a pair
    assert r(pred=by48, ld=48) == EALIGN
    big = lib.strotss_sliced_workspace_bytes(1024, 1024, call.ld, 1024)
    assert r(n=1025, nbytes=big) == ERANGE and r(ns=1025, nbytes=big) == ERANGE and r(n_proj=1025, nbytes=big) == ERANGE
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((loss == SENTINEL).all()) and bool((call.ws == 0x5A).all())
    assert int(call.counter.item()) == c.t
    assert r() == 0 and r(xs=None, xp=None) == 0                              # the same arguments unspoiled are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g[:c.n]).all()) and bool((loss[1:] == SENTINEL).all()) and float(loss[0]) != SENTINEL
    assert int(call.counter.item()) == c.t + 2


# ------------------------------------------------------------------ the step
def _engine(P, transport="sliced", blend_weights=None, deterministic=None, **kw):
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
    if transport == "sliced":
        kw = dict(dict(sliced_projections=SC.STEP_PROJECTIONS, sliced_seed=SC.STEP_SEED), **kw)
    if transport is not None:
        kw["style_transport"] = transport
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic, **kw)


def _check_step(P, blend_weights=None):
    import test_hip_engine as THE
    eng = _engine(P, blend_weights=blend_weights)
    eng.forward_backward([torch.from_numpy(i).to(DEV) for i in P["idx"]])
    torch.cuda.synchronize()
    calls = sum(len(s) if blend_weights is not None else 1 for s in P["s_idx"])
    assert int(eng._sliced_counter.item()) == calls
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(P["weights"], dtype=torch.float64)), eng)
    ref = SR.reference_step(P, SC.STEP_PROJECTIONS, SC.STEP_SEED, blend_weights=blend_weights, vgg=vgg)
    got = eng.losses()
    assert got["l_sliced"] == got["l_remd"] > 0
    for k in ("loss", "loss_c", "loss_s"):
        rel = abs(got[k] - float(ref[k])) / max(1.0, abs(float(ref[k])))
        report(f"step:{k}", f"{eng.h}x{eng.w}", f"{rel:.3e}")
        assert rel < SR.TOL_SCALAR, (k, got[k], float(ref[k]))
    for k, (g, gr) in enumerate(zip(eng.gvars, ref["grads"])):
        rel = float((g.cpu().double() - gr).norm() / gr.norm())
        report(f"step:grad_level{k}", f"{eng.h}x{eng.w}", f"{rel:.3e}")
        assert rel < SR.GRAD_TOL, (k, rel)


@pytest.mark.parametrize("spec", SC.STEPS, ids=[s[0] for s in SC.STEPS])
def test_sliced_step_matches_the_float64_restatement(spec):
    _, h, w, n, seed, masked = spec
    _check_step(TR.step_problem(h, w, n, seed, masks=TC.step_masks(h, w) if masked else None))


def test_sliced_blend_step_matches_the_float64_restatement():
    _check_step(TR.step_problem(*SC.BLEND_STEP[1:5], n_styles=2), blend_weights=SC.BLEND_WEIGHTS)


def test_engine_refuses_what_the_term_does_not_run_with():
    from nn import engine
    P = TR.step_problem(64, 64, 128, 1)
    for kw in (dict(sliced_projections=0), dict(sliced_projections=1025), dict(sliced_projections=2.5),
               dict(sliced_projections=True), dict(dist_group=object())):
        with pytest.raises(ValueError):
            _engine(P, **kw)
    with pytest.raises(ValueError):
        engine.check_style_transport("sliced", 10.0, 30, 0)
    engine.check_style_transport("sliced", 10.0, 30)
    engine.check_style_transport("sliced", 10.0, 30, 1024)


@pytest.mark.parametrize("transport", ("remd", "sinkhorn"))
def test_other_transports_keep_their_bits_with_the_new_keywords(transport):
    from nn import engine
    P = TR.step_problem(64, 64, 256, 9)
    rng = np.random.default_rng(4)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng)).to(DEV)] for _ in range(2)]
    finals = []
    for kw in ({}, dict(sliced_projections=engine.DEFAULT_SLICED_PROJECTIONS, sliced_seed=0)):
        eng = _engine(P, transport=None if (transport == "remd" and not kw) else transport, deterministic=True, **kw)
        assert eng._sliced_counter is None
        scalars = []
        for i in idx:
            eng.step(i)
            scalars.append(eng.scalars.clone())
        torch.cuda.synchronize()
        finals.append([v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + scalars)
        assert "l_sliced" not in eng.losses()
    for a, b in zip(*finals):
        assert torch.equal(a, b)


def test_captured_sliced_steps_equal_eager_ones(monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    P = TR.step_problem(64, 64, 256, 11, masks=TC.step_masks(64, 64))
    rng = np.random.default_rng(5)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, 256, rng, mask=cm)).to(DEV) for cm, _ in TC.step_masks(64, 64)]
           for _ in range(3)]
    finals = []
    for graph in (False, True):
        eng = _engine(P, deterministic=True)
        if graph:
            eng.capture_graph(idx[0])
            assert int(eng._sliced_counter.item()) == 0, "warm-up and capture leave the draw number where it was"
        for i in idx:
            eng.step(i)
        torch.cuda.synchronize()
        assert int(eng._sliced_counter.item()) == 3 * 2, "3 steps x (2 regions x 1 style) calls"
        finals.append([v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()])
    for a, b in zip(*finals):
        assert torch.equal(a, b), "eager vs graph replay"


# ------------------------------------------------------------------ the command line
GOLDEN = os.path.join(ROOT, "tests", "golden")


def _cli_args(out, *extra):
    import run_strotss
    return run_strotss.build_parser().parse_args(
        [os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg"), "-o", str(out), "--max_size", "64",
         "--level", "1", "--max_iter", "10", "--log_every", "10"] + list(extra))


def test_cli_sliced_run(tmp_path, monkeypatch):
    import run_strotss
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    sliced = ("--style_transport", "sliced", "--sliced_projections", "32")
    outs, traces = {}, {}
    for tag, extra in (("remd", ()), ("sw_a", sliced), ("sw_b", sliced)):
        traces[tag] = []
        run_strotss.run(_cli_args(tmp_path / f"{tag}.jpg", *extra), trace=traces[tag])
        outs[tag] = open(tmp_path / f"{tag}.jpg", "rb").read()
        assert outs[tag][:2] == b"\xff\xd8"
    assert outs["sw_a"] == outs["sw_b"] and outs["sw_a"] != outs["remd"]
    steps = traces["sw_a"][0]["steps"]
    assert len(steps) == 10 and "l_sliced" in steps[0] and "l_sliced" not in traces["remd"][0]["steps"][0]


def test_cli_sliced_video(tmp_path):
    import run_strotss
    from PIL import Image
    from test_hip_color import _moved_frames, _texture          # the three synthetic frames of the colour test
    frames = str(tmp_path / "frames")
    paths = _moved_frames(frames)
    style = str(tmp_path / "style.jpg")
    Image.fromarray((_texture(56, 60, 7, (0.3, 0.5, 1.0)) * 255).astype(np.uint8)).save(style, quality=95)
    run_strotss.run(run_strotss.build_parser().parse_args(
        [frames, style, "--video", "--compute_flow", "-o", str(tmp_path / "out"), "--max_size", "64", "--level", "1",
         "--max_iter", "10", "--style_transport", "sliced", "--sliced_projections", "32"]))
    stems = [os.path.splitext(os.path.basename(q))[0] for q in paths]
    assert len(stems) == 3 and sorted(os.listdir(tmp_path / "out")) == sorted(t + ".jpg" for t in stems)
