"""The sliced palette term on the GPU: strotss_palette_sliced_fwd_bwd against the float64 restatement of
tests/_palette_sliced_ref.py -- element by element at the tie-free and duplicate cases of tests/_palette_sliced_cases.py
(searched at sort widths 64 and 128, constructed at 256, 512 and 1024, where the same bits are also asked of three calls and
the whole-number coefficients of one direction are recovered), in
norm at the full-shape cases -- its output contract, determinism and refusals; then StepEngine(palette_transport="sliced")
against the float64 restatement of the step (tests/_palette_step_cases.py), graph capture, the bits of the default engine and
the command line."""
import ctypes as C
import functools
import os

import numpy as np
import pytest
import torch

import _palette_sliced_cases as PC
import _palette_sliced_ref as PR
import _palette_step_cases as PS
import _step_cases as SC
from oracle import strotss_oracle as O

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda"
EINVAL, EALIGN, ERANGE = -1, -2, -3
SENTINEL = 7.25
GSCALES = (1.0, 0.37)


def pad32(v):
    return (v + 31) // 32 * 32


def rows(x, ld):
    """(pad32(m), ld) device rows: the colours in the first three columns, NaN everywhere else (a read of it shows)"""
    m = x.shape[0]
    b = torch.full((pad32(m), ld), float("nan"), dtype=torch.float32, device=DEV)
    b[:m, :3] = torch.as_tensor(x, dtype=torch.float32, device=DEV)
    return b


@functools.lru_cache(maxsize=None)
def ref64(label):
    c = PC.case_of(label)
    return PR.palette_sliced(c.x, c.y, c.dirs, c.rgb_to_yuv)


class Call:
    """the entry on one case: device rows, directions and a workspace of its own, filled with NaN bytes"""

    def __init__(self, c):
        from nn import _hip
        self.lib, self.hip, self.c = _hip.lib(), _hip, c
        self.style, self.pred = rows(c.x, c.ld), rows(c.y, c.ld)
        self.dirs = torch.from_numpy(c.dirs).to(DEV).contiguous()
        self.nb = self.lib.strotss_palette_sliced_workspace_bytes(c.ns, c.n, c.n_proj)
        assert self.nb > 0
        self.ws = torch.full((self.nb,), 0xFF, dtype=torch.uint8, device=DEV)

    def zeros(self):
        return (torch.zeros((pad32(self.c.n), self.c.ld), dtype=torch.float32, device=DEV),
                torch.zeros(4, dtype=torch.float32, device=DEV))

    def __call__(self, gp, lo, gs=1.0, **kw):
        p = self.hip.ptr
        a = dict(style=self.style, ns=self.c.ns, pred=self.pred, n=self.c.n, ld=self.c.ld, convert=self.c.rgb_to_yuv,
                 dirs=self.dirs, n_proj=self.c.n_proj, gp=gp, lo=lo, ws=self.ws, nbytes=self.nb)
        a.update(kw)
        return self.lib.strotss_palette_sliced_fwd_bwd(p(a["style"]), a["ns"], p(a["pred"]), a["n"], a["ld"], a["convert"],
                                                       p(a["dirs"]), a["n_proj"], C.c_float(gs), p(a["gp"]), p(a["lo"]),
                                                       p(a["ws"]), a["nbytes"], self.hip.stream_ptr())


def _run(c, gs):
    """one call into zeros: (gradient [:n, :3] as float64, loss); everything else of the outputs must still be zero"""
    call = Call(c)
    gp, lo = call.zeros()
    assert call(gp, lo, gs) == 0
    torch.cuda.synchronize()
    assert not bool(gp[c.n:].any()) and not bool(gp[:, 3:].any()) and not bool(lo[1:].any())
    g = gp[:c.n, :3].double().cpu().numpy()
    assert np.isfinite(g).all()
    return g, float(lo[0])


@pytest.mark.parametrize("label", PC.ELEMENTWISE)
def test_entry_matches_float64_element_by_element(label):
    c = PC.make_case(label)
    ref_l, ref_g = ref64(label)
    tol = PR.TOL_GRAD[PR.family(c)]
    losses = []
    for gs in GSCALES:
        g, loss = _run(c, gs)
        rel = abs(loss - ref_l) / abs(ref_l)
        err = PR.err_over_max(g / gs, ref_g)
        print(f"MEASURE palette_sliced g{gs} {label} loss {rel:.3e} grad max {err:.3e} of tol {tol:.3e}")
        assert rel <= PR.LOSS_TOL, (loss, ref_l)
        assert (np.abs(g / gs - ref_g) <= tol * np.abs(ref_g).max()).all(), (err, tol)
        losses.append(loss)
    assert losses[0] == losses[1], "the loss depends on gscale"


@pytest.mark.parametrize("label", PC.FULL_LABELS)
def test_entry_matches_float64_in_norm_at_full_shapes(label):
    c = PC.make_full(label)
    ref_l, ref_g = ref64(label)
    g, loss = _run(c, 1.0)
    rel, err = abs(loss - ref_l) / abs(ref_l), PR.rel_fro(g, ref_g)
    print(f"MEASURE palette_sliced {label} loss {rel:.3e} grad_fro {err:.3e} of tol {PR.TOL_FRO[label]:.3e}")
    assert rel <= PR.LOSS_TOL, (loss, ref_l)
    assert err <= PR.TOL_FRO[label], err


@pytest.mark.parametrize("label", PC.CONSTRUCTED)
def test_wide_sorts_give_the_same_bits_three_times(label):
    """widths 256, 512 and 1024 (three, six and ten cross-wave stages on two alternating LDS buffers): twice from fresh
    NaN-byte workspaces and once more on the workspace the second call left.  A buffer reused a stage early or a missing barrier
    shows as a changed bit before it shows as a wrong rank"""
    c = PC.make_case(label)
    assert PC.width(c.n, c.ns) in (256, 512, 1024)
    outs, call = [], None
    for fresh in (True, True, False):
        if fresh:
            call = Call(c)
        g, lo = call.zeros()
        assert call(g, lo) == 0
        torch.cuda.synchronize()
        outs.append((g, lo))
    g0, l0 = outs[0]
    assert bool(torch.isfinite(g0).all()) and bool(g0[:c.n, :3].any()) and float(l0[0]) > 0
    for g, lo in outs[1:]:
        assert torch.equal(g, g0) and torch.equal(lo, l0)


def test_coefficients_at_full_width_are_the_restatements_whole_numbers():
    """1024 x 1024, P = 1, no YUV, the points on a line along the direction: a row's gradient is (2 / sqrt(3)) K / (n ns) times
    the direction with K a whole number (a sum of +-len).  K recovered from either non-zero component equals the
    restatement's to 0.5; float32 division costs about n ns 2^-24 = 0.06"""
    c = PC.make_case(PC.INTEGER_LABEL)
    assert (c.n, c.ns, c.n_proj, c.rgb_to_yuv) == (1024, 1024, 1, 0)
    _, ref_g = ref64(c.label)
    g, _ = _run(c, 1.0)
    theta = c.dirs[0].astype(np.float64)
    live = [k for k in range(3) if abs(theta[k]) > 0.1]
    assert len(live) >= 2
    for k in live:
        unit = c.n * c.ns / (2.0 / np.sqrt(3.0) * theta[k])
        want = ref_g[:, k] * unit
        assert np.abs(want - np.rint(want)).max() <= 1e-6 and set(np.abs(np.rint(want))) == {float(c.n)}
        worst = np.abs(g[:, k] * unit - np.rint(want)).max()
        print(f"MEASURE palette_sliced whole numbers {c.label} component {k}: worst {worst:.3e} of 0.5")
        assert worst <= 0.5
    for k in set(range(3)) - set(live):
        assert not g[:, k].any()


def test_packed_rgb_rows_are_taken_as_the_relaxed_emd_entry_takes_them():
    """ld = 3: no alignment is asked of the row stride (strotss_palette_remd_fwd_bwd asks none either)"""
    c0 = PC.make_case("n65_ns33_p8")
    c = PC.Case("packed", c0.n, c0.ns, c0.n_proj, 3, c0.rgb_to_yuv, c0.kind, c0.x, c0.y, c0.seed, c0.row_seed)
    ref_l, ref_g = ref64("n65_ns33_p8")
    g, loss = _run(c, 1.0)
    assert abs(loss - ref_l) <= PR.LOSS_TOL * abs(ref_l)
    assert (np.abs(g - ref_g) <= PR.TOL_GRAD[PR.family(c)] * np.abs(ref_g).max()).all()


def test_equal_sets_give_zero_loss_and_zero_coefficients():
    call = Call(PC.equal_case())
    gp, lo = call.zeros()
    lo.fill_(SENTINEL)
    assert call(gp, lo) == 0
    torch.cuda.synchronize()
    assert float(lo[0]) == 0.0 and not bool(gp.any()) and bool((lo[1:] == SENTINEL).all())


def test_contract_accumulation_untouched_parts_gscale_and_bits():
    c = PC.make_case("n65_ns33_p8")                        # ld = 2208; rows 65 .. 95 past the end
    call = Call(c)
    g0, l0 = call.zeros()
    assert call(g0, l0) == 0
    torch.cuda.synchronize()
    assert bool(g0[:c.n, :3].any())
    # a filled gpred with a tail past it: contents plus the gradient bit for bit, everything else untouched
    rows_, tail = pad32(c.n), 4096
    flat = torch.full((rows_ * c.ld + tail,), SENTINEL, dtype=torch.float32, device=DEV)
    g1 = flat[:rows_ * c.ld].view(rows_, c.ld)
    g1[:c.n, :3] = torch.as_tensor(np.random.default_rng(3).standard_normal((c.n, 3)) * float(g0.abs().max()),
                                   dtype=torch.float32, device=DEV)
    base = flat.clone()
    l1 = torch.zeros_like(l0)
    assert call(g1, l1) == 0
    torch.cuda.synchronize()
    b1 = base[:rows_ * c.ld].view(rows_, c.ld)
    assert torch.equal(g1[:c.n, :3], (b1 + g0)[:c.n, :3]) and torch.equal(l1, l0)
    assert torch.equal(g1[c.n:], b1[c.n:]) and torch.equal(g1[:, 3:], b1[:, 3:])
    assert torch.equal(flat[rows_ * c.ld:], base[rows_ * c.ld:])
    # again, and on a second stream: the same bits
    g2, l2 = call.zeros()
    assert call(g2, l2) == 0
    g3, l3 = call.zeros()
    side = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        assert call(g3, l3) == 0
    torch.cuda.synchronize()
    assert torch.equal(g2, g0) and torch.equal(l2, l0) and torch.equal(g3, g0) and torch.equal(l3, l0)
    # gscale = 0 adds nothing and still reports the loss; a negative gscale mirrors the gradient exactly
    g4, l4 = b1.clone(), torch.zeros_like(l0)
    assert call(g4, l4, 0.0) == 0
    g5, l5 = call.zeros()
    assert call(g5, l5, -1.0) == 0
    g6, l6 = call.zeros()
    assert call(g6, l6, -0.37) == 0
    g7, l7 = call.zeros()
    assert call(g7, l7, 0.37) == 0
    torch.cuda.synchronize()
    assert torch.equal(g4, b1) and torch.equal(l4, l0)
    assert torch.equal(g5, -g0) and torch.equal(g6, -g7) and torch.equal(l5, l0) and torch.equal(l6, l0)


def test_refusals_leave_outputs_and_workspace_untouched():
    c = PC.make_case("n65_ns33_p1")
    call = Call(c)
    lib = call.lib
    g = torch.full((pad32(c.n), c.ld), SENTINEL, dtype=torch.float32, device=DEV)
    loss = torch.full((4,), SENTINEL, dtype=torch.float32, device=DEV)
    call.ws.fill_(0x5A)
    q = lib.strotss_palette_sliced_workspace_bytes
    assert q(1024, 1024, 1024) > 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-2, 1, 1), (1025, 1, 1), (1, 1025, 1), (1, 1, 1025)):
        assert q(*bad) == 0, bad
    r = lambda gp=g, lo=loss, **kw: call(gp, lo, **kw)
    assert r(style=None) == EINVAL and r(pred=None) == EINVAL and r(dirs=None) == EINVAL and r(gp=None) == EINVAL
    assert r(lo=None) == EINVAL and r(ws=None) == EINVAL
    assert r(ns=0) == EINVAL and r(n=0) == EINVAL and r(n=-3) == EINVAL and r(n_proj=0) == EINVAL and r(n_proj=-1) == EINVAL
    assert r(ld=2) == EINVAL and r(ld=0) == EINVAL and r(nbytes=call.nb - 1) == EINVAL and r(nbytes=0) == EINVAL
    big = q(1024, 1024, 1024)
    assert r(n=1025, nbytes=big) == ERANGE and r(ns=1025, nbytes=big) == ERANGE and r(n_proj=1025, nbytes=big) == ERANGE
    torch.cuda.synchronize()
    assert bool((g == SENTINEL).all()) and bool((loss == SENTINEL).all()) and bool((call.ws == 0x5A).all())
    assert r() == 0                                                           # the same arguments unspoiled are accepted
    torch.cuda.synchronize()
    assert bool(torch.isfinite(g).all()) and bool((loss[1:] == SENTINEL).all()) and float(loss[0]) != SENTINEL
    assert bool((g[c.n:] == SENTINEL).all()) and bool((g[:, 3:] == SENTINEL).all())


# ------------------------------------------------------------------ the step
def _engine(lb, deterministic=None, palette="sliced", **kw):
    """test_hip_step_combos._engine with the palette keywords"""
    from nn import _ops, engine
    from nn.model import VGGParams
    row, P = PS.ROWS[lb], PS.problem(lb)
    params = VGGParams(P["weights"], '16', None, DEV)
    cfeat = engine.extract_features(params, P["content"].to(DEV))
    sfeats = [engine.extract_features(params, s.to(DEV)) for s in P["styles"]]
    bw = SC.blend_of(row)
    targets = []
    for sets in P["s_idx"]:
        ts = [engine.StyleTarget.build(_ops.hypercol_gather(sf, torch.from_numpy(si).to(DEV), False), si.shape[0], 2179)
              for sf, si in zip(sfeats, sets)]
        targets.append(ts[0] if bw is None else engine.StyleBlend(ts, list(bw)))
    c64, s64 = P["content"].double(), P["styles"][0].double()
    init = O.make_laplacian(c64) + s64.mean(dim=(1, 2), keepdim=True)
    tr = SC.transport_of(row)
    kw = dict(kw, style_transport=tr[0])
    if tr[0] == "sliced":
        kw.update(sliced_projections=tr[1], sliced_seed=tr[2])
    if palette is not None:
        kw.update(palette_transport=palette)
        if palette == "sliced":
            kw.update(palette_projections=PS.PROJECTIONS)
    return engine.StepEngine(params, cfeat, targets, init.float().to(DEV), P["alpha"], P["denom"], 2e-3,
                             sample_size=P["n_samples"], deterministic=deterministic,
                             content_weight=None if P["wmap"] is None else P["wmap"].to(DEV), **kw)


def _indices(lb):
    return [torch.from_numpy(i).to(DEV) for i in PS.problem(lb)["idx"]]


@pytest.mark.parametrize("lb", PS.LABELS)
def test_step_matches_the_float64_restatement(lb):
    import test_hip_engine as THE
    eng = _engine(lb)
    eng.forward_backward(_indices(lb))
    torch.cuda.synchronize()
    vgg = THE._oracle_vgg(dict(vgg=O.VGG(PS.problem(lb)["weights"], dtype=torch.float64)), eng)
    ref = PS.reference_step(lb, vgg=vgg)
    got = dict(eng.losses())
    got["grads"] = [g.detach().cpu().double() for g in eng.gvars]
    assert got["l_palette_sliced"] == got["l_palette"] > 0
    sc, gr = PS.step_distance(got, ref)
    for k in PS.SCALARS:
        print(f"MEASURE step:{k} {lb} {abs(got[k] - float(ref[k])) / max(1.0, abs(float(ref[k]))):.3e}")
    print(f"MEASURE step:grad {lb} {gr:.3e}")
    assert sc < PS.TOL_SCALAR and gr < PS.GRAD_TOL, (sc, gr)


def _state(eng):
    return [v.clone() for v in eng.variables] + [g.clone() for g in eng.gvars] + [eng.scalars.clone()]


@pytest.mark.parametrize("lb", ["remd-regions-map-t0-64x64", "sliced-blend-nomap-t0-64x64"])
def test_captured_steps_equal_eager_ones(lb, monkeypatch):
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    row, P = PS.ROWS[lb], PS.problem(lb)
    (h, w), n = row[4], P["n_samples"]
    cmasks = [None] if SC.masks_of(row) is None else [cm for cm, _ in SC.masks_of(row)]
    rng = np.random.default_rng(5)
    idx = [_indices(lb)] + [[torch.from_numpy(O.make_indices(h, w, True, n, rng, mask=cm)).to(DEV) for cm in cmasks]
                            for _ in range(2)]
    finals = []
    for graph in (False, True):
        eng = _engine(lb, deterministic=True)
        if graph:
            eng.capture_graph(idx[0])
        for i in idx:
            eng.step(i)
        torch.cuda.synchronize()
        finals.append((_state(eng), eng.losses()))
    assert finals[0][1] == finals[1][1]
    for a, b in zip(finals[0][0], finals[1][0]):
        assert torch.equal(a, b), "eager vs graph replay"


def test_remd_engine_keeps_the_bits_of_one_built_without_the_argument():
    lb = "remd-one-nomap-t0-64x64"
    rng = np.random.default_rng(4)
    idx = [[torch.from_numpy(O.make_indices(64, 64, True, PS.problem(lb)["n_samples"], rng)).to(DEV)] for _ in range(2)]
    finals = []
    for palette in (None, "remd", "sliced"):
        eng = _engine(lb, deterministic=True, palette=palette)
        assert (eng._palette_dirs is not None) == (palette == "sliced")
        for i in idx:
            eng.step(i)
        torch.cuda.synchronize()
        finals.append(_state(eng))
        assert ("l_palette_sliced" in eng.losses()) == (palette == "sliced")
    for a, b in zip(finals[0], finals[1]):
        assert torch.equal(a, b)
    assert not torch.equal(finals[0][0], finals[2][0]), "the sliced term is another loss"


def test_engine_refuses_what_the_term_does_not_run_with():
    lb = "remd-one-nomap-t0-64x64"
    for kw in (dict(palette_projections=0), dict(palette_projections=1025), dict(palette_projections=2.5),
               dict(palette_projections=True), dict(dist_group=object())):
        with pytest.raises(ValueError):
            _engine(lb, palette=None, palette_transport="sliced", **kw)
    with pytest.raises(ValueError):
        _engine(lb, palette=None, palette_transport="sinkhorn")


# ------------------------------------------------------------------ the command line
GOLDEN = os.path.join(ROOT, "tests", "golden")


def test_cli_run_with_the_sliced_palette_term(tmp_path, monkeypatch):
    import run_strotss
    monkeypatch.setenv("STROTSS_DETERMINISTIC", "1")
    base = [os.path.join(GOLDEN, "content_im.jpg"), os.path.join(GOLDEN, "style_im.jpg"), "--max_size", "64", "--level", "1",
            "--max_iter", "10", "--log_every", "10"]
    pal = ["--palette_transport", "sliced", "--palette_projections", "32"]
    outs, traces = {}, {}
    for tag, extra in (("remd", []), ("pal_a", pal), ("pal_b", pal), ("pal_sliced", pal + ["--style_transport", "sliced",
                                                                                         "--sliced_projections", "32"])):
        traces[tag] = []
        run_strotss.run(run_strotss.build_parser().parse_args(base + ["-o", str(tmp_path / f"{tag}.jpg")] + extra),
                        trace=traces[tag])
        outs[tag] = open(tmp_path / f"{tag}.jpg", "rb").read()
        assert outs[tag][:2] == b"\xff\xd8"
    assert outs["pal_a"] == outs["pal_b"] and outs["pal_a"] != outs["remd"] and outs["pal_sliced"] != outs["pal_a"]
    steps = traces["pal_a"][0]["steps"]
    assert len(steps) == 10 and all(s["l_palette_sliced"] > 0 for s in steps)
    assert "l_palette_sliced" not in traces["remd"][0]["steps"][0]
    assert "l_sliced" in traces["pal_sliced"][0]["steps"][0] and "l_palette_sliced" in traces["pal_sliced"][0]["steps"][0]
